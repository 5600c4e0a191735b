// bam_resort.hpp — FADEHIP_BAM_KEEP_SORTED: the clipped output of a coordinate-sorted input stays in coordinate order.
// A hard clip only moves a record's pos up (a left clip), leaves it (a right clip) or resets the record, which then counts
// as unmapped; so a written record can only be overtaken by records that come a little later, and holding a small tail back
// on the device until the input has passed it gives coordinate order as the file streams through.
//
//   key   (refID as u32) << 32 | (pos + 1 as u32) of the record as it leaves; a reset record: RS_KEY_UNMAPPED
//   W     the key AS IT CAME IN of the call's last record (the last call: all ones)
//   call  {held over} u {the call's records}, stably sorted by key; the records with key <= W are a prefix of that order and
//         leave, the rest is held.  Held-over records carry the lower indices, so ties keep stream order.
//
// The sort is a stable LSD radix sort of all of the call's items, eight passes of eight bits (histogram per tile, one scan,
// scatter by rank): linear in the items whatever share of them is displaced.  All kernels here are new; a run without the
// flag launches none of them, and fadehip_coord_order_batch runs the same sort over records the caller brings.
#pragma once
#include "bam_device.hpp"
#include "bam_from_tags.hpp"

namespace fadehip {
namespace bam {

constexpr uint64_t RS_KEY_UNMAPPED = 0xffffffff00000000ull;  // refID -1, pos -1: where a reset record sorts
constexpr uint64_t RS_FROM_HOLD = 1ull << 63;                // a move source in the previous call's hold, not in the staging bytes
constexpr uint32_t RS_ROUNDS = 8, RS_TILE = 256 * RS_ROUNDS;  // items per block of the histogram and scatter kernels

__device__ __forceinline__ uint64_t rs_key(int32_t tid, int32_t pos) { return ((uint64_t)(uint32_t)tid << 32) | (uint32_t)(pos + 1); }

// what a call leaves for the host (copied behind the stage) and for the next call (read on the device)
struct ResortCtl {
    unsigned long long W;            // the key as it came in of the last record framed so far
    unsigned long long emit_bytes;   // bytes of the records that leave with this call
    unsigned long long total_bytes;  // those and the held ones'
    unsigned long long bad;          // 0: none; else (0xffffffff - record) << 8 | 1: the first record in front of which the input's order breaks
    uint32_t n_in;                   // items: held over + the call's records
    uint32_t n_emit;                 // of them leave; the others are held
    uint32_t n_held_in;              // held over from the previous call
    uint32_t pad;
};

struct ResortArgs {
    ResortCtl *ctl;
    // the previous call's: its ctl and its arrays in final order (nullptr on a stream's first call)
    const ResortCtl *prev;
    const uint64_t *p_key, *p_dst;
    const uint32_t *p_size;
    uint32_t h_cap;                  // the host's bound on prev->n_hold: what the arrays hold beside the call's records
    uint32_t n, last;                // the call's records; the stream's last call
    const uint8_t *u;
    const uint32_t *rec_off;         // the file path's record offsets ...
    const uint64_t *rec_off64;       // ... or a record batch's
    const uint32_t *out_size;        // the records' sizes as they leave
    const uint64_t *blk_base;        // and their blocks' bases in the staging bytes
    uint64_t *key0, *key1;           // the sort's two sides: keys ...
    uint32_t *idx0, *idx1;           // ... and item numbers
    uint32_t *hist, *hist_base;      // [256 digits][tiles]
    uint64_t *isrc;                  // per item: where its bytes are (RS_FROM_HOLD | offset) ...
    uint32_t *isize;                 // ... and how many
    uint64_t *msrc, *dst;            // the same in final order; dst [n_in + 1]: offsets in final order
    uint32_t *msize;
    uint64_t *sblk;                  // block sums of the sizes in final order, their bases behind them
    const uint8_t *stage, *hold_in;  // the move: the call's records in input order, the previous call's hold
    uint8_t *out, *hold_out;
};

__device__ __forceinline__ uint32_t rs_tiles(uint32_t m) { return (m + RS_TILE - 1u) / RS_TILE; }

// One thread per held-over record, behind the previous call's stage: its key, its place in the previous hold and its size
// become items 0 .. n_held_in - 1.  Thread 0 also sets the call's ctl: the item count and W.
__global__ __launch_bounds__(256) void bam_resort_carry_kernel(ResortArgs a) {
    uint32_t h = 0, e = 0;
    if (a.prev) {
        e = a.prev->n_emit;
        h = min(a.prev->n_in - e, a.h_cap);
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        unsigned long long w = a.prev ? a.prev->W : 0ull;
        if (a.n) {
            const uint8_t *p = a.u + a.rec_off[a.n - 1u];
            w = rs_key(ld32s(p + 4), ld32s(p + 8));
        }
        a.ctl->W = a.last ? ~0ull : w;
        a.ctl->bad = 0;  // (the keys kernel, behind this one, raises it)
        a.ctl->emit_bytes = 0;
        a.ctl->total_bytes = 0;
        a.ctl->n_in = h + a.n;
        a.ctl->n_emit = 0;
        a.ctl->n_held_in = h;
        a.ctl->pad = 0;
    }
    if (i >= h) return;
    a.key0[i] = a.p_key[e + i];
    a.idx0[i] = i;
    a.isrc[i] = RS_FROM_HOLD | (a.p_dst[e + i] - a.prev->emit_bytes);
    a.isize[i] = a.p_size[e + i];
}

// One thread per record of the call, behind the size kernels and their scan (a block per TAG_BLOCK records, whose base
// applies): the key as it came in against the record in front (the first record: against the previous call's W), the key as
// the record leaves from the clip plan the rewrite will follow, and where the rewrite puts it in the staging bytes.
template <bool FROM_TAGS>
__global__ __launch_bounds__(TAG_BLOCK) void bam_resort_keys_kernel(ResortArgs a, TagArgs ta, FromTagsArgs fa) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t sz = i < a.n ? a.out_size[i] : 0u;
    uint64_t tot;
    const uint64_t at = a.blk_base[blockIdx.x] + block_scan_256((uint64_t)sz, &tot);
    if (i >= a.n) return;
    const RecHdr r = rec_header(a.u + a.rec_off[i]);
    const uint64_t key_in = rs_key(r.tid, r.pos);
    uint64_t front = a.prev ? a.prev->W : 0ull;
    if (i) {
        const uint8_t *q = a.u + a.rec_off[i - 1u];
        front = rs_key(ld32s(q + 4), ld32s(q + 8));
    }
    if (key_in < front) atomicMax(&a.ctl->bad, ((unsigned long long)(0xffffffffu - i) << 8) | 1ull);
    ClipPlan c;
    c.mode = 0;
    if constexpr (FROM_TAGS) {
        if (!(fa.info[i] & INFO_BAD)) c = clip_plan(r, fa.rsb[i], fa.trim_l[i], fa.trim_r[i]);
    } else {
        uint8_t rs;
        const fadehip_aln *al = aln_of(ta, ta.sent_of[i], &rs);
        if (al && !(ta.info[i] & INFO_BAD)) {
            const uint32_t trim = art_ref_len(al);
            c = clip_plan(r, rs, trim, trim);
        }
    }
    const uint32_t h = a.prev ? min(a.prev->n_in - a.prev->n_emit, a.h_cap) : 0u;
    a.key0[h + i] = c.mode == 2u ? RS_KEY_UNMAPPED : c.mode == 1u ? rs_key(r.tid, c.pos) : key_in;
    a.idx0[h + i] = h + i;
    a.isrc[h + i] = at;
    a.isize[h + i] = sz;
}

// fadehip_coord_order_batch: the keys of records the caller brings, as they are
__global__ __launch_bounds__(256) void bam_resort_batch_keys_kernel(ResortArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        a.ctl->W = ~0ull;
        a.ctl->emit_bytes = 0;
        a.ctl->total_bytes = 0;
        a.ctl->bad = 0;
        a.ctl->n_in = a.n;
        a.ctl->n_emit = 0;
        a.ctl->n_held_in = 0;
        a.ctl->pad = 0;
    }
    if (i >= a.n) return;
    const uint8_t *p = a.u + a.rec_off64[i];
    a.key0[i] = rs_key(ld32s(p + 4), ld32s(p + 8));
    a.idx0[i] = i;
}

// ---- the sort: pass `pass` of eight takes the keys' bits 8 pass .. 8 pass + 7, from side pass & 1 to the other
// how many items of a tile carry each digit
__global__ __launch_bounds__(256) void bam_resort_hist_kernel(ResortArgs a, uint32_t pass) {
    __shared__ uint32_t h[256];
    const uint32_t m = a.ctl->n_in, nblk = rs_tiles(m);
    if (blockIdx.x >= nblk) return;
    const uint64_t *kin = (pass & 1u) ? a.key1 : a.key0;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t round = 0; round < RS_ROUNDS; round++) {
        const uint32_t j = blockIdx.x * RS_TILE + round * 256u + threadIdx.x;
        if (j < m) atomicAdd(&h[(uint32_t)(kin[j] >> (8u * pass)) & 255u], 1u);
    }
    __syncthreads();
    a.hist[threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// where every (digit, tile) starts: digit-major, so that a digit's items stay in tile order
__global__ __launch_bounds__(1024) void bam_resort_scan_kernel(ResortArgs a) {
    scan_block_sums<uint32_t, false>(a.hist, a.hist_base, 256u * rs_tiles(a.ctl->n_in), (uint32_t *)nullptr);
}

// Every item to its digit's place, in the order it came: 256 items a round, a wave's items of one digit found by ballot
// (their count from the group's first lane, a lane's rank from the lanes below it), the waves and the rounds so far added up
// in LDS.
__global__ __launch_bounds__(256) void bam_resort_scatter_kernel(ResortArgs a, uint32_t pass) {
    __shared__ uint32_t cnt[4][256];
    __shared__ uint32_t run[256];
    const uint32_t m = a.ctl->n_in, nblk = rs_tiles(m);
    if (blockIdx.x >= nblk) return;
    const uint64_t *kin = (pass & 1u) ? a.key1 : a.key0;
    uint64_t *kout = (pass & 1u) ? a.key0 : a.key1;
    const uint32_t *iin = (pass & 1u) ? a.idx1 : a.idx0;
    uint32_t *iout = (pass & 1u) ? a.idx0 : a.idx1;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    run[tid] = a.hist_base[tid * nblk + blockIdx.x];
    for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
    __syncthreads();
    for (uint32_t round = 0; round < RS_ROUNDS; round++) {
        const uint32_t j = blockIdx.x * RS_TILE + round * 256u + tid;
        const bool valid = j < m;
        uint64_t key = 0;
        uint32_t ix = 0, d = 0;
        if (valid) {
            key = kin[j];
            ix = iin[j];
            d = (uint32_t)(key >> (8u * pass)) & 255u;
        }
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++) {
            const unsigned long long set = __ballot(valid && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && below == 0u) cnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t at = run[d] + below;
            for (uint32_t w = 0; w < wave; w++) at += cnt[w][d];
            if (at < m) {  // (always: the histogram counted these very items)
                kout[at] = key;
                iout[at] = ix;
            }
        }
        __syncthreads();
        uint32_t s = 0;
        for (int w = 0; w < 4; w++) {
            s += cnt[w][tid];
            cnt[w][tid] = 0;
        }
        run[tid] += s;
        __syncthreads();
    }
}

// ---- behind the eighth pass (side 0 holds the final order): the cut, the sizes in final order and their block sums
__global__ __launch_bounds__(TAG_BLOCK) void bam_resort_cut_kernel(ResortArgs a) {
    const uint32_t m = a.ctl->n_in;
    const uint32_t j = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;
    if (j < m) {
        const uint32_t i = a.idx0[j];
        sz = a.isize[i];
        a.msize[j] = (uint32_t)sz;
        a.msrc[j] = a.isrc[i];
        const unsigned long long w = a.ctl->W;
        if (a.key0[j] <= w && (j + 1u == m || a.key0[j + 1u] > w)) a.ctl->n_emit = j + 1u;  // (the order is by key: one thread finds the cut)
    }
    const uint64_t t = block_sum_256(sz);
    if (threadIdx.x == 0) a.sblk[blockIdx.x] = t;
}

__global__ __launch_bounds__(1024) void bam_resort_offsets_scan_kernel(ResortArgs a, uint32_t nblk_cap) {
    const uint32_t nblk = (a.ctl->n_in + TAG_BLOCK - 1u) / TAG_BLOCK;
    scan_block_sums<uint64_t, false>(a.sblk, a.sblk + nblk_cap, nblk, (uint64_t *)nullptr);
}

// the offsets in final order; the bytes that leave, and all of them
__global__ __launch_bounds__(TAG_BLOCK) void bam_resort_offsets_kernel(ResortArgs a, uint32_t nblk_cap) {
    const uint32_t m = a.ctl->n_in;
    const uint32_t j = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint64_t sz = j < m ? (uint64_t)a.msize[j] : 0ull;
    uint64_t tot;
    const uint64_t at = a.sblk[nblk_cap + blockIdx.x] + block_scan_256(sz, &tot);
    if (j >= m) return;
    a.dst[j] = at;
    const uint32_t e = a.ctl->n_emit;
    if (j == e) a.ctl->emit_bytes = at;
    if (j + 1u == m) {
        a.dst[m] = at + sz;
        a.ctl->total_bytes = at + sz;
        if (e == m) a.ctl->emit_bytes = at + sz;
    }
}

// fadehip_coord_order_batch: the final order itself
__global__ __launch_bounds__(256) void bam_resort_order_kernel(ResortArgs a, int32_t *order) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < a.ctl->n_in) order[j] = (int32_t)a.idx0[j];
}

// The move, behind the rewrite: sixteen lanes per item in final order, (unaligned) dwords as the rewrite kernel's body copy.
// An item comes from the staging bytes the rewrite has just written or from the previous call's hold, and goes to the
// call's output or to the hold the next call reads.
__global__ __launch_bounds__(256) void bam_resort_move_kernel(ResortArgs a, uint32_t m, uint32_t n_emit, uint64_t emit_bytes) {
    const uint32_t j = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
    if (j >= m) return;
    const uint64_t s = a.msrc[j], d = a.dst[j];
    const uint8_t *from = (s & RS_FROM_HOLD) ? a.hold_in + (s & ~RS_FROM_HOLD) : a.stage + s;
    uint8_t *to = j < n_emit ? a.out + d : a.hold_out + (d - emit_bytes);
    copy16(to, from, a.msize[j], sl);
}

}  // namespace bam
}  // namespace fadehip
