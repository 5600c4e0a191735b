// bam_index.hpp — FADEHIP_BAM_INDEX: the BAM index (.bai) entries of a call's records as they leave, made on the device in
// the call's back half (the rule is stated in include/fadehip.h and tests/bai_model.py).
//
//   key     a thread per record that leaves: its fixed fields and CIGAR out of the output bytes -> span, bin, windows, the
//           mapped bit, its virtual offsets (from its byte offset, the block size and the compressor's member_off[], or from
//           offsets the caller brings); the order check against the record in front; per block the maximum of
//           (refID << 32 | last window + 1) over its mapped records
//   scan    that maximum over the blocks in front (one block)
//   count   heads of (refID, bin) runs and of refID runs; the windows a mapped record newly covers, [max(w0, m + 1), w1] with
//           m the running maximum of w1 over the earlier mapped records of its refID — refID as uint32 does not decrease in
//           sorted records, so one plain max-scan of (refID << 32 | w1 + 1) is that segmented maximum; per block the sums
//   sums    the sums over the blocks in front, the totals (one block)
//   write   chunks, linear entries and reference runs, dense and in stream order: a run's head writes where it begins, its
//           last record where it ends, so the work per record does not grow with a run's length
//   refs    the reference runs' record counts out of the running counts the write kernel left at their ends
//   key under a CSI geometry (min_shift, depth): a second key kernel, bam_index_key_geo_kernel, with the bin by a level loop,
//           windows of 2^min_shift positions and the span held to 2^(min_shift + 3 depth); the kernels behind it are the same
//
// All kernels here are new; a run without the flag launches none of them, and fadehip_index_batch runs the same kernels over
// records and offsets the caller brings.  Nothing is carried from call to call on the device.
#pragma once
#include "bam_device.hpp"
#include "bam_resort.hpp"

namespace fadehip {
namespace bam {

constexpr uint32_t IX_NONE = 0xffffffffu;     // the flags' rest value: no record
constexpr uint64_t IX_MAX_END = 1ull << 29;   // a BAI's coordinates end here

// what a call leaves for the host
struct IndexCtl {
    unsigned long long n_chunks, n_linear, n_refs, n_mapped;  // (the last: mapped records, the write kernel's running count)
    unsigned long long first_key, last_key;
    uint32_t bad_order;   // the lowest record whose key is below the key in front of it, or IX_NONE
    uint32_t bad_span;    // the lowest record with refID >= 0 and end > 2^29 (under a geometry: its limit), or IX_NONE
    uint32_t n, pad;
};

struct IndexRec {   // a record's part of the index, between the kernels
    int32_t tid;
    uint32_t bin;
    uint32_t w0, w1;      // windows of a mapped record; w0 > w1: none (flag 4, or no reference)
    uint32_t wlo;         // count kernel: the first window the record newly covers (wlo > w1: none)
    uint32_t heads;       // count kernel: bit 0 head of a (refID, bin) run, bit 1 head of a refID run, bit 2 mapped (flag 4 clear)
};

struct IndexArgs {
    IndexCtl *ctl;
    const uint8_t *u;           // the records as they leave ...
    const uint64_t *at;         // ... [n + 1]: where each starts in u, at[n] behind the last
    uint32_t n;                 // records (launches are sized from it) ...
    const uint32_t *n_ptr;      // ... or, where only the device has their number, that and n a bound of it
    // virtual offsets: the caller's [n + 1] ...
    const uint64_t *voff;
    // ... or from `at`: blocks of `block` bytes, member k at member_off[k] (nullptr: k * member_stride), the offset behind
    // the last member at *behind_ptr (nullptr: behind)
    const uint64_t *member_off;
    const uint64_t *behind_ptr;
    uint64_t member_stride, behind;
    uint32_t block;
    uint32_t cap_linear;        // entries `linear` holds
    IndexRec *rec;              // [n]
    uint64_t *uo;               // [n + 1] virtual offsets of the record starts, [n] behind the last
    uint64_t *blk_max, *blk_carry;   // [blocks] the key kernel's maxima, and over the blocks in front
    uint64_t *blk_sums, *blk_base;   // [4][blocks] chunk heads, refID heads, new windows, mapped records
    uint64_t *cum;              // [2][n] at a reference run's number: records and mapped records up to its end
    fadehip_index_chunk *chunks;
    fadehip_index_linear *linear;
    fadehip_index_ref *refs;
};

__device__ __forceinline__ uint32_t ix_reg2bin(uint32_t beg, uint32_t end) {
    end--;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

__device__ __forceinline__ uint32_t ix_n(const IndexArgs &a) { return a.n_ptr ? min(*a.n_ptr, a.n) : a.n; }

__device__ __forceinline__ uint64_t ix_voff(const IndexArgs &a, uint64_t p, uint64_t total) {
    if (p >= total) return (a.behind_ptr ? *a.behind_ptr : a.behind) << 16;
    const uint64_t k = p / a.block;
    return ((a.member_off ? a.member_off[k] : k * a.member_stride) << 16) | (p - k * a.block);
}

// inclusive running maximum of v over a block of TAG_BLOCK threads; *excl: over the threads in front (0 for the first)
__device__ __forceinline__ uint64_t ix_block_max_scan(uint64_t v, uint64_t *excl) {
    __shared__ uint64_t wmax[TAG_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
        if (lane >= d) inc = max(inc, o);
    }
    uint64_t ex = (uint64_t)__shfl_up((long long)inc, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) wmax[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; w++) {
        inc = max(inc, wmax[w]);
        ex = max(ex, wmax[w]);
    }
    *excl = ex;
    return inc;
}

// The key stage under a CSI geometry (tests/csi_model.py): IndexArgs as it is, and beside it the geometry.
// min_shift, depth and limit are kernel arguments, so they sit in scalar registers: the level loop below has a wave-uniform
// trip count and shifts by scalar operands, and no lane leaves it early.
struct IndexGeoArgs {
    IndexArgs a;
    uint32_t min_shift, depth;   // 4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32 (the host checks)
    uint64_t limit;              // 2^(min_shift + 3 * depth)
};

// the deepest bin that holds [beg, end], both below 2^32: level l = 1 .. depth has bins of 2^(min_shift + 3 (depth - l))
// positions from number (8^l - 1) / 7.  Two positions that share a bin share its ancestors, so walking down from level 1 the
// last level that still holds both is the deepest; the root (bin 0) holds everything.
__device__ __forceinline__ uint32_t ix_reg2bin_geo(uint32_t beg, uint32_t end, uint32_t min_shift, uint32_t depth) {
    uint32_t bin = 0, first = 1, s = min_shift + 3u * (depth - 1u);
    for (uint32_t l = 1; l <= depth; l++) {
        const uint32_t b = beg >> s;
        if (b == end >> s) bin = first + b;
        first = first * 8u + 1u;
        s -= 3u;
    }
    return bin;
}

// the key kernel's body: GEO false is BAI's fixed tree (the three arguments behind `a` are not read), true the geometry's
template <bool GEO>
__device__ __forceinline__ void ix_key(const IndexArgs &a, uint32_t min_shift, uint32_t depth, uint64_t limit) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t n = ix_n(a);
    uint64_t val = 0;
    if (i < n) {
        const uint64_t p = a.at[i], pe = a.at[i + 1u], total = a.at[n];
        const uint8_t *r = a.u + p;
        const int32_t tid = ld32s(r + 4), pos = ld32s(r + 8);
        const uint32_t lname = r[12], flag = ld16(r + 18);
        uint32_t ncig = ld16(r + 16);
        const uint64_t room = pe - p > 36u + lname ? (pe - p - 36u - lname) / 4u : 0u;  // (ops beyond the record's bytes are never read)
        if (ncig > room) ncig = (uint32_t)room;
        const bool mapped = !(flag & 4u);
        uint64_t reflen = 0;
        if (mapped) {
            const uint8_t *c = r + 36u + lname;
            for (uint32_t k = 0; k < ncig; k++) {
                const uint32_t op = ld32(c + 4u * k);
                if (FADEHIP_OP_CONSUMES_REF(op)) reflen += op >> 4;
            }
        }
        const uint64_t beg = pos > 0 ? (uint64_t)pos : 0ull;
        const uint64_t end = beg + (reflen ? reflen : 1ull);
        const uint64_t key = rs_key(tid, pos);
        if (i) {
            const uint8_t *q = a.u + a.at[i - 1u];
            if (key < rs_key(ld32s(q + 4), ld32s(q + 8))) atomicMin(&a.ctl->bad_order, i);
        } else a.ctl->first_key = key;
        if (i + 1u == n) a.ctl->last_key = key;
        IndexRec x;
        x.tid = tid;
        x.bin = 0;
        x.w0 = 1;
        x.w1 = 0;
        x.wlo = 1;
        x.heads = mapped ? 4u : 0u;
        if (tid >= 0) {
            if (end > (GEO ? limit : IX_MAX_END)) atomicMin(&a.ctl->bad_span, i);
            else {
                x.bin = GEO ? ix_reg2bin_geo((uint32_t)beg, (uint32_t)(end - 1u), min_shift, depth) : ix_reg2bin((uint32_t)beg, (uint32_t)end);
                if (mapped) {
                    // (GEO: end <= limit <= 2^32, so (end - 1) >> min_shift < 2^(32 - min_shift) <= 2^28 with min_shift >= 4:
                    // w1 + 1 <= 2^28 fits the low 32 bits of the packed maximum, as BAI's 2^15 does)
                    x.w0 = (uint32_t)(beg >> (GEO ? min_shift : 14u));
                    x.w1 = (uint32_t)((end - 1u) >> (GEO ? min_shift : 14u));
                    val = ((uint64_t)(uint32_t)tid << 32) | (x.w1 + 1u);
                }
            }
        }
        a.rec[i] = x;
        a.uo[i] = a.voff ? a.voff[i] : ix_voff(a, p, total);
        if (i + 1u == n) a.uo[n] = a.voff ? a.voff[n] : ix_voff(a, pe, total);
    }
    uint64_t ex;
    const uint64_t m = ix_block_max_scan(val, &ex);
    if (threadIdx.x == TAG_BLOCK - 1) a.blk_max[blockIdx.x] = m;
}

__global__ __launch_bounds__(TAG_BLOCK) void bam_index_key_kernel(IndexArgs a) { ix_key<false>(a, 14u, 5u, IX_MAX_END); }

// ... and under a geometry: everything behind it (max scan, count, sum scan, write, refs) reads only tid, bin, w0 and w1
__global__ __launch_bounds__(TAG_BLOCK) void bam_index_key_geo_kernel(IndexGeoArgs g) { ix_key<true>(g.a, g.min_shift, g.depth, g.limit); }

__global__ __launch_bounds__(1024) void bam_index_max_scan_kernel(IndexArgs a, uint32_t n_blocks) {
    scan_block_sums<uint64_t, true>(a.blk_max, a.blk_carry, n_blocks, (uint64_t *)nullptr);
}

// the four counts of a record, as the count and the write kernel both need them
__device__ __forceinline__ void ix_counts(const IndexRec &x, uint64_t c[4]) {
    c[0] = x.heads & 1u;
    c[1] = (x.heads >> 1) & 1u;
    c[2] = x.wlo <= x.w1 ? (uint64_t)(x.w1 - x.wlo) + 1ull : 0ull;
    c[3] = (x.heads >> 2) & 1u;
}

__global__ __launch_bounds__(TAG_BLOCK) void bam_index_count_kernel(IndexArgs a, uint32_t n_blocks) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t n = ix_n(a);
    IndexRec x;
    x.tid = -1;
    x.bin = 0;
    x.w0 = x.wlo = 1;
    x.w1 = 0;
    x.heads = 0;
    uint64_t val = 0;
    if (i < n) {
        x = a.rec[i];
        if (x.w0 <= x.w1) val = ((uint64_t)(uint32_t)x.tid << 32) | (x.w1 + 1u);
    }
    uint64_t ex;
    ix_block_max_scan(val, &ex);
    ex = max(ex, a.blk_carry[blockIdx.x]);
    if (i < n) {
        bool bin_head = x.tid >= 0, ref_head = true;
        if (i) {
            const int32_t f_tid = a.rec[i - 1u].tid;  // (tid and bin: the key kernel's, which this kernel leaves alone)
            const uint32_t f_bin = a.rec[i - 1u].bin;
            ref_head = f_tid != x.tid;
            bin_head = x.tid >= 0 && (ref_head || f_bin != x.bin);
        }
        x.heads = (x.heads & 4u) | (bin_head ? 1u : 0u) | (ref_head ? 2u : 0u);
        if (x.w0 <= x.w1) {
            const uint32_t m1 = (uint32_t)(ex >> 32) == (uint32_t)x.tid ? (uint32_t)ex : 0u;  // 1 + the windows reached so far
            x.wlo = max(x.w0, m1);
        }
        a.rec[i].wlo = x.wlo;
        a.rec[i].heads = x.heads;
    }
    uint64_t c[4];
    ix_counts(x, c);
    for (int k = 0; k < 4; k++) {
        const uint64_t t = block_sum_256(c[k]);
        if (threadIdx.x == 0) a.blk_sums[(size_t)k * n_blocks + blockIdx.x] = t;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void bam_index_sum_scan_kernel(IndexArgs a, uint32_t n_blocks) {
    unsigned long long *tot[4] = {&a.ctl->n_chunks, &a.ctl->n_refs, &a.ctl->n_linear, &a.ctl->n_mapped};
    for (int k = 0; k < 4; k++) {
        scan_block_sums<uint64_t, false>(a.blk_sums + (size_t)k * n_blocks, a.blk_base + (size_t)k * n_blocks, n_blocks, (uint64_t *)tot[k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.ctl->n = ix_n(a);
}

__global__ __launch_bounds__(TAG_BLOCK) void bam_index_write_kernel(IndexArgs a, uint32_t n_blocks) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t n = ix_n(a);
    IndexRec x;
    x.tid = -1;
    x.bin = 0;
    x.w0 = x.wlo = 1;
    x.w1 = 0;
    x.heads = 0;
    bool bin_tail = false, ref_tail = false;
    if (i < n) {
        x = a.rec[i];
        ref_tail = true;
        bin_tail = x.tid >= 0;
        if (i + 1u < n) {
            const uint32_t h = a.rec[i + 1u].heads;
            ref_tail = (h & 2u) != 0u;
            bin_tail = x.tid >= 0 && ((h & 1u) != 0u || ref_tail);
        }
    }
    uint64_t c[4], at[4];
    ix_counts(x, c);
    for (int k = 0; k < 4; k++) {
        uint64_t tot;
        at[k] = a.blk_base[(size_t)k * n_blocks + blockIdx.x] + block_scan_256(c[k], &tot);
        __syncthreads();
    }
    if (i >= n) return;
    const uint64_t uo = a.uo[i], vo = a.uo[i + 1u];
    if (c[0]) {
        a.chunks[at[0]].tid = x.tid;
        a.chunks[at[0]].bin = x.bin;
        a.chunks[at[0]].beg = uo;
    }
    if (bin_tail) a.chunks[at[0] + c[0] - 1ull].end = vo;  // (a record of a run is behind its head: at least one head is counted)
    if (c[1]) {
        a.refs[at[1]].tid = x.tid;
        a.refs[at[1]].reserved = 0;
        a.refs[at[1]].off_beg = uo;
    }
    if (ref_tail) {
        const uint64_t r = at[1] + c[1] - 1ull;
        a.refs[r].off_end = vo;
        a.cum[2ull * r] = (uint64_t)i + 1ull;
        a.cum[2ull * r + 1ull] = at[3] + c[3];
    }
    for (uint64_t k = 0; k < c[2]; k++) {
        const uint64_t j = at[2] + k;
        if (j < a.cap_linear) {
            a.linear[j].tid = x.tid;
            a.linear[j].window = x.wlo + (uint32_t)k;
            a.linear[j].off = uo;
        }
    }
}

// a thread per reference run (n_refs of them: the host has the count, or a bound of it)
__global__ __launch_bounds__(256) void bam_index_refs_kernel(IndexArgs a, uint32_t n_runs_cap) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_runs_cap || r >= a.ctl->n_refs) return;
    const uint64_t n0 = r ? a.cum[2ull * (r - 1u)] : 0ull, m0 = r ? a.cum[2ull * (r - 1u) + 1ull] : 0ull;
    const uint64_t n1 = a.cum[2ull * r], m1 = a.cum[2ull * r + 1ull];
    a.refs[r].n_mapped = m1 - m0;
    a.refs[r].n_unmapped = (n1 - n0) - (m1 - m0);
}

// ---- where the records lie that the rewrite kernel writes (a call without KEEP_SORTED, whose move kernel has the offsets
// in final order already): record i is written when out_size[i] != 0 — an ejected record has none — at its block's base plus
// the sizes in front of it in its block, as the rewrite kernel finds it.  Dense, in input order, the total behind the last.
struct IndexAtArgs {
    const uint32_t *out_size;   // [n]
    const uint64_t *blk_base;   // [blocks of TAG_BLOCK records] the tag scan's
    uint32_t n;
    uint32_t *cnt, *cnt_base;   // [blocks] records written per block, and in the blocks in front
    uint32_t *n_out;            // the records written
    uint64_t *at;               // [n + 1]
};

__global__ __launch_bounds__(TAG_BLOCK) void bam_index_present_kernel(IndexAtArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint64_t t = block_sum_256(i < a.n && a.out_size[i] ? 1ull : 0ull);
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = (uint32_t)t;
}

__global__ __launch_bounds__(1024) void bam_index_present_scan_kernel(IndexAtArgs a, uint32_t n_blocks) {
    scan_block_sums<uint32_t, false>(a.cnt, a.cnt_base, n_blocks, a.n_out);
}

__global__ __launch_bounds__(TAG_BLOCK) void bam_index_at_kernel(IndexAtArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint64_t sz = i < a.n ? (uint64_t)a.out_size[i] : 0ull;
    uint64_t tot;
    const uint64_t p = a.blk_base[blockIdx.x] + block_scan_256(sz, &tot);
    __syncthreads();
    const uint64_t j = a.cnt_base[blockIdx.x] + block_scan_256(sz ? 1ull : 0ull, &tot);
    if (i >= a.n) return;
    if (sz) a.at[j] = p;
    if (i + 1u == a.n) a.at[j + (sz ? 1ull : 0ull)] = p + sz;
}

}  // namespace bam
}  // namespace fadehip
