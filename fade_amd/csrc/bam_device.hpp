// bam_device.hpp — the BAM record stream handled on the device (gfx950), between the BGZF inflater and the BGZF
// compressor: what dhtslib's SAMReader / SAMRecord / SAMWriter do around annotateTask (anno.d:44-50, 61-107), so that a
// file passes through the device as bytes and the host only moves compressed blocks.
//
//   inflated bytes U  --frame-->  record offsets  --pack-->  the batch arrays of fadehip_read_batch (the records
//   anno.d:61-65 does not settle)  --[gate, score pass, pass 2: fadehip_kernels.hpp]-->  rs, alignments
//   --tag sizes, scan-->  output offsets  --rewrite-->  output bytes O (records + rs / am / as / ar / ab)  --> compressor
//
// Framing.  BAM records are chained by block_size; following the chain is serial, so it is done speculatively per 64 KB
// segment: a wave looks for the first position in its segment that looks like a record (block_size, refID, pos,
// l_read_name, n_cigar_op, l_seq, next_refID, next_pos consistent with each other and with the header, name
// NUL-terminated) and walks the chain from there; a single wave then checks, segment by segment, that the chain really
// enters each segment where its wave assumed — and walks any segment again, serially, where it did not.  The plausibility
// test only decides how often that happens, never what the result is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fadehip.h"

namespace fadehip {
namespace bam {

typedef uint32_t u32u __attribute__((aligned(1)));
typedef int32_t i32u __attribute__((aligned(1)));
typedef uint16_t u16u __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return *reinterpret_cast<const u32u *>(p); }
__device__ __forceinline__ int32_t ld32s(const uint8_t *p) { return *reinterpret_cast<const i32u *>(p); }
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return *reinterpret_cast<const u16u *>(p); }

// framing segment: a walk is a chain of one dependent load per record, so the segment sets the framing's latency (64 KB: ~200
// records, 185 us per call; 16 KB: a quarter of that).  The resolving wave no longer pays per segment (bam_frame_resolve_kernel
// takes the linked segments of a group at once), which is what kept the segments large.
constexpr uint32_t SEG = 16384;
constexpr uint32_t SEG_SLOTS = SEG / 36 + 2;    // record starts a segment can hold (a record takes at least 36 bytes)
constexpr uint32_t EXIT_INCOMPLETE = 0x80000000u, EXIT_BAD = 0x40000000u, EXIT_MASK = 0x3fffffffu;
constexpr uint32_t MAX_U = 0x3fffff00u;         // inflated bytes per chunk (offsets are 30 bits + two flags)

// ---- counters of a chunk, read back by the host between the stages
struct ChunkCounts {
    uint32_t n_records;     // complete records framed
    uint32_t consumed;      // bytes of U covered by them (the rest is carried over to the next chunk)
    uint32_t frame_err;     // != 0: a record on the chain is impossible (block_size < 32), at offset frame_err_at
    uint32_t frame_err_at;
    uint32_t n_redone;      // segments whose speculative entry was wrong (diagnostics)
    uint32_t n_bad_layout;  // records whose fields do not fit their block_size / whose aux area is not whole fields
    uint32_t n_sent;        // records that go to the gate kernel (mapped, with an S op)
    uint32_t n_cig;         // their CIGAR ops
    uint32_t n_seq;         // their packed sequence bytes
    uint32_t l_seq_min, l_seq_max, span_max, n_long_q;
    uint32_t n_ours;        // records that already carry one of rs / am / as / ar / ab
    uint32_t n_ejected;     // records the eject kernels took out of the output (FADEHIP_BAM_EJECT)
    uint32_t pad1;
    uint64_t out_bytes;     // bytes of the rewritten record stream
    uint64_t pad2;
};

// ============================================================================================ framing
__device__ __forceinline__ bool plausible(const uint8_t *u, uint32_t at, uint32_t u_len, int32_t n_ref) {
    if (at + 36u > u_len) return false;
    const uint8_t *p = u + at;
    const uint32_t bs = ld32(p);
    const int32_t tid = ld32s(p + 4), pos = ld32s(p + 8), lseq = ld32s(p + 20), ntid = ld32s(p + 24), npos = ld32s(p + 28);
    const uint32_t lname = p[12], ncig = ld16(p + 16);
    if (bs < 33u || bs > (1u << 29)) return false;
    if (tid < -1 || tid >= n_ref || ntid < -1 || ntid >= n_ref || pos < -1 || npos < -1 || lseq < 0 || lname == 0) return false;
    const uint64_t need = 32ull + lname + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq;
    if (need > bs) return false;
    const uint32_t nul = at + 36u + lname - 1u;
    if (nul < u_len && u[nul] != 0) return false;
    return true;
}

// Walk the chain from `c` while records start in front of seg_end; record starts go to slots[0 .. n).  Returns the exit:
// the start of the first record at or behind seg_end, or (| EXIT_INCOMPLETE) the start of a record that is not whole in
// U, or (| EXIT_BAD) the start of an impossible one.
__device__ __forceinline__ uint32_t walk_segment(const uint8_t *u, uint32_t u_len, uint32_t c, uint32_t seg_end, uint32_t *slots, uint32_t *n_out) {
    uint32_t n = 0;
    uint32_t ex;
    for (;;) {
        if (c >= seg_end) { ex = c; break; }
        if (c + 4u > u_len) { ex = c | EXIT_INCOMPLETE; break; }
        const uint32_t bs = ld32(u + c);
        if (bs < 32u || bs > (1u << 29)) { ex = c | EXIT_BAD; break; }
        if ((uint64_t)c + 4ull + bs > (uint64_t)u_len) { ex = c | EXIT_INCOMPLETE; break; }
        if (n < SEG_SLOTS) slots[n] = c;
        n++;
        c += 4u + bs;
    }
    *n_out = n;
    return ex;
}

struct FrameArgs {
    const uint8_t *u;
    uint32_t u_len;             // bytes of U (carried-over bytes + this chunk's inflated bytes)
    uint32_t first;             // where the chain starts in U
    int32_t n_ref;
    uint32_t n_seg_cap;         // segments the arrays hold
    uint32_t *cand, *exit_, *cnt, *base;  // per segment
    uint32_t *slots;            // [n_seg][SEG_SLOTS]
    uint32_t *rec_off;          // [n_records + 1] out
    uint32_t rec_cap;
    ChunkCounts *counts;
};

// one wave per WALK_SEGS segments: the lanes look for each segment's first plausible record together, then WALK_SEGS lanes walk
// one segment each (a walk is a chain of ~200 dependent loads: the more waves share the segments, the sooner it is over)
constexpr uint32_t WALK_SEGS = 8;
__global__ __launch_bounds__(64) void bam_frame_walk_kernel(FrameArgs a) {
    const uint32_t u_len = a.u_len;
    const uint32_t n_seg = (u_len + SEG - 1) / SEG;
    const int lane = threadIdx.x;
    const uint32_t s0 = blockIdx.x * WALK_SEGS;
    uint32_t my_cand = 0xffffffffu;
    for (uint32_t j = 0; j < WALK_SEGS; j++) {
        const uint32_t s = s0 + j;
        if (s >= n_seg) break;  // (uniform)
        uint32_t found = 0xffffffffu;
        if (s == 0) {
            found = a.first;
        } else {
            // a record start in this segment, or — when one record covers it all — none: the search stops at the segment's end
            const uint32_t lo = s * SEG, hi = min(lo + SEG, u_len);
            for (uint32_t at = lo; at < hi && found == 0xffffffffu; at += 64u) {
                const bool ok = at + (uint32_t)lane < hi && plausible(a.u, at + (uint32_t)lane, u_len, a.n_ref);
                const unsigned long long m = __ballot(ok);
                if (m) found = at + (uint32_t)__ffsll((long long)m) - 1u;
            }
        }
        if ((uint32_t)lane == j) my_cand = found;
    }
    const uint32_t s = s0 + (uint32_t)lane;
    if ((uint32_t)lane < WALK_SEGS && s < n_seg && s < a.n_seg_cap) {
        uint32_t n = 0, ex = 0xffffffffu;
        if (my_cand != 0xffffffffu) ex = walk_segment(a.u, u_len, my_cand, min((s + 1u) * SEG, 0xffffffffu - SEG), a.slots + (size_t)s * SEG_SLOTS, &n);
        a.cand[s] = my_cand;
        a.exit_[s] = ex;
        a.cnt[s] = n;
    }
}

// one wave: the true chain through the segments
__global__ __launch_bounds__(64) void bam_frame_resolve_kernel(FrameArgs a) {
    const uint32_t u_len = a.u_len;
    const uint32_t n_seg = min((u_len + SEG - 1) / SEG, a.n_seg_cap);
    const int lane = threadIdx.x;
    uint32_t entry = a.first, total = 0, redone = 0, err = 0, err_at = 0;
    bool stop = false;
    if (entry > u_len) { stop = true; err = 2; err_at = entry; }
    for (uint32_t s0 = 0; s0 < n_seg; s0 += 64u) {
        const uint32_t s = s0 + (uint32_t)lane;
        uint32_t c = 0xffffffffu, e = 0, n = 0;
        if (s < n_seg) { c = a.cand[s]; e = a.exit_[s]; n = a.cnt[s]; }
        uint32_t my_base = 0, my_n = 0;
        // The group's head without a chain: a segment's walk is the true one when it started where the chain enters it — its
        // candidate is the exit of the segment in front (for the group's first: the entry carried here), inside the segment.
        // That holds for all but a handful of a call's segments (where a look-alike precedes the first record, or one record
        // covers a whole segment); for the lanes up to the first that is different, or the first whose walk ended early, the
        // record counts are a prefix sum and the entry is the last one's exit.  The rest of the group takes the chain below.
        uint32_t j_from = 0;
        if (!stop) {
            uint32_t prev_e = (uint32_t)__shfl_up((int)e, 1, 64);
            if (lane == 0) prev_e = entry;
            const bool clean = !(e & (EXIT_BAD | EXIT_INCOMPLETE));
            const bool link = s < n_seg && c != 0xffffffffu && prev_e == c && c < (s + 1u) * SEG;  // (a flagged exit in front never equals a candidate: the flags are high bits)
            const unsigned long long links = __ballot(link), cleans = __ballot(clean || s >= n_seg);
            uint32_t k = ~links ? (uint32_t)__builtin_ctzll(~links) : 64u;          // lanes [0, k) are linked
            if (~cleans) k = min(k, (uint32_t)__builtin_ctzll(~cleans) + 1u);         // ... up to and with the first walk that ended early
            if (k) {
                // exclusive prefix sum of the counts over lanes [0, k)
                uint32_t inc = (uint32_t)lane < k ? n : 0u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
                    if (lane >= d) inc += up;
                }
                if ((uint32_t)lane < k) { my_base = total + inc - n; my_n = n; }
                total += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                const uint32_t ex = (uint32_t)__shfl((int)e, (int)k - 1, 64);
                if (ex & EXIT_BAD) { stop = true; err = 1; err_at = ex & EXIT_MASK; entry = ex & EXIT_MASK; }
                else if (ex & EXIT_INCOMPLETE) { stop = true; entry = ex & EXIT_MASK; }
                else entry = ex;
                j_from = k;
            }
        }
        for (uint32_t j = j_from; j < 64u && s0 + j < n_seg; j++) {
            const uint32_t sj = s0 + j;
            const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)j), ej = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)j),
                           nj = (uint32_t)__builtin_amdgcn_readlane((int)n, (int)j);
            uint32_t use_n = 0;
            const uint32_t base_j = total;
            if (!stop && entry < (sj + 1u) * SEG) {
                uint32_t ex = ej;
                use_n = nj;
                if (entry != cj) {
                    // the wave of this segment assumed another entry: walk it again from the true one (one lane; rare)
                    uint32_t n2 = 0, ex2 = 0;
                    if (lane == 0) ex2 = walk_segment(a.u, u_len, entry, (sj + 1u) * SEG, a.slots + (size_t)sj * SEG_SLOTS, &n2);
                    ex = (uint32_t)__builtin_amdgcn_readlane((int)ex2, 0);
                    use_n = (uint32_t)__builtin_amdgcn_readlane((int)n2, 0);
                    redone++;
                }
                total += use_n;
                if (ex & EXIT_BAD) { stop = true; err = 1; err_at = ex & EXIT_MASK; entry = ex & EXIT_MASK; }
                else if (ex & EXIT_INCOMPLETE) { stop = true; entry = ex & EXIT_MASK; }
                else entry = ex;
            }
            if ((uint32_t)lane == j) { my_base = base_j; my_n = use_n; }
        }
        if (s < n_seg) { a.base[s] = my_base; a.cnt[s] = my_n; }
    }
    if (lane == 0) {
        ChunkCounts *cc = a.counts;
        cc->n_records = total;
        cc->consumed = min(entry, u_len);
        cc->frame_err = err;
        cc->frame_err_at = err_at;
        cc->n_redone = redone;
    }
}

// rec_off[base[s] + k] = slots[s][k]; rec_off[n_records] = consumed
__global__ __launch_bounds__(256) void bam_frame_compact_kernel(FrameArgs a) {
    const uint32_t u_len = a.u_len;
    const uint32_t n_seg = min((u_len + SEG - 1) / SEG, a.n_seg_cap);
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.counts->n_records < a.rec_cap) a.rec_off[a.counts->n_records] = a.counts->consumed;
    if (s >= n_seg) return;
    const uint32_t n = min(a.cnt[s], SEG_SLOTS), b = a.base[s];
    for (uint32_t k = (uint32_t)lane; k < n; k += 64u)
        if (b + k < a.rec_cap) a.rec_off[b + k] = a.slots[(size_t)s * SEG_SLOTS + k];
}

// ============================================================================================ records
struct RecHdr {
    const uint8_t *p;   // at block_size
    uint32_t bs;        // block_size
    int32_t tid, pos, lseq;
    uint32_t lname, ncig, flag;
    uint32_t cig_off, seq_off, qual_off, aux_off;  // relative to p
    uint32_t end;                                  // 4 + bs
};
__device__ __forceinline__ RecHdr rec_header(const uint8_t *p) {
    RecHdr r;
    r.p = p;
    r.bs = ld32(p);
    r.tid = ld32s(p + 4);
    r.pos = ld32s(p + 8);
    r.lname = p[12];
    r.ncig = ld16(p + 16);
    r.flag = ld16(p + 18);
    r.lseq = ld32s(p + 20);
    r.cig_off = 36u + r.lname;
    r.seq_off = r.cig_off + 4u * r.ncig;
    const uint32_t lq = r.lseq > 0 ? (uint32_t)r.lseq : 0u;
    r.qual_off = r.seq_off + (lq + 1u) / 2u;
    r.aux_off = r.qual_off + lq;
    r.end = 4u + r.bs;
    return r;
}
__device__ __forceinline__ int aux_type_size(uint8_t t) {
    switch (t) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}
// size of the aux field whose type byte is at offset q of the record (type byte included), 0 if malformed / not whole
__device__ __forceinline__ uint32_t aux_field_size(const uint8_t *p, uint32_t q, uint32_t end) {
    if (q >= end) return 0;
    const uint8_t t = p[q];
    const int s = aux_type_size(t);
    if (s) return q + 1u + (uint32_t)s <= end ? 1u + (uint32_t)s : 0u;
    if (t == 'Z' || t == 'H') {
        uint32_t k = q + 1u;
        while (k + 4u <= end) {  // four bytes per load: stop at the dword that holds a zero byte
            const uint32_t v = ld32(p + k);
            if ((v - 0x01010101u) & ~v & 0x80808080u) break;
            k += 4u;
        }
        while (k < end && p[k]) k++;
        return k < end ? k - q + 1u : 0u;
    }
    if (t == 'B') {
        if (q + 6u > end) return 0;
        const int es = aux_type_size(p[q + 1]);
        const uint64_t cnt = ld32(p + q + 2);
        if (!es) return 0;
        const uint64_t fs = 6ull + (uint64_t)es * cnt;
        return fs <= (uint64_t)(end - q) ? (uint32_t)fs : 0u;
    }
    return 0;
}
__device__ __forceinline__ bool is_ours(uint8_t a0, uint8_t a1) {
    return (a0 == 'r' && a1 == 's') || (a0 == 'a' && (a1 == 'm' || a1 == 's' || a1 == 'r' || a1 == 'b'));
}

enum : uint32_t { INFO_NEED = 1, INFO_SA = 2, INFO_OURS = 4, INFO_BAD = 8 };

struct PackArgs {
    const uint8_t *u;
    const uint32_t *rec_off;
    const ChunkCounts *counts_in;  // n_records
    uint32_t r0, r1_cap;           // records [r0, min(r1_cap, n_records)) of the chunk are this batch
    uint32_t *info;                // per record of the batch
    uint32_t *blk_sums;            // [n_blocks][3]: sent, cig, seq
    uint32_t *blk_base;            // [n_blocks][3]
    ChunkCounts *counts;           // the batch's totals
    // outputs of the write pass: the batch block (fadehip_read_batch's arrays) + the maps
    int32_t *tid, *pos, *lseq;
    uint32_t *cigar_off, *seq_off;
    uint16_t *flag;
    uint8_t *has_sa;
    uint32_t *cigar_ops;
    uint8_t *seq;
    int32_t *sent_of;              // [records of the batch]: index among the sent records or -1
};
constexpr int PACK_BLOCK = 1024;

__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t *tmp16, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == 63) tmp16[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int w = 0; w < 16; w++) {
        const uint32_t t = tmp16[w];
        if (w < wave) base += t;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

constexpr int TAG_BLOCK = 256;  // records per block of the tag-size, extract and eject kernels

// sum of v over a block of TAG_BLOCK threads: the waves by shuffle, then their sums by thread 0 — which alone gets the total
__device__ __forceinline__ uint64_t block_sum_256(uint64_t v) {
    __shared__ uint64_t red[TAG_BLOCK / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((long long)v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < TAG_BLOCK / 64; w++) t += red[w];
    return t;
}

// one block of 1024 threads: exclusive scan (sum, or MAX: running maximum) of n_blocks block sums -> base, the total -> *total
template <class T, bool MAX>
__device__ __forceinline__ void scan_block_sums(const T *sums, T *base, uint32_t n_blocks, T *total) {
    __shared__ T part[1024];
    const int tid = threadIdx.x;
    const uint32_t per = (n_blocks + 1023u) / 1024u, lo = (uint32_t)tid * per, hi = min(lo + per, n_blocks);
    T s = 0;
    for (uint32_t k = lo; k < hi; k++) s = MAX ? max(s, sums[k]) : s + sums[k];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        T run = 0;
        for (int k = 0; k < 1024; k++) { const T t = part[k]; part[k] = run; run = MAX ? max(run, t) : run + t; }
        if (total) *total = run;
    }
    __syncthreads();
    T at = part[tid];
    for (uint32_t k = lo; k < hi; k++) { base[k] = at; at = MAX ? max(at, sums[k]) : at + sums[k]; }
}

// thread per record: layout check, anno.d:61-65 (does the record go to the device?), SA, our own tags; block sums
// (The launch is sized from an ESTIMATE of the records the bytes hold — a bound from the bytes alone would be eight times
// too many workgroups, each waiting for a wave slot beside the compressor; the grid strides over the blocks of PACK_BLOCK
// records there really are, whatever the estimate was.)
__global__ __launch_bounds__(PACK_BLOCK) void bam_pack_count_kernel(PackArgs a) {
    __shared__ uint32_t red[16][8];
    const uint32_t n_all = a.counts_in->n_records;
    const uint32_t r1 = min(a.r1_cap, n_all);
    const uint32_t n_blk = r1 > a.r0 ? (r1 - a.r0 + PACK_BLOCK - 1) / PACK_BLOCK : 0u;
    for (uint32_t blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
    const uint32_t i = a.r0 + blk * PACK_BLOCK + threadIdx.x;
    uint32_t info = 0, ncig = 0, nseq = 0, lq = 0, span = 0;
    if (i < r1) {
        const RecHdr r = rec_header(a.u + a.rec_off[i]);
        bool ok = r.bs >= 32u && r.lseq >= 0 && r.lname >= 1u && r.aux_off <= r.end;
        bool sa = false, ours = false;
        if (ok) {
            uint32_t q = r.aux_off;
            while (q < r.end) {
                if (q + 3u > r.end) { ok = false; break; }
                const uint32_t fs = aux_field_size(r.p, q + 2u, r.end);
                if (!fs) { ok = false; break; }
                const uint8_t a0 = r.p[q], a1 = r.p[q + 1];
                sa |= (a0 == 'S' && a1 == 'A');
                ours |= is_ours(a0, a1);
                q += 2u + fs;
            }
        }
        if (!ok) info = INFO_BAD;
        else {
            bool soft = false;
            uint64_t sp = 0;
            for (uint32_t k = 0; k < r.ncig; k++) {
                const uint32_t op = ld32(r.p + r.cig_off + 4u * k);
                soft |= (op & 15u) == 4u;
                if (FADEHIP_OP_CONSUMES_REF(op & 15u)) sp += op >> 4;
            }
            const bool need = !(r.flag & 4u) && soft;
            info = (need ? INFO_NEED : 0u) | (sa ? INFO_SA : 0u) | (ours ? INFO_OURS : 0u);
            if (need) {
                ncig = r.ncig;
                lq = (uint32_t)r.lseq;
                nseq = (lq + 1u) / 2u;
                span = (uint32_t)min(sp, (uint64_t)0x7fffffffu);
            }
        }
        a.info[i - a.r0] = info;
    }
    // block reductions: sums of sent / cig / seq, min / max of l_seq, max span, counts of long queries, bad, ours
    const bool need = (info & INFO_NEED) != 0;
    uint32_t v[8] = {need ? 1u : 0u, ncig, nseq, need ? lq : 0xffffffffu, need ? lq : 0u, span, (need && lq > 512u) ? 1u : 0u,
                     ((info & INFO_BAD) ? 1u : 0u) | ((info & INFO_OURS) ? 0x10000u : 0u)};
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        v[0] += (uint32_t)__shfl_xor((int)v[0], m, 64);
        v[1] += (uint32_t)__shfl_xor((int)v[1], m, 64);
        v[2] += (uint32_t)__shfl_xor((int)v[2], m, 64);
        v[3] = min(v[3], (uint32_t)__shfl_xor((int)v[3], m, 64));
        v[4] = max(v[4], (uint32_t)__shfl_xor((int)v[4], m, 64));
        v[5] = max(v[5], (uint32_t)__shfl_xor((int)v[5], m, 64));
        v[6] += (uint32_t)__shfl_xor((int)v[6], m, 64);
        v[7] += (uint32_t)__shfl_xor((int)v[7], m, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 8; k++) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t[8] = {0, 0, 0, 0xffffffffu, 0, 0, 0, 0};
        for (int w = 0; w < 16; w++) {
            t[0] += red[w][0]; t[1] += red[w][1]; t[2] += red[w][2];
            t[3] = min(t[3], red[w][3]); t[4] = max(t[4], red[w][4]); t[5] = max(t[5], red[w][5]);
            t[6] += red[w][6]; t[7] += red[w][7];
        }
        a.blk_sums[3 * blk + 0] = t[0];
        a.blk_sums[3 * blk + 1] = t[1];
        a.blk_sums[3 * blk + 2] = t[2];
        ChunkCounts *c = a.counts;
        if (t[0]) {
            atomicMin(&c->l_seq_min, t[3]);
            atomicMax(&c->l_seq_max, t[4]);
            atomicMax(&c->span_max, t[5]);
        }
        if (t[6]) atomicAdd(&c->n_long_q, t[6]);
        if (t[7] & 0xffffu) atomicAdd(&c->n_bad_layout, t[7] & 0xffffu);
        if (t[7] >> 16) atomicAdd(&c->n_ours, t[7] >> 16);
    }
    __syncthreads();  // `red` is written again by the block's next round
    }
}

// one block: exclusive scan of the block sums (three columns) -> blk_base, totals -> counts
__global__ __launch_bounds__(1024) void bam_pack_scan_kernel(PackArgs a, uint32_t n_blocks) {
    __shared__ uint32_t part[1024][3];
    const int tid = threadIdx.x;
    {   // (the count kernel wrote sums for the blocks of records there are; beyond them the array holds nothing)
        const uint32_t r1 = min(a.r1_cap, a.counts_in->n_records);
        n_blocks = min(n_blocks, r1 > a.r0 ? (r1 - a.r0 + PACK_BLOCK - 1) / PACK_BLOCK : 0u);
    }
    const uint32_t per = (n_blocks + 1023u) / 1024u, lo = (uint32_t)tid * per, hi = min(lo + per, n_blocks);
    uint32_t s[3] = {0, 0, 0};
    for (uint32_t k = lo; k < hi; k++)
        for (int c = 0; c < 3; c++) s[c] += a.blk_sums[3 * k + c];
    for (int c = 0; c < 3; c++) part[tid][c] = s[c];
    __syncthreads();
    if (tid < 3) {
        uint32_t run = 0;
        for (int k = 0; k < 1024; k++) { const uint32_t t = part[k][tid]; part[k][tid] = run; run += t; }
        if (tid == 0) a.counts->n_sent = run;
        if (tid == 1) a.counts->n_cig = run;
        if (tid == 2) a.counts->n_seq = run;
    }
    __syncthreads();
    uint32_t at[3] = {part[tid][0], part[tid][1], part[tid][2]};
    for (uint32_t k = lo; k < hi; k++)
        for (int c = 0; c < 3; c++) { a.blk_base[3 * k + c] = at[c]; at[c] += a.blk_sums[3 * k + c]; }
}

// thread per record: the sent records' fields, CIGARs and bases into the batch arrays
__global__ __launch_bounds__(PACK_BLOCK) void bam_pack_write_kernel(PackArgs a) {
    __shared__ uint32_t tmp[16];
    const uint32_t n_all = a.counts_in->n_records;
    const uint32_t r1 = min(a.r1_cap, n_all);
    const uint32_t i = a.r0 + blockIdx.x * PACK_BLOCK + threadIdx.x;
    const bool live = i < r1;
    const uint32_t info = live ? a.info[i - a.r0] : 0u;
    const bool need = (info & INFO_NEED) != 0;
    RecHdr r;
    uint32_t ncig = 0, nseq = 0;
    if (need) {
        r = rec_header(a.u + a.rec_off[i]);
        ncig = r.ncig;
        nseq = ((uint32_t)r.lseq + 1u) / 2u;
    }
    uint32_t tot;
    const uint32_t k = a.blk_base[3 * blockIdx.x + 0] + block_scan_1024(need ? 1u : 0u, tmp, &tot);
    const uint32_t c0 = a.blk_base[3 * blockIdx.x + 1] + block_scan_1024(ncig, tmp, &tot);
    const uint32_t q0 = a.blk_base[3 * blockIdx.x + 2] + block_scan_1024(nseq, tmp, &tot);
    if (live) a.sent_of[i - a.r0] = need ? (int32_t)k : -1;
    if (need) {
        a.tid[k] = r.tid;
        a.pos[k] = r.pos;
        a.lseq[k] = r.lseq;
        a.flag[k] = (uint16_t)r.flag;
        a.has_sa[k] = (info & INFO_SA) ? 1 : 0;
        a.cigar_off[k] = c0;
        a.seq_off[k] = q0;
        for (uint32_t j = 0; j < ncig; j++) a.cigar_ops[c0 + j] = ld32(r.p + r.cig_off + 4u * j);
        const uint8_t *s = r.p + r.seq_off;
        for (uint32_t j = 0; j < nseq; j++) a.seq[q0 + j] = s[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.cigar_off[a.counts->n_sent] = a.counts->n_cig;
        a.seq_off[a.counts->n_sent] = a.counts->n_seq;
    }
}

// ============================================================================================ tags
// art_of[sent index] = index of the record's alignment entry when it is an artifact call (anno.d:94-107)
__global__ void bam_art_index_kernel(const fadehip_aln *aln, const uint32_t *n_aln_dev, uint32_t aln_cap, int32_t *art_of, uint32_t n_sent) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = min(*n_aln_dev, aln_cap);
    if (k >= n) return;
    const fadehip_aln &a = aln[k];
    if (a.art && a.read_idx >= 0 && (uint32_t)a.read_idx < n_sent) art_of[a.read_idx] = (int32_t)k;
}

struct Names {
    const char *text;         // contig names back to back
    const uint32_t *off;      // [n + 1]
    int32_t n;
};

__device__ __forceinline__ uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10ull) { v /= 10ull; n++; }
    return n;
}
// a byte sink that either counts or writes
struct Sink {
    uint8_t *d;  // nullptr: count only
    uint32_t n;
    __device__ __forceinline__ void put(uint8_t c) {
        if (d) d[n] = c;
        n++;
    }
    __device__ __forceinline__ void dec(int64_t v) {
        if (v < 0) { put('-'); v = -v; }
        const uint32_t len = dec_len((uint64_t)v);
        if (d) {
            uint64_t x = (uint64_t)v;
            for (uint32_t k = len; k-- > 0;) { d[n + k] = (uint8_t)('0' + x % 10ull); x /= 10ull; }
        }
        n += len;
    }
};

// What anno.d:94-107 adds to one record, given the device's results (one thread; artifact calls are a few per cent of
// the records and their strings a few hundred bytes).  The strings: analysis.d:84-92 / 108-118 + anno.d:98-107, as
// fade_main.cpp:artifact_strings builds them on the host.
struct ArtStrings {
    const RecHdr *r;
    const fadehip_aln *a;
    const Names *nm;
    int lq, nops;
    int64_t apos;
    int64_t plen_l, plen_r;  // -1: that side is absent
    __device__ __forceinline__ void init(const RecHdr *r_, const fadehip_aln *a_, const Names *nm_) {
        r = r_; a = a_; nm = nm_;
        lq = r->lseq;
        nops = min(a->sw.n_ops, FADEHIP_MAX_OPS);
        apos = a->win_start + a->sw.beg_ref;
        const int64_t pos = r->pos;
        plen_l = plen_r = -1;
        if (a->art & 1) {  // analysis.d:84-92
            const int64_t clip = a->clip_left;
            const int64_t overlap = apos >= pos - clip ? apos - (pos - clip) : 0;
            const int64_t lead = (nops > 0 && (a->sw.ops[0] & 15u) == 4u) ? (int64_t)(a->sw.ops[0] >> 4) : 0;
            plen_l = min((int64_t)lq, ((int64_t)lq - lead) + overlap);
            plen_l = max(plen_l, (int64_t)0);
        }
        if (a->art & 2) {  // analysis.d:108-118
            const int64_t clip = a->clip_right;
            int64_t res_al = 0;
            for (int q = 0; q < nops; q++) {
                const uint32_t op = a->sw.ops[q] & 15u;
                if (FADEHIP_OP_CONSUMES_REF(op)) res_al += a->sw.ops[q] >> 4;
            }
            const int64_t lhs = pos + a->aligned_len + clip, rhs = apos + res_al;
            const int64_t overlap = lhs >= rhs ? lhs - rhs : 0;
            const int64_t trail = (nops > 0 && (a->sw.ops[nops - 1] & 15u) == 4u) ? (int64_t)(a->sw.ops[nops - 1] >> 4) : 0;
            plen_r = min((int64_t)lq, ((int64_t)lq - trail) + overlap);
            plen_r = max(plen_r, (int64_t)0);
        }
    }
    __device__ __forceinline__ void am_side(Sink &s) const {
        if (r->tid >= 0 && r->tid < nm->n) {
            for (uint32_t k = nm->off[r->tid]; k < nm->off[r->tid + 1]; k++) s.put((uint8_t)nm->text[k]);
        } else s.put('*');
        s.put(',');
        s.dec(apos);
        s.put(',');
        for (int k = 0; k < nops; k++) {
            s.dec((int64_t)(a->sw.ops[k] >> 4));
            s.put((uint8_t)"MIDNSHP=XB"[min(a->sw.ops[k] & 15u, 9u)]);
        }
    }
    __device__ __forceinline__ uint8_t base_code(int j) const { return (r->p[r->seq_off + ((uint32_t)j >> 1)] >> ((~j & 1) << 2)) & 15; }
    // which: 0 am, 1 as, 2 ar, 3 ab — the string "left;right" without its NUL
    __device__ __forceinline__ void string(int which, Sink &s) const {
        const char *nt16 = "=ACMGRSVTWYHKDBN";
        const uint8_t comp[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};  // util.d:18-20
        const uint8_t *ql = r->p + r->qual_off;
        if (which == 0) {
            if (plen_l >= 0) am_side(s);
            s.put(';');
            if (plen_r >= 0) am_side(s);
            return;
        }
        if (plen_l >= 0) {
            const int pl = (int)plen_l;
            if (which == 1) for (int j = 0; j < pl; j++) s.put((uint8_t)nt16[base_code(j)]);                        // seq[0 : plen]
            if (which == 2) for (int m = lq - pl; m < lq; m++) s.put((uint8_t)nt16[comp[base_code(lq - 1 - m)]]);   // qrc[lq - plen :]
            if (which == 3) for (int j = 0; j < pl; j++) s.put((uint8_t)(ql[j] + 33));                              // bq[0 : plen]
        }
        s.put(';');
        if (plen_r >= 0) {
            const int pr = (int)plen_r;
            if (which == 1) for (int j = lq - pr; j < lq; j++) s.put((uint8_t)nt16[base_code(j)]);                   // seq[lq - plen :]
            if (which == 2) for (int m = 0; m < pr; m++) s.put((uint8_t)nt16[comp[base_code(lq - 1 - m)]]);         // qrc[0 : plen]
            if (which == 3) for (int j = lq - pr; j < lq; j++) s.put((uint8_t)(ql[j] + 33));                        // bq[lq - plen :]
        }
    }
};

// ============================================================================================ hard clip
// `fade annotate --clip` (FADEHIP_BAM_CLIP) / fadehip_clip_batch: filter.d:15-91 clipRead in the pass that writes the records.
// The decision (rs bits 1 and 2) and the lengths (reference bases of the artifact alignment's CIGAR) are THIS run's results,
// never tags read back from the record: a record that came in with a wrong-kind rs:Z or am:i keeps that tag as it is
// (htslib's EINVAL), and `fade out -c` behind `fade annotate` would then clip by the stale tag — the fused pass clips by what
// it computed.  That is the one deliberate difference from the two-step pipeline.
//
// Left (rs & 2): if the length is below the record's aligned length, ops are taken from the front until that many
// reference bases are gone — every query base taken (leading S and I too) drops a base and a quality and counts into a new
// leading H, every reference base moves pos; ops that consume neither go without effect.  Right (rs & 4): the same from the
// back, against what the left step left; pos stays.  A length that is not below the aligned length resets the record: a
// zero-filled one that keeps its name and the bases and qualities as trimmed so far.  Whole ops at a time (min(len, left)),
// not base by base; an op of length zero that the walk reaches is dropped.
__device__ __forceinline__ bool op_consumes_query(uint32_t op) { return (0x193u >> (op & 15u)) & 1u; }  // M I S = X

struct ClipPlan {
    uint32_t mode;          // 0: the record leaves as it is, 1: clipped, 2: reset
    uint32_t sb, lseq;      // first surviving base, number of surviving bases
    int32_t pos;
    uint32_t cf, ce;        // surviving ops [cf, ce) of the record's CIGAR ...
    uint32_t eat_f, eat_b;  // ... less these bases of op cf and of op ce - 1
    uint32_t has_l, has_r, hard_l, hard_r;  // the H ops that go around them
    uint32_t ncig;          // ops of the new CIGAR
    uint32_t bin;
    uint32_t pre;           // bytes in front of the aux area: block_size, fixed fields, name, CIGAR, bases, qualities
};

// (every lane of a record's group computes the same plan: the loads are broadcasts and there is nothing to pass around)
__device__ __forceinline__ ClipPlan clip_plan(const RecHdr &r, uint32_t rs, uint32_t trim_l, uint32_t trim_r) {
    ClipPlan c;
    c.mode = 0;
    if (!(rs & 6u)) return c;
    const uint8_t *cig = r.p + r.cig_off;
    const uint32_t lq = r.lseq > 0 ? (uint32_t)r.lseq : 0u;
    uint64_t aligned = 0;
    for (uint32_t k = 0; k < r.ncig; k++) {
        const uint32_t op = ld32(cig + 4u * k);
        if (FADEHIP_OP_CONSUMES_REF(op & 15u)) aligned += op >> 4;
    }
    c.cf = 0; c.ce = r.ncig;
    c.eat_f = c.eat_b = c.has_l = c.has_r = c.hard_l = c.hard_r = 0;
    int64_t pos = r.pos;
    bool reset = false;
    uint64_t hard_l = 0, hard_r = 0;  // (a CIGAR may claim more query bases than l_seq holds: the bases stop at none left)
    if (rs & 2u) {
        uint64_t t = trim_l;
        if (t < aligned) {  // (so the walk ends inside the CIGAR)
            while (t && c.cf < c.ce) {
                const uint32_t op = ld32(cig + 4u * c.cf), len = op >> 4;
                uint32_t k = len;
                if (FADEHIP_OP_CONSUMES_REF(op & 15u)) { k = (uint32_t)min((uint64_t)len, t); t -= k; pos += k; }
                if (op_consumes_query(op)) hard_l += k;
                if (k == len) c.cf++; else c.eat_f = k;
            }
            aligned -= trim_l;
            c.has_l = 1;
        } else reset = true;
    }
    const uint32_t sb = (uint32_t)min(hard_l, (uint64_t)lq);
    uint32_t left = lq - sb;
    if (!reset && (rs & 4u)) {
        uint64_t t = trim_r;
        if (t < aligned) {
            while (t && c.ce > c.cf) {
                const uint32_t op = ld32(cig + 4u * (c.ce - 1u)), len = (op >> 4) - (c.ce - 1u == c.cf ? c.eat_f : 0u);
                uint32_t k = len;
                if (FADEHIP_OP_CONSUMES_REF(op & 15u)) { k = (uint32_t)min((uint64_t)len, t); t -= k; }
                if (op_consumes_query(op)) hard_r += k;
                if (k == len) c.ce--; else c.eat_b = k;
            }
            aligned -= trim_r;
            c.has_r = 1;
            left -= (uint32_t)min(hard_r, (uint64_t)left);
        } else reset = true;
    }
    c.sb = sb;
    c.lseq = left;
    if (reset) {  // build_rec(name, 0, 0, 0, 0, 0, 0, 0, {}, bases, qualities)
        c.mode = 2;
        c.pos = 0;
        c.ncig = 0;
        c.bin = 4681;  // reg2bin(0, 1)
    } else {
        c.mode = 1;
        c.pos = (int32_t)pos;
        c.hard_l = (uint32_t)hard_l;
        c.hard_r = (uint32_t)hard_r;
        c.ncig = c.has_l + (c.ce - c.cf) + c.has_r;
        // reg2bin over the new span, as build_rec has it
        const int64_t beg = c.pos < 0 ? 0 : c.pos, end = beg + (aligned > 0 ? (int64_t)aligned : 1) - 1;
        c.bin = beg >> 14 == end >> 14 ? (uint32_t)(4681 + (beg >> 14))
              : beg >> 17 == end >> 17 ? (uint32_t)(585 + (beg >> 17))
              : beg >> 20 == end >> 20 ? (uint32_t)(73 + (beg >> 20))
              : beg >> 23 == end >> 23 ? (uint32_t)(9 + (beg >> 23))
              : beg >> 26 == end >> 26 ? (uint32_t)(1 + (beg >> 26)) : 0u;
    }
    c.pre = 36u + r.lname + 4u * c.ncig + (c.lseq + 1u) / 2u + c.lseq;
    return c;
}

// n bytes by the sixteen lanes of a record: (unaligned) dwords, then the bytes that are left
__device__ __forceinline__ void copy16(uint8_t *to, const uint8_t *from, uint32_t n, uint32_t sl) {
    const uint32_t whole = n & ~3u;
    for (uint32_t q = 4u * sl; q < whole; q += 64u) *reinterpret_cast<u32u *>(to + q) = ld32(from + q);
    if (sl < n - whole) to[whole + sl] = from[whole + sl];
}

// op j of a clipped record's new CIGAR (c.mode == 1, j < c.ncig): the new H ops around the surviving ones, the first and
// the last of those less what the walk ate of them
__device__ __forceinline__ uint32_t clip_op(const RecHdr &r, const ClipPlan &c, uint32_t j) {
    const uint32_t idx = c.cf + j - c.has_l;
    if (c.has_l && j == 0u) return (c.hard_l << 4) | 5u;
    if (idx >= c.ce) return (c.hard_r << 4) | 5u;
    return ld32(r.p + r.cig_off + 4u * idx) - (((idx == c.cf ? c.eat_f : 0u) + (idx + 1u == c.ce ? c.eat_b : 0u)) << 4);
}

// The clipped (or reset) record up to its aux area, by the record's sixteen lanes: the fixed fields a dword per lane, the
// name, the new CIGAR an op per lane, the bases — shifted by a nibble when an odd number of them went at the front — and
// the qualities.  bs_out = the record's block_size as it leaves.
__device__ __forceinline__ void clip_write_head(const RecHdr &r, const ClipPlan &c, uint8_t *dst, uint32_t bs_out, uint32_t sl) {
    if (sl < 9u) {
        uint32_t v = c.mode == 2u ? 0u : ld32(r.p + 4u * sl);  // (reset: refID, pos, mapq, flag, mate fields and tlen are zero)
        if (sl == 0u) v = bs_out;
        if (sl == 2u) v = (uint32_t)c.pos;
        if (sl == 3u) v = (c.mode == 2u ? r.lname : (v & 0xffffu)) | (c.bin << 16);
        if (sl == 4u) v = (v & 0xffff0000u) | (c.ncig & 0xffffu);
        if (sl == 5u) v = c.lseq;
        *reinterpret_cast<u32u *>(dst + 4u * sl) = v;
    }
    copy16(dst + 36u, r.p + 36u, r.lname, sl);
    uint8_t *oc = dst + 36u + r.lname;
    for (uint32_t j = sl; j < c.ncig; j += 16u) {
        *reinterpret_cast<u32u *>(oc + 4u * j) = clip_op(r, c, j);
    }
    uint8_t *os = oc + 4u * c.ncig;
    const uint8_t *s = r.p + r.seq_off + (c.sb >> 1);
    const uint32_t nb = (c.lseq + 1u) / 2u, whole = nb & ~3u;
    const bool odd = c.sb & 1u, pad = c.lseq & 1u;  // pad: the last byte's low nibble is no base (zero, as build_rec leaves it)
    for (uint32_t q = 4u * sl; q < whole; q += 64u) {
        uint32_t v = ld32(s + q);
        if (odd) {  // (the byte behind the dword is a byte of the record: bases or, behind them, the first quality)
            const uint64_t w = (uint64_t)v | ((uint64_t)s[q + 4u] << 32);
            v = (uint32_t)((w & 0x0f0f0f0full) << 4) | (uint32_t)((w >> 12) & 0x0f0f0f0full);
        }
        if (pad && q + 4u == nb) v &= 0xf0ffffffu;
        *reinterpret_cast<u32u *>(os + q) = v;
    }
    if (sl < nb - whole) {
        const uint32_t k = whole + sl;
        uint32_t b = odd ? ((uint32_t)s[k] << 4) | ((uint32_t)s[k + 1u] >> 4) : s[k];
        if (pad && k + 1u == nb) b &= 0xf0u;
        os[k] = (uint8_t)b;
    }
    copy16(os + nb, r.p + r.qual_off + c.sb, c.lseq, sl);
}

// reference bases of an artifact alignment's CIGAR: what `fade out -c` parses back from the am tag (filter.d:24-27,58-61)
__device__ __forceinline__ uint32_t art_ref_len(const fadehip_aln *a) {
    const int nops = min(a->sw.n_ops, FADEHIP_MAX_OPS);
    uint32_t n = 0;
    for (int q = 0; q < nops; q++)
        if (FADEHIP_OP_CONSUMES_REF(a->sw.ops[q] & 15u)) n += a->sw.ops[q] >> 4;
    return n;
}

// The record as it leaves: block_size, the record's bytes, and the tags of anno.d:63,94-107 — appended when absent,
// updated the way htslib's bam_aux_update_int / bam_aux_update_str do when the record already carries them (first
// occurrence, in place or replaced at the same position).  One thread; `out` = nullptr counts.  Returns the bytes.
// CLIP: the record is being hard-clipped (clip_plan below); `pre` bytes — block_size, the fixed fields, name, CIGAR, bases and
// qualities as clipped — go in front of the aux area and are written by the caller's lanes, as is block_size.
template <bool CLIP>
__device__ __forceinline__ uint32_t emit_record(const RecHdr &r, uint32_t info, uint8_t rs, const fadehip_aln *a, const Names *nm, uint8_t *out, uint32_t pre = 0) {
    Sink s{out, 4u};  // (block_size is written last)
    ArtStrings st;
    if (a) st.init(&r, a, nm);
    const char tags[5][2] = {{'r', 's'}, {'a', 'm'}, {'a', 's'}, {'a', 'r'}, {'a', 'b'}};
    bool done[5] = {false, a == nullptr, a == nullptr, a == nullptr, a == nullptr};  // (no artifact: the strings are not touched)
    if (!(info & INFO_OURS)) {
        // the body is copied by the caller's wave (rewrite kernel) or counted here
        if constexpr (CLIP) s.n = pre + (r.end - r.aux_off);
        else s.n += r.bs;
    } else {
        // fixed part up to the aux area, then field by field
        if constexpr (CLIP) s.n = pre;
        else for (uint32_t k = 4; k < r.aux_off; k++) s.put(r.p[k]);
        uint32_t q = r.aux_off;
        while (q + 3u <= r.end) {
            const uint32_t fs = aux_field_size(r.p, q + 2u, r.end);
            if (!fs) break;
            int mine = -1;
            for (int t = 0; t < 5; t++)
                if (!done[t] && r.p[q] == (uint8_t)tags[t][0] && r.p[q + 1] == (uint8_t)tags[t][1]) mine = t;
            if (mine < 0) {
                for (uint32_t k = q; k < q + 2u + fs; k++) s.put(r.p[k]);
            } else if (mine == 0) {
                // bam_aux_update_int (htslib sam.c) of a value 0 .. 63: every integer slot is wide enough, it is reused and
                // its type letter becomes the unsigned one of its size ("\0CS\0I"[old_sz]); a non-integer rs: EINVAL, the
                // field stays as it is and nothing is appended
                done[0] = true;
                const uint8_t ot = r.p[q + 2];
                const uint32_t os = (uint32_t)aux_type_size(ot);
                const bool is_int = ot == 'c' || ot == 'C' || ot == 's' || ot == 'S' || ot == 'i' || ot == 'I';
                if (is_int) {
                    s.put('r'); s.put('s');
                    s.put(os == 1u ? 'C' : os == 2u ? 'S' : 'I');
                    s.put(rs);
                    for (uint32_t k = 1; k < os; k++) s.put(0);
                } else {
                    for (uint32_t k = q; k < q + 2u + fs; k++) s.put(r.p[k]);
                }
            } else {
                done[mine] = true;
                if (r.p[q + 2] == 'Z') {
                    s.put((uint8_t)tags[mine][0]); s.put((uint8_t)tags[mine][1]); s.put('Z');
                    st.string(mine - 1, s);
                    s.put(0);
                } else {  // bam_aux_update_str on a tag of another type: EINVAL, unchanged
                    for (uint32_t k = q; k < q + 2u + fs; k++) s.put(r.p[k]);
                }
            }
            q += 2u + fs;
        }
    }
    if (!done[0]) { s.put('r'); s.put('s'); s.put('C'); s.put(rs); }  // bam_aux_update_int of a ubyte: the smallest type
    for (int t = 1; t < 5; t++)
        if (!done[t]) {
            s.put((uint8_t)tags[t][0]); s.put((uint8_t)tags[t][1]); s.put('Z');
            st.string(t - 1, s);
            s.put(0);
        }
    if (!CLIP && out) {
        const uint32_t bs = s.n - 4u;
        out[0] = (uint8_t)bs; out[1] = (uint8_t)(bs >> 8); out[2] = (uint8_t)(bs >> 16); out[3] = (uint8_t)(bs >> 24);
    }
    return s.n;
}

struct TagArgs {
    const uint8_t *u;
    const uint32_t *rec_off;
    const ChunkCounts *counts_in;
    uint32_t r0, r1_cap;
    const uint32_t *info;
    const int32_t *sent_of;
    const uint8_t *rs;         // per sent record
    const fadehip_aln *aln;
    const int32_t *art_of;     // per sent record: alignment entry or -1
    Names names;
    uint32_t *out_size;        // per record of the batch
    uint64_t *blk_sums, *blk_base;
    ChunkCounts *counts;       // out_bytes
    uint64_t out_base;         // bytes of O in front of this batch
    uint8_t *o;
};
__device__ __forceinline__ const fadehip_aln *aln_of(const TagArgs &a, int32_t sent, uint8_t *rs) {
    *rs = 0;
    if (sent < 0) return nullptr;
    *rs = a.rs[sent];
    const int32_t k = a.art_of[sent];
    return k >= 0 ? a.aln + k : nullptr;
}

// CLIP (FADEHIP_BAM_CLIP) is a parameter of the kernels themselves, not of a body they share: <false> is, instruction for
// instruction, the kernel of before the flag existed (a shared body inlined into two kernels was not).
// (Likewise it keeps its own block sum: with block_sum_256 inlined, <false>'s adds came out with their operands swapped.)
template <bool CLIP>
__global__ __launch_bounds__(TAG_BLOCK) void bam_tag_size_kernel(TagArgs a) {
    __shared__ uint64_t red[TAG_BLOCK / 64];
    const uint32_t r1 = min(a.r1_cap, a.counts_in->n_records);
    const uint32_t i = a.r0 + blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;
    if (i < r1) {
        const RecHdr r = rec_header(a.u + a.rec_off[i]);
        uint8_t rs;
        const fadehip_aln *al = aln_of(a, a.sent_of[i - a.r0], &rs);
        const uint32_t info = a.info[i - a.r0];
        if constexpr (CLIP) {
            ClipPlan c;
            c.mode = 0;
            if (al && !(info & INFO_BAD)) {
                const uint32_t trim = art_ref_len(al);
                c = clip_plan(r, rs, trim, trim);
            }
            if (info & INFO_BAD) sz = 0u;
            else if (c.mode == 1u) sz = emit_record<true>(r, info, rs, al, &a.names, nullptr, c.pre);
            else if (c.mode == 2u) sz = c.pre;  // (a reset record has no aux area)
            else sz = emit_record<false>(r, info, rs, al, &a.names, nullptr);
        } else {
            sz = (info & INFO_BAD) ? 0u : emit_record<false>(r, info, rs, al, &a.names, nullptr);
        }
        a.out_size[i - a.r0] = (uint32_t)sz;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sz += (uint64_t)__shfl_xor((long long)sz, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sz;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < TAG_BLOCK / 64; w++) t += red[w];
        a.blk_sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void bam_tag_scan_kernel(TagArgs a, uint32_t n_blocks) {
    scan_block_sums<uint64_t, false>(a.blk_sums, a.blk_base, n_blocks, &a.counts->out_bytes);
}

// Sixteen lanes per record, four records per wavefront at a time: the body moved as (unaligned) dwords by the sixteen, the
// tags written by the first of them.  A record costs a chain of dependent loads (info, offset, header, then the body) —
// a wave that took its records one after the other spent 22 us on each; four chains side by side, and a third of the copy
// instructions.  A block serves the TAG_BLOCK records of one tag-size block (whose base applies) with REWRITE_WAVES waves.
constexpr int REWRITE_WAVES = 16;
template <bool CLIP>
__global__ __launch_bounds__(REWRITE_WAVES * 64) void bam_rewrite_kernel(TagArgs a) {
    __shared__ uint64_t off[TAG_BLOCK];
    __shared__ uint64_t wave_sum[TAG_BLOCK / 64 + 1];
    const uint32_t r1 = min(a.r1_cap, a.counts_in->n_records);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i0 = a.r0 + blockIdx.x * TAG_BLOCK;
    // offsets of the block's records: a scan of out_size by the first TAG_BLOCK threads
    uint64_t sz = 0, inc = 0;
    if (threadIdx.x < TAG_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        sz = i < r1 ? (uint64_t)a.out_size[i - a.r0] : 0ull;
        inc = sz;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wave_sum[wave + 1] = inc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        wave_sum[0] = 0;
        for (int w = 1; w <= TAG_BLOCK / 64; w++) wave_sum[w] += wave_sum[w - 1];
    }
    __syncthreads();
    if (threadIdx.x < TAG_BLOCK) off[threadIdx.x] = a.out_base + a.blk_base[blockIdx.x] + wave_sum[wave] + inc - sz;
    __syncthreads();
    constexpr int PER_WAVE = TAG_BLOCK / REWRITE_WAVES;
    static_assert(PER_WAVE % 4 == 0, "four records per wavefront at a time");
    const uint32_t sub = (uint32_t)lane >> 4, sl = (uint32_t)lane & 15u;
    for (int j = 0; j < PER_WAVE / 4; j++) {
        const uint32_t k = (uint32_t)wave * PER_WAVE + 4u * (uint32_t)j + sub, ij = i0 + k;
        if (ij >= r1) continue;
        const uint32_t info = a.info[ij - a.r0];
        if (info & INFO_BAD) continue;
        const RecHdr r = rec_header(a.u + a.rec_off[ij]);
        uint8_t *dst = a.o + off[k];
        if constexpr (CLIP) {
            // the clipped record: everything in front of the aux area and an aux area that is only copied by the sixteen
            // lanes, the tags (and an aux area that carries some of them already) by the first
            uint8_t rs;
            const fadehip_aln *al = aln_of(a, a.sent_of[ij - a.r0], &rs);
            if (al) {
                const uint32_t trim = art_ref_len(al);
                const ClipPlan c = clip_plan(r, rs, trim, trim);
                if (c.mode) {
                    clip_write_head(r, c, dst, a.out_size[ij - a.r0] - 4u, sl);
                    if (c.mode == 1u) {
                        if (!(info & INFO_OURS)) copy16(dst + c.pre, r.p + r.aux_off, r.end - r.aux_off, sl);
                        if (sl == 0) emit_record<true>(r, info, rs, al, &a.names, dst, c.pre);
                    }
                    continue;
                }
            }
        }
        if (!(info & INFO_OURS)) {
            const uint32_t nbody = r.end - 4u, whole = nbody & ~3u;
            const uint8_t *from = r.p + 4;
            uint8_t *to = dst + 4;
            for (uint32_t q = 4u * sl; q < whole; q += 64u) *reinterpret_cast<u32u *>(to + q) = ld32(from + q);
            if (sl < nbody - whole) to[whole + sl] = from[whole + sl];
        }
        if (sl == 0) {
            uint8_t rs;
            const fadehip_aln *al = aln_of(a, a.sent_of[ij - a.r0], &rs);
            emit_record<false>(r, info, rs, al, &a.names, dst);  // (a record without our tags: its body is counted, not written, here)
        }
    }
}

// ---- fadehip_clip_batch: clip_plan / clip_write_head over records the caller brings, with the caller's rs and lengths
struct ClipBatchArgs {
    const uint8_t *in;
    const uint64_t *in_off;    // [n + 1]
    const uint8_t *rs;         // [n]
    const uint32_t *trim_l, *trim_r;  // [n] reference bases
    uint32_t n;
    uint32_t *out_size;        // [n]   (size kernel)
    const uint64_t *out_off;   // [n]   (write kernel)
    uint8_t *out;
};
__global__ __launch_bounds__(256) void clip_batch_size_kernel(ClipBatchArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const RecHdr r = rec_header(a.in + a.in_off[i]);
    const ClipPlan c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
    a.out_size[i] = c.mode == 2u ? c.pre : c.mode == 1u ? c.pre + (r.end - r.aux_off) : r.end;
}
__global__ __launch_bounds__(256) void clip_batch_write_kernel(ClipBatchArgs a) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
    if (i >= a.n) return;
    const RecHdr r = rec_header(a.in + a.in_off[i]);
    const ClipPlan c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
    uint8_t *dst = a.out + a.out_off[i];
    if (!c.mode) { copy16(dst, r.p, r.end, sl); return; }
    clip_write_head(r, c, dst, a.out_size[i] - 4u, sl);
    if (c.mode == 1u) copy16(dst + c.pre, r.p + r.aux_off, r.end - r.aux_off, sl);
}

// ============================================================================================ extract
// `fade annotate --extract` (FADEHIP_BAM_EXTRACT) / fadehip_extract_batch: remap.d:11-87 (`fade extract`) in the pass that
// writes the records.  One new mapped record per artifact side, left (rs & 2) before right (rs & 4), built from the read as
// it came in (never from the clipped one) and from THIS run's alignment, not from an am tag read back: refID and position
// of the alignment, its padded CIGAR, the read reverse-complemented, its qualities reversed, flag 0x10 when the read has it
// clear, everything else what a zero-filled bam1_t holds (mapq 0, mate refID 0, mate pos 0, tlen 0), no aux area.
// These kernels are of their own: the kernels of a run without the flag are not touched and share no body with them.
__device__ __forceinline__ uint32_t extract_size(const RecHdr &r, uint32_t nops) {
    const uint32_t lq = r.lseq > 0 ? (uint32_t)r.lseq : 0u;
    return 36u + r.lname + 4u * nops + (lq + 1u) / 2u + lq;
}

// One extract record by sixteen lanes.  The bases eight at a time: bit reversal of a dword of 4-bit codes (v_bfrev_b32)
// reverses the order of its eight codes AND complements each (util.d:18-20's table is bit reversal of the code), so the
// dword read from the mirrored end is the output dword; an odd l_seq leaves the input's pad nibble in front of the
// reversed stream, which is shifted out with the nibble shift clip_write_head uses, and the output's own pad nibble is
// zeroed.  The qualities are byte-swapped dwords from the mirrored end.
__device__ __forceinline__ void extract_write(const RecHdr &r, int32_t tid, int64_t pos, const uint32_t *ops, uint32_t nops, uint8_t *dst, uint32_t sl) {
    const uint32_t lq = r.lseq > 0 ? (uint32_t)r.lseq : 0u, nb = (lq + 1u) / 2u;
    if (sl < 9u) {
        uint32_t v = 0u;  // (mate refID, mate pos, tlen)
        if (sl == 0u) v = 32u + r.lname + 4u * nops + nb + lq;
        if (sl == 1u) v = (uint32_t)tid;
        if (sl == 2u) v = (uint32_t)(int32_t)pos;
        if (sl == 3u) {  // l_read_name, mapq 0, reg2bin over the new CIGAR's span
            int64_t reflen = 0;
            for (uint32_t k = 0; k < nops; k++)
                if (FADEHIP_OP_CONSUMES_REF(ops[k] & 15u)) reflen += ops[k] >> 4;
            const int64_t beg = pos < 0 ? 0 : pos, end = beg + (reflen > 0 ? reflen : 1) - 1;
            const uint32_t bin = beg >> 14 == end >> 14 ? (uint32_t)(4681 + (beg >> 14))
                               : beg >> 17 == end >> 17 ? (uint32_t)(585 + (beg >> 17))
                               : beg >> 20 == end >> 20 ? (uint32_t)(73 + (beg >> 20))
                               : beg >> 23 == end >> 23 ? (uint32_t)(9 + (beg >> 23))
                               : beg >> 26 == end >> 26 ? (uint32_t)(1 + (beg >> 26)) : 0u;
            v = r.lname | (bin << 16);
        }
        if (sl == 4u) v = (nops & 0xffffu) | ((r.flag & 0x10u) ? 0u : 0x100000u);
        if (sl == 5u) v = lq;
        *reinterpret_cast<u32u *>(dst + 4u * sl) = v;
    }
    copy16(dst + 36u, r.p + 36u, r.lname, sl);
    uint8_t *oc = dst + 36u + r.lname;
    for (uint32_t j = sl; j < nops; j += 16u) *reinterpret_cast<u32u *>(oc + 4u * j) = ops[j];
    uint8_t *os = oc + 4u * nops;
    const uint8_t *s = r.p + r.seq_off;
    const bool odd = lq & 1u;
    {
        // output bytes [q, q + 4) mirror input bytes [nb - 4 - q, nb - q); with an odd l_seq also the byte in front of them
        // (for the last output dword that is the byte in front of the bases — a byte of the record, name or CIGAR — and
        // what it brings lands in the pad nibble, which is cleared)
        const uint32_t whole = nb & ~3u;
        for (uint32_t q = 4u * sl; q < whole; q += 64u) {
            const uint8_t *m = s + (nb - 4u - q);
            uint32_t v = __builtin_bitreverse32(ld32(m));
            if (odd) {
                const uint64_t w = (uint64_t)v | ((uint64_t)(__builtin_bitreverse32(m[-1]) >> 24) << 32);
                v = (uint32_t)((w & 0x0f0f0f0full) << 4) | (uint32_t)((w >> 12) & 0x0f0f0f0full);
                if (q + 4u == nb) v &= 0xf0ffffffu;
            }
            *reinterpret_cast<u32u *>(os + q) = v;
        }
        if (sl < nb - whole) {
            const uint32_t k = whole + sl;
            const uint8_t *m = s + (nb - 1u - k);
            uint32_t b = __builtin_bitreverse32(m[0]) >> 24;
            if (odd) {
                b = ((b << 4) | (__builtin_bitreverse32(m[-1]) >> 28)) & 0xffu;
                if (k + 1u == nb) b &= 0xf0u;
            }
            os[k] = (uint8_t)b;
        }
    }
    uint8_t *oq = os + nb;
    const uint8_t *ql = r.p + r.qual_off;
    const uint32_t whole = lq & ~3u;
    for (uint32_t q = 4u * sl; q < whole; q += 64u) *reinterpret_cast<u32u *>(oq + q) = __builtin_bswap32(ld32(ql + (lq - 4u - q)));
    if (sl < lq - whole) oq[whole + sl] = ql[lq - 1u - (whole + sl)];
}

// The file path.  TagArgs as the tag kernels have them, with out_size / blk_sums / blk_base / counts / o of the extract
// stream's own (counts: a second ChunkCounts whose out_bytes the scan fills and whose n_records counts extract records).
// Thread per record of a TAG_BLOCK block, so that the sizes feed bam_tag_scan_kernel as the tag sizes do and the records
// come out in input order; a record that is no artifact call costs its thread two index words and nothing of the record.
__global__ __launch_bounds__(TAG_BLOCK) void bam_extract_size_kernel(TagArgs a) {
    const uint32_t r1 = min(a.r1_cap, a.counts_in->n_records);
    const uint32_t i = a.r0 + blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;  // bytes, and the number of records above bit 40
    if (i < r1) {
        uint8_t rs;
        const fadehip_aln *al = aln_of(a, a.sent_of[i - a.r0], &rs);
        if (al && (rs & 6u) && !(a.info[i - a.r0] & INFO_BAD)) {
            const RecHdr r = rec_header(a.u + a.rec_off[i]);
            const uint32_t n = (rs & 6u) == 6u ? 2u : 1u;
            sz = (uint64_t)n * extract_size(r, (uint32_t)min(max(al->sw.n_ops, 0), FADEHIP_MAX_OPS)) | ((uint64_t)n << 40);
        }
        a.out_size[i - a.r0] = (uint32_t)sz;
    }
    const uint64_t t = block_sum_256(sz);
    if (threadIdx.x == 0) {
        a.blk_sums[blockIdx.x] = t & ((1ull << 40) - 1ull);
        if (t >> 40) atomicAdd(&a.counts->n_records, (uint32_t)(t >> 40));
    }
}

// A block per TAG_BLOCK records (whose base applies): the artifact calls among them — a few per cent — are gathered into a
// list by one scan of (bytes, is-a-call), and the block's sixteen groups of sixteen lanes take them side by side, as the
// rewrite kernel takes its records: a record is a chain of dependent loads, and several chains at once hide them.
__global__ __launch_bounds__(TAG_BLOCK) void bam_extract_write_kernel(TagArgs a) {
    __shared__ uint64_t wave_sum[TAG_BLOCK / 64 + 1];
    __shared__ uint64_t l_off[TAG_BLOCK];
    __shared__ uint32_t l_rec[TAG_BLOCK];
    const uint32_t r1 = min(a.r1_cap, a.counts_in->n_records);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i0 = a.r0 + blockIdx.x * TAG_BLOCK, i = i0 + threadIdx.x;
    const uint64_t sz = i < r1 ? (uint64_t)a.out_size[i - a.r0] : 0ull;
    const uint64_t v = sz | (sz ? 1ull << 40 : 0ull);
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave + 1] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        wave_sum[0] = 0;
        for (int w = 1; w <= TAG_BLOCK / 64; w++) wave_sum[w] += wave_sum[w - 1];
    }
    __syncthreads();
    if (sz) {
        const uint64_t ex = wave_sum[wave] + inc - v;
        l_rec[ex >> 40] = threadIdx.x;
        l_off[ex >> 40] = a.out_base + a.blk_base[blockIdx.x] + (ex & ((1ull << 40) - 1ull));
    }
    __syncthreads();
    const uint32_t cnt = (uint32_t)(wave_sum[TAG_BLOCK / 64] >> 40);
    const uint32_t sl = threadIdx.x & 15u;
    for (uint32_t g = threadIdx.x >> 4; g < cnt; g += TAG_BLOCK / 16) {
        const uint32_t ij = i0 + l_rec[g];
        const RecHdr r = rec_header(a.u + a.rec_off[ij]);
        uint8_t rs;
        const fadehip_aln *al = aln_of(a, a.sent_of[ij - a.r0], &rs);  // (never null: the size pass found the call)
        const uint32_t nops = (uint32_t)min(max(al->sw.n_ops, 0), FADEHIP_MAX_OPS);
        const int64_t pos = al->win_start + al->sw.beg_ref;  // what am holds
        uint8_t *dst = a.o + l_off[g];
        extract_write(r, r.tid, pos, al->sw.ops, nops, dst, sl);
        if ((rs & 6u) == 6u) extract_write(r, r.tid, pos, al->sw.ops, nops, dst + extract_size(r, nops), sl);  // (am names the one alignment on both sides)
    }
}

// ---- fadehip_extract_batch: extract_write over records the caller brings; side 2k is the left one of record k, 2k + 1 the right
struct ExtractBatchArgs {
    const uint8_t *in;
    const uint64_t *in_off;    // [n + 1]
    const uint8_t *rs;         // [n]
    const int32_t *tid;        // [2n]
    const int64_t *pos;        // [2n]
    const uint64_t *cig_off;   // [2n + 1]
    const uint32_t *cig;
    uint32_t n;
    uint32_t *out_size;        // [2n]  (size kernel; 0: that side's bit is clear)
    const uint64_t *out_off;   // [2n]  (write kernel)
    uint8_t *out;
};
__global__ __launch_bounds__(256) void extract_batch_size_kernel(ExtractBatchArgs a) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= 2u * a.n) return;
    uint32_t sz = 0;
    if (a.rs[s >> 1] & (2u << (s & 1u))) sz = extract_size(rec_header(a.in + a.in_off[s >> 1]), (uint32_t)(a.cig_off[s + 1u] - a.cig_off[s]));
    a.out_size[s] = sz;
}
__global__ __launch_bounds__(256) void extract_batch_write_kernel(ExtractBatchArgs a) {
    const uint32_t s = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
    if (s >= 2u * a.n || !a.out_size[s]) return;
    const RecHdr r = rec_header(a.in + a.in_off[s >> 1]);
    extract_write(r, a.tid[s], a.pos[s], a.cig + a.cig_off[s], (uint32_t)(a.cig_off[s + 1u] - a.cig_off[s]), a.out + a.out_off[s], sl);
}

// ============================================================================================ eject
// `fade annotate --eject` (FADEHIP_BAM_EJECT / FADEHIP_BAM_EJECT_GROUPS) / fadehip_eject_batch: filter.d:209-265 (plain
// `fade out`) in the pass that writes the records.  An artifact call (rs & 6 of THIS run, never an rs tag read back) is
// not written; in grouped mode neither is any record of its name group — the maximal run of consecutive records with
// byte-equal names.  These kernels are of their own: a run without the flag launches none of them, and they mark an
// ejected record the way the kernels of such a run already understand (out_size 0, INFO_BAD, which the rewrite kernel
// skips by), so those kernels are not touched.
//
// Names are equal when l_read_name and all name bytes are: (unaligned) dwords, the last one masked.  The loads reach up to
// three bytes behind the name — bytes of the record when l_read_name fits block_size, which the callers have checked.
__device__ __forceinline__ bool same_name(const uint8_t *p, const uint8_t *q) {
    const uint32_t ln = p[12];
    if (ln != (uint32_t)q[12]) return false;
    for (uint32_t k = 0; k < ln; k += 4u) {
        uint32_t x = ld32(p + 36u + k) ^ ld32(q + 36u + k);
        if (k + 4u > ln) x &= 0xffffffffu >> (8u * (k + 4u - ln));
        if (x) return false;
    }
    return true;
}

// Grouped mode, a call that is not the last: a name group must not lie across two calls, so the call gives its last group
// back — n_records and consumed are lowered to the group's start, and the carry (the bytes behind `consumed`) moves the
// group into the next call.  One wave, behind bam_frame_compact_kernel: the 64 records in front are compared with the last
// record's name at a time, by ballot.  A call that is one group gives everything back.  (The layout of these records has
// not been checked yet: one whose name does not fit its block_size ends the run of equal names and fails the call later.)
__global__ __launch_bounds__(64) void bam_eject_hold_kernel(FrameArgs a) {
    ChunkCounts *cc = a.counts;
    const uint32_t n = min(cc->n_records, a.rec_cap - 1u);
    if (n == 0 || cc->frame_err) return;
    const uint32_t lane = threadIdx.x;
    const uint8_t *last = a.u + a.rec_off[n - 1u];
    uint32_t start = n - 1u;
    if (32u + last[12] <= ld32(last)) {
        for (uint32_t hi = n - 1u; hi > 0u;) {  // records [start, n) carry the last record's name; hi == start
            bool eq = false;
            if (lane < hi) {
                const uint8_t *p = a.u + a.rec_off[hi - 1u - lane];
                eq = 32u + p[12] <= ld32(p) && same_name(p, last);
            }
            const unsigned long long ne = ~__ballot(eq);
            const uint32_t k = ne ? (uint32_t)__builtin_ctzll(ne) : 64u;
            hi -= k;
            start = hi;
            if (k < 64u) break;
        }
    }
    if (lane == 0) {
        cc->n_records = start;
        cc->consumed = a.rec_off[start];
    }
}

struct EjectArgs {
    const uint8_t *u;
    const uint32_t *off32;     // the file path: rec_off ...
    const uint64_t *off64;     // ... fadehip_eject_batch: in_off (the one that is not null)
    uint32_t n;                // records
    const int32_t *sent_of;    // the file path: rs is per sent record; nullptr: rs is per record
    const uint8_t *rs;
    uint32_t *head_of;         // [n]  bit 31: the record is an artifact call; bits 0-30: 1 + index of its group's first record
    uint32_t *blk_head;        // [blocks of TAG_BLOCK records]  1 + index of the last group start in the block, 0: none
    uint32_t *blk_carry;       // [blocks]  the same over all blocks in front
    uint32_t *grp;             // [n]  at a group's first record: != 0 when a record of the group is an artifact call (zeroed)
    // what the decision goes into: the file path's arrays ...
    uint32_t *out_size, *info;
    uint64_t *blk_sums;
    ChunkCounts *counts;       // n_ejected
    uint8_t *keep;             // ... or fadehip_eject_batch's answer
};
__device__ __forceinline__ const uint8_t *eject_rec(const EjectArgs &a, uint32_t i) { return a.u + (a.off32 ? (uint64_t)a.off32[i] : a.off64[i]); }
__device__ __forceinline__ bool eject_art(const EjectArgs &a, uint32_t i) {
    if (!a.sent_of) return (a.rs[i] & 6u) != 0;
    const int32_t s = a.sent_of[i];
    return s >= 0 && (a.rs[s] & 6u) != 0;  // (a record that never reached the gate has rs 0)
}

// Thread per record: is it the first of its name group (its name differs from the record's in front; record 0 is one), is it
// an artifact call; then a max-scan of (1 + index of a group start) over the block — wave, then the block's four waves —
// leaves every record the start of its group, or 0 when the group began in a block in front.
__global__ __launch_bounds__(TAG_BLOCK) void bam_eject_head_kernel(EjectArgs a) {
    __shared__ uint32_t wmax[TAG_BLOCK / 64];
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = 0;
    bool art = false;
    if (i < a.n) {
        const bool head = i == 0u || !same_name(eject_rec(a, i), eject_rec(a, i - 1u));
        art = eject_art(a, i);
        v = head ? i + 1u : 0u;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wmax[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; w++) v = max(v, wmax[w]);
    if (i < a.n) a.head_of[i] = v | (art ? 0x80000000u : 0u);
    if (threadIdx.x == TAG_BLOCK - 1) a.blk_head[blockIdx.x] = v;  // (threads behind the last record pass the maximum on)
}

// one block: exclusive max-scan of the blocks' last group starts, as bam_tag_scan_kernel sums the blocks' bytes
__global__ __launch_bounds__(1024) void bam_eject_scan_kernel(EjectArgs a, uint32_t n_blocks) {
    scan_block_sums<uint32_t, true>(a.blk_head, a.blk_carry, n_blocks, nullptr);
}

// thread per record: the group start is final now; an artifact call leaves its mark at the group's first record
__global__ __launch_bounds__(TAG_BLOCK) void bam_eject_mark_kernel(EjectArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t w = a.head_of[i];
    uint32_t h = w & 0x7fffffffu;
    if (!h) {
        h = a.blk_carry[blockIdx.x];  // (never 0: record 0 starts a group)
        a.head_of[i] = w | h;
    }
    if (w >> 31) atomicOr(&a.grp[h - 1u], 1u);
}

// thread per record: the decision, applied.  The file path: an ejected record gets out_size 0 and INFO_BAD, and the block's
// bytes are summed again — in front of bam_tag_scan_kernel, so that the offsets never hold it; fadehip_eject_batch: keep[].
__global__ __launch_bounds__(TAG_BLOCK) void bam_eject_apply_kernel(EjectArgs a, int grouped) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;  // bytes, and the number of ejected records above bit 40
    if (i < a.n) {
        const bool ej = grouped ? a.grp[(a.head_of[i] & 0x7fffffffu) - 1u] != 0u : eject_art(a, i);
        if (a.keep) a.keep[i] = ej ? 0 : 1;
        if (a.out_size) {
            if (ej) {
                a.out_size[i] = 0u;
                a.info[i] |= INFO_BAD;
                sz = 1ull << 40;
            } else sz = a.out_size[i];
        }
    }
    if (!a.out_size) return;  // (uniform)
    const uint64_t t = block_sum_256(sz);
    if (threadIdx.x == 0) {
        a.blk_sums[blockIdx.x] = t & ((1ull << 40) - 1ull);
        if (t >> 40) atomicAdd(&a.counts->n_ejected, (uint32_t)(t >> 40));
    }
}

// ============================================================================================ tags read back
// fadehip_tags_batch: rs and am out of records that were annotated earlier — by this library, by the reference, or by a
// tool in between — into the arrays the clip, eject and extract kernels take (remap.d:31-50, filter.d:24-25,58-59,190-196).
// The first field named rs and the first named am count, as with bam_aux_get.  rs is what tag.to!ubyte makes of an integer
// field: the low byte of its little-endian value, whatever its width; a field of another type is no rs.  am:Z is
// "left;right", cut at its first ';' (without one: everything is the left side), a side "name,pos,cigar".
struct TagsRead {
    uint32_t am_off, am_len;  // the am:Z string (without its NUL), relative to the record; 0, 0: none
    uint8_t rs, have;         // have: bit 0 an integer rs, bit 1 an am of type Z
    bool whole;               // the aux area is whole fields
};
__device__ __forceinline__ TagsRead read_tags(const RecHdr &r) {
    TagsRead t;
    t.am_off = t.am_len = 0u;
    t.rs = t.have = 0;
    t.whole = r.aux_off <= r.end;
    bool seen_rs = false, seen_am = false;
    uint32_t q = r.aux_off;
    while (t.whole && q < r.end) {
        if (q + 3u > r.end) { t.whole = false; break; }
        const uint32_t fs = aux_field_size(r.p, q + 2u, r.end);
        if (!fs) { t.whole = false; break; }
        const uint8_t a0 = r.p[q], a1 = r.p[q + 1], ty = r.p[q + 2];
        if (a0 == 'r' && a1 == 's' && !seen_rs) {
            seen_rs = true;
            if (ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I') {
                t.rs = r.p[q + 3];
                t.have |= 1;
            }
        }
        if (a0 == 'a' && a1 == 'm' && !seen_am) {
            seen_am = true;
            if (ty == 'Z') {
                t.am_off = q + 3u;
                t.am_len = fs - 2u;
                t.have |= 2;
            }
        }
        q += 2u + fs;
    }
    if (!t.whole) {
        t.am_off = t.am_len = 0u;
        t.rs = t.have = 0;
    }
    return t;
}

// the BAM code of a CIGAR letter (MIDNSHP=XB), 0xff for any other byte
__device__ __forceinline__ uint32_t cigar_op_of(uint32_t c) {
    switch (c) {
        case 'M': return 0u;
        case 'I': return 1u;
        case 'D': return 2u;
        case 'N': return 3u;
        case 'S': return 4u;
        case 'H': return 5u;
        case 'P': return 6u;
        case '=': return 7u;
        case 'X': return 8u;
        case 'B': return 9u;
        default: return 0xffu;
    }
}
// One CIGAR of am, as text: pairs of a count (digits, a value below 2^28) and a letter of MIDNSHP=XB, or nothing at all.
// Returns whether all n bytes are such pairs; *nops their number, *ref the reference bases they take.
__device__ __forceinline__ bool am_cigar(const uint8_t *s, uint32_t n, uint32_t *nops, uint64_t *ref) {
    uint32_t num = 0, k = 0;
    uint64_t sum = 0;
    bool digits = false;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t c = s[j];
        if (c - '0' < 10u) {
            num = num * 10u + (c - '0');
            if (num >= (1u << 28)) return false;
            digits = true;
            continue;
        }
        const uint32_t op = cigar_op_of(c);
        if (op == 0xffu || !digits) return false;
        if (FADEHIP_OP_CONSUMES_REF(op)) sum += num;
        k++;
        num = 0;
        digits = false;
    }
    *nops = k;
    *ref = sum;
    return !digits;
}

// The contigs' names, as fadehip_tags_batch uploads them: the bytes back to back, their offsets, and for every contig the
// first one that carries the same name (itself, unless a header names a contig twice).
struct RefNames {
    const uint8_t *bytes;
    const uint32_t *off;    // [n_ref + 1]
    const int32_t *first;   // [n_ref]
    int32_t n_ref;
};
__device__ __forceinline__ bool name_is(const RefNames &nm, int32_t c, const uint8_t *s, uint32_t n) {
    const uint32_t o = nm.off[c];
    if (nm.off[c + 1] - o != n) return false;
    for (uint32_t j = 0; j < n; j++)
        if (nm.bytes[o + j] != s[j]) return false;
    return true;
}
// the first contig named s[0 .. n), or -1: the record's own contig is tried first (what annotate writes), then the table
__device__ __forceinline__ int32_t tid_of_name(const RefNames &nm, int32_t own, const uint8_t *s, uint32_t n) {
    if (!n) return -1;
    if (own >= 0 && own < nm.n_ref && name_is(nm, own, s, n)) return nm.first[own];
    for (int32_t c = 0; c < nm.n_ref; c++)
        if (name_is(nm, c, s, n)) return c;
    return -1;
}

struct AmSide {
    bool ok;            // "name,pos,cigar", each part as the grammar has it
    int32_t tid;
    int64_t pos;
    uint32_t nops, cig_at;  // ops of the CIGAR; where its text starts, relative to the record
    int32_t trim;       // the reference bases its ops take, at most INT32_MAX
};
// one side of am, s[0 .. n) at offset `at` of the record.  pos is what std.conv.to!long takes: a sign or none, digits, no
// more, a value of 64 bits.
__device__ __forceinline__ AmSide am_side(const RecHdr &r, const RefNames &nm, uint32_t at, uint32_t n) {
    AmSide a;
    a.ok = false;
    a.tid = -1;
    a.pos = 0;
    a.nops = 0u;
    a.cig_at = 0u;
    a.trim = 0;
    const uint8_t *s = r.p + at;
    uint32_t c1 = 0;
    while (c1 < n && s[c1] != ',') c1++;
    if (c1 >= n) return a;
    uint32_t c2 = c1 + 1u;
    while (c2 < n && s[c2] != ',') c2++;
    if (c2 >= n) return a;
    uint32_t j = c1 + 1u;
    const bool neg = s[j] == '-';
    if (s[j] == '-' || s[j] == '+') j++;  // (s[c2] is the comma: j stays within the side)
    if (j >= c2) return a;
    uint64_t mag = 0;
    for (; j < c2; j++) {
        const uint32_t d = (uint32_t)s[j] - '0';
        if (d >= 10u || mag > 922337203685477580ull) return a;
        mag = mag * 10ull + d;  // (at most 9223372036854775809: no wrap)
    }
    if (mag > 0x7fffffffffffffffull + (neg ? 1ull : 0ull)) return a;
    uint32_t nops;
    uint64_t ref;
    if (!am_cigar(s + c2 + 1u, n - c2 - 1u, &nops, &ref)) return a;
    a.ok = true;
    a.tid = tid_of_name(nm, r.tid, s, c1);
    a.pos = neg ? (int64_t)(0ull - mag) : (int64_t)mag;
    a.nops = nops;
    a.cig_at = at + c2 + 1u;
    a.trim = (int32_t)min(ref, (uint64_t)0x7fffffffu);
    return a;
}

// exclusive sum of v over a block of TAG_BLOCK threads, the block's total to every thread
__device__ __forceinline__ uint64_t block_scan_256(uint64_t v, uint64_t *total) {
    __shared__ uint64_t wsum[TAG_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
    for (int w = 0; w < TAG_BLOCK / 64; w++) {
        const uint64_t t = wsum[w];
        if (w < wave) base += t;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

struct TagsArgs {
    const uint8_t *in;
    const uint64_t *in_off;   // [n + 1]
    uint32_t n;
    RefNames names;
    uint8_t *rs, *have;       // [n]
    int32_t *trim_l, *trim_r; // [n]
    int32_t *tid;             // [2n]
    int64_t *pos;             // [2n]
    uint32_t *cnt, *cig_at;   // [2n]  ops of a side; where its CIGAR text starts (count kernel -> write kernel)
    uint64_t *blk_sums, *blk_base;  // [blocks of TAG_BLOCK records]
    uint64_t *total;          // ops of the call
    uint32_t *bad;            // the first record whose aux area is not whole fields (0xffffffff: none)
    uint64_t *cig_off;        // [2n + 1]
    uint32_t *cig;            // [*total]
};

// pass 1, thread per record: everything but the ops — rs, have, both sides' contig, position and trim, their op counts
__global__ __launch_bounds__(TAG_BLOCK) void tags_count_kernel(TagsArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t ops = 0;
    if (i < a.n) {
        const RecHdr r = rec_header(a.in + a.in_off[i]);
        const TagsRead t = read_tags(r);
        if (!t.whole) atomicMin(a.bad, i);
        uint32_t semi = 0;
        while (semi < t.am_len && r.p[t.am_off + semi] != ';') semi++;
        uint8_t have = t.have;
        int32_t trim[2];
        for (uint32_t side = 0; side < 2u; side++) {
            AmSide s;
            if (!(t.have & 2)) s = am_side(r, a.names, 0u, 0u);  // (no text: not well-formed)
            else if (side == 0u) s = am_side(r, a.names, t.am_off, semi);
            else s = am_side(r, a.names, t.am_off + min(semi + 1u, t.am_len), t.am_len - min(semi + 1u, t.am_len));
            if (s.ok) have |= (uint8_t)(4u << side);
            a.tid[2u * i + side] = s.tid;
            a.pos[2u * i + side] = s.pos;
            a.cnt[2u * i + side] = s.nops;
            a.cig_at[2u * i + side] = s.cig_at;
            trim[side] = s.trim;
            ops += s.nops;
        }
        a.rs[i] = t.rs;
        a.have[i] = have;
        a.trim_l[i] = trim[0];
        a.trim_r[i] = trim[1];
    }
    const uint64_t tot = block_sum_256(ops);
    if (threadIdx.x == 0) a.blk_sums[blockIdx.x] = tot;
}

// pass 2, one block: where every block's ops start, and how many there are
__global__ __launch_bounds__(1024) void tags_scan_kernel(TagsArgs a, uint32_t n_blocks) {
    scan_block_sums<uint64_t, false>(a.blk_sums, a.blk_base, n_blocks, a.total);
}

// pass 3, thread per record: the sides' offsets by a scan over the block, then the ops, parsed again from the text
__global__ __launch_bounds__(TAG_BLOCK) void tags_write_kernel(TagsArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint32_t nl = 0, nr = 0;
    if (i < a.n) {
        nl = a.cnt[2u * i];
        nr = a.cnt[2u * i + 1u];
    }
    uint64_t tot;
    const uint64_t at = a.blk_base[blockIdx.x] + block_scan_256((uint64_t)nl + nr, &tot);
    if (i >= a.n) return;
    a.cig_off[2u * i] = at;
    a.cig_off[2u * i + 1u] = at + nl;
    if (i + 1u == a.n) a.cig_off[2u * i + 2u] = at + nl + nr;
    const uint8_t *p = a.in + a.in_off[i];
    for (uint32_t side = 0; side < 2u; side++) {
        const uint32_t nops = side ? nr : nl;
        if (!nops) continue;
        // the side was found well-formed: its CIGAR text ends where the nops-th op letter stands
        const uint8_t *s = p + a.cig_at[2u * i + side];
        uint32_t *dst = a.cig + at + (side ? nl : 0u);
        uint32_t num = 0, k = 0;
        for (uint32_t j = 0; k < nops; j++) {
            const uint32_t c = s[j];
            if (c - '0' < 10u) { num = num * 10u + (c - '0'); continue; }
            dst[k++] = (num << 4) | cigar_op_of(c);
            num = 0;
        }
    }
}

}  // namespace bam
}  // namespace fadehip
