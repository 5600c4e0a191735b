// bam_intervals.hpp — a set of genomic intervals resident in HBM and the overlap query over it: fadehip_intervals_*, and the
// two columns `fade stats --repeats` appends to a row.  An interval is (chrom id, start, end), 0-based
// half-open, 0 <= start < end <= 2^31 - 1; a query (chrom id, qs, qe) of int64 hits iff qs < qe and the set holds an interval
// of that chrom with start < qe and qs < end — `bedtools subtract -A`'s "any overlap of at least one base", negated.
//
//   raw     what add brings, in the order it came: key = chrom << 32 | start, the end, the item number, written by
//           intervals_key_kernel, which also validates; the first bad interval is named through ctl->bad (RepCtl's idiom) and
//           the host then leaves the call's items out
//   sort    bam_resort.hpp's stable LSD radix sort (histogram, scan and scatter kernels as they stand) over the keys and the
//           item numbers, as bam_recstore.hpp calls it
//   sealed  per interval in order of (chrom id, start): start [] u32, and maxend [] u64 = chrom id << 32 | end under an
//           INCLUSIVE RUNNING MAXIMUM.  Chrom ids rise along the order, so the plain 64-bit maximum is segmented by contig
//           already: an entry of a later contig is above every entry of an earlier one whatever the ends are, and a long
//           interval at the end of one contig cannot reach into the next.  chrom_first [n_chrom + 1]: each contig's range
//   query   j = the contig's intervals with start < qe (a binary search inside the contig's range); the query hits iff
//           qs < qe, j > 0 and the low word of maxend[first + j - 1] is > qs: about log2(n) probes, no list walked
//
// All kernels here are new; a run without a set launches none of them.
#pragma once
#include "bam_device.hpp"
#include "bam_report.hpp"
#include "bam_resort.hpp"

namespace fadehip {
namespace bam {

constexpr int64_t IV_MAX_END = 0x7fffffffll;  // 2^31 - 1

struct IvCtl {
    unsigned long long bad;  // 0: none; else ((0xffffffff - index in the call) << 8) | 1: the first interval that fails the call
    unsigned long long pad;
};

// what add uploads, and where its items go
struct IvAddArgs {
    const int32_t *chrom;         // [n] the caller's
    const int64_t *start, *end;   // [n]
    uint32_t n, item0;            // the call's intervals; items in the set in front of them
    int32_t n_chrom;
    uint64_t *key;                // [items] chrom << 32 | start
    uint32_t *end32, *idx;        // [items] the end; the item's number
    IvCtl *ctl;
};

// thread per interval: chrom in range and 0 <= start < end <= 2^31 - 1, else the call fails at the first such interval
__global__ __launch_bounds__(256) void intervals_key_kernel(IvAddArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const int32_t c = a.chrom[i];
    const int64_t s = a.start[i], e = a.end[i];
    if (c < 0 || c >= a.n_chrom || s < 0 || s >= e || e > IV_MAX_END) {
        atomicMax(&a.ctl->bad, ((unsigned long long)(0xffffffffu - i) << 8) | 1ull);
        return;
    }
    a.key[a.item0 + i] = ((uint64_t)(uint32_t)c << 32) | (uint32_t)s;
    a.end32[a.item0 + i] = (uint32_t)e;
    a.idx[a.item0 + i] = a.item0 + i;
}

// the sealed set, as the query kernels read it
struct IvSetRef {
    const uint32_t *start;        // [n]
    const uint64_t *maxend;       // [n]
    const uint32_t *chrom_first;  // [n_chrom + 1]
    uint32_t n;
    int32_t n_chrom;
};

struct IvSealArgs {
    const uint64_t *key;          // [n] in final order (the sort's side 0)
    const uint32_t *idx;          // [n] the items' numbers in final order
    const uint32_t *end32;        // [items] by item number
    uint32_t n;
    int32_t n_chrom;
    uint32_t *start;              // [n]
    uint64_t *maxend;             // [n]
    uint64_t *blk_max, *blk_carry;  // [blocks of 256]
    uint32_t *chrom_first;        // [n_chrom + 1]
};

// thread per interval in final order: its start, and chrom id << 32 | end
__global__ __launch_bounds__(256) void intervals_gather_kernel(IvSealArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t k = a.key[j];
    a.start[j] = (uint32_t)k;
    a.maxend[j] = (k & 0xffffffff00000000ull) | a.end32[a.idx[j]];
}

// inclusive running maximum of v over a block of 256 threads
__device__ __forceinline__ uint64_t iv_block_max_scan(uint64_t v) {
    __shared__ uint64_t wmax[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
        if (lane >= d) inc = max(inc, o);
    }
    if (lane == 63) wmax[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; w++) inc = max(inc, wmax[w]);
    return inc;
}

// the max-scan, first step: within every block of 256 entries, and the blocks' maxima
__global__ __launch_bounds__(256) void intervals_block_max_kernel(IvSealArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const uint64_t m = iv_block_max_scan(j < a.n ? a.maxend[j] : 0ull);
    if (j < a.n) a.maxend[j] = m;
    if (threadIdx.x == 255u) a.blk_max[blockIdx.x] = m;
}

// second step, one block: every block's maximum of the blocks in front
__global__ __launch_bounds__(1024) void intervals_max_scan_kernel(IvSealArgs a, uint32_t n_blocks) {
    scan_block_sums<uint64_t, true>(a.blk_max, a.blk_carry, n_blocks, (uint64_t *)nullptr);
}

// third step: the carry into every entry
__global__ __launch_bounds__(256) void intervals_max_apply_kernel(IvSealArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < a.n) a.maxend[j] = max(a.maxend[j], a.blk_carry[blockIdx.x]);
}

// thread per contig (and one behind the last): where its intervals start in final order — the first key >= chrom << 32
__global__ __launch_bounds__(256) void intervals_chrom_first_kernel(IvSealArgs a) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c > (uint32_t)a.n_chrom) return;
    const uint64_t want = (uint64_t)c << 32;
    uint32_t lo = 0, hi = a.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.key[mid] < want) lo = mid + 1u;
        else hi = mid;
    }
    a.chrom_first[c] = lo;
}

// the rule: does the set hold an interval of contig c that shares a base with [qs, qe)?  c outside the set: no
__device__ __forceinline__ bool iv_overlaps(const IvSetRef &s, int32_t c, int64_t qs, int64_t qe) {
    if (c < 0 || c >= s.n_chrom || qs >= qe) return false;
    const uint32_t first = s.chrom_first[c];
    uint32_t lo = first, hi = s.chrom_first[c + 1];
    while (lo < hi) {  // the contig's intervals with start < qe are a prefix of its range
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)s.start[mid] < qe) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == first) return false;
    return (int64_t)(uint32_t)s.maxend[lo - 1u] > qs;  // (the low word: the largest end among them)
}

struct IvQueryArgs {
    IvSetRef s;
    const int32_t *chrom;        // [n]
    const int64_t *start, *end;  // [n]
    uint32_t n;
    uint8_t *hit;                // [n]
};

__global__ __launch_bounds__(256) void intervals_overlap_kernel(IvQueryArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    a.hit[i] = iv_overlaps(a.s, a.chrom[i], a.start[i], a.end[i]) ? 1u : 0u;
}

// ---- the report's two columns
struct RepeatArgs {
    IvSetRef s;
    const int32_t *ref_chrom;    // [n_ref] the set's chrom id of every contig of the header, by name bytes; -1: the set has none
    const uint8_t *name_bytes;   // the set's own names back to back ...
    const uint32_t *name_off;    // ... [n_chrom + 1]
    uint8_t *rpm;                // [2n] per slot: bit 0 read_rpm, bit 1 art_rpm
};

// Thread per slot, behind report_stage_kernel: the two queries of the slot's row, in the values the row prints — read_rpm is
// (rname, art_start, art_end), art_rpm is (aln_rname, aln_start, aln_end).  aln_rname is the am side's name as its bytes
// stand: through the header where the header carries it, else looked up in the set's own names.
__global__ __launch_bounds__(TAG_BLOCK) void report_repeats_kernel(RepArgs a, RepeatArgs q) {
    const size_t s = (size_t)blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (s >= 2 * (size_t)a.n) return;
    uint8_t bits = 0;
    if (a.kind[0][s]) {
        const StatsRow &w = a.srow[s];
        const RecHdr r = rec_header(rep_rec(a, (uint32_t)(s >> 1)));
        if (iv_overlaps(q.s, q.ref_chrom[r.tid], w.art0, w.art1)) bits |= 1u;  // (a row's refID is inside the header: the stage's rule)
        const uint8_t *nm = r.p + w.am_at;
        const int32_t t = tid_of_name(a.names, r.tid, nm, w.am_name_len);
        int32_t c = -1;
        if (t >= 0) c = q.ref_chrom[t];
        else
            for (int32_t k = 0; k < q.s.n_chrom && c < 0; k++) {
                const uint32_t o = q.name_off[k];
                if (q.name_off[k + 1] - o != w.am_name_len) continue;
                uint32_t m = 0;
                while (m < w.am_name_len && q.name_bytes[o + m] == nm[m]) m++;
                if (m == w.am_name_len) c = k;
            }
        if (iv_overlaps(q.s, c, (int64_t)w.aln_start, w.aln_end)) bits |= 2u;
    }
    q.rpm[s] = bits;
}

}  // namespace bam
}  // namespace fadehip
