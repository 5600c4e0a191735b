// bam_sortwin.hpp — FADEHIP_BAM_STORE_OUTPUT: a stream's output records stay on the device, in a record store
// (bam_recstore.hpp), which sorts them by coordinate once the input has passed — for inputs in any order.
// A file whose records do not fit the device at once is written in windows of the key space: the first pass over the input
// measures, per bucket of 2^SW_SHIFT positions, the bytes and records that leave (host/recstore_host.hpp cuts the windows from
// that table), and every later pass keeps only the records whose key lies in its window.
//
//   key     bam_resort.hpp's rs_key(refID, pos) of the record AS IT LEAVES: a clipped record at its new pos, a reset record
//           RS_KEY_UNMAPPED.  But for the reset record that is what recstore_append_kernel reads from the written record's own
//           bytes; bam_sortwin_rekey_kernel gives a clipping stream's items the keys computed here
//   bucket  first[r] + min(uint32(key) >> SW_SHIFT, nb[r] - 1); refID -1 or outside the header: the last bucket
//
// The window kernel runs behind the kernels that decide which records leave (eject apply, eject named, the mate plan) and in front of
// bam_tag_scan_kernel, so that the offsets never hold a record it removes.  A run without the flag does not launch it.
#pragma once
#include "bam_device.hpp"
#include "bam_from_tags.hpp"
#include "bam_recstore.hpp"
#include "bam_resort.hpp"

namespace fadehip {
namespace bam {

constexpr uint32_t SW_SHIFT = 16;
// buckets a wavefront adds up by ballot, one after the other, before the lanes left over fall back to atomics of their own:
// coordinate-sorted input has one or two per wavefront, name-collated pairs a handful
constexpr int SW_WAVE_BUCKETS = 4;

struct SortWinArgs {
    const uint8_t *u;
    const uint32_t *rec_off;
    uint32_t n, clip;                // records; FADEHIP_BAM_CLIP: the key follows the clip plan
    // what the decision goes into: bam_eject_apply_kernel's arrays
    uint32_t *out_size, *info;
    uint64_t *blk_sums;
    ChunkCounts *counts;             // pad1: records outside the window; pad2: records that remain | reset records among all that leave << 32
    // measure (table != nullptr): bytes [n_buckets], then records [n_buckets]
    unsigned long long *table;
    const uint32_t *first, *nb;      // [n_ref]
    uint32_t n_ref, n_buckets;
    uint64_t lo, hi;                 // the window, both ends inclusive
    uint64_t *leave_key;             // [n] or nullptr: the key of every record that remains, for bam_sortwin_rekey_kernel
};

// The key of record i as it leaves: bam_resort_keys_kernel's lines, restated (the clip plan the rewrite will follow).
template <bool FROM_TAGS>
__device__ __forceinline__ uint64_t leave_key(const RecHdr &r, uint32_t i, bool clip, const TagArgs &ta, const FromTagsArgs &fa, bool *reset) {
    ClipPlan c;
    c.mode = 0;
    if (clip) {
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
    }
    *reset = c.mode == 2u;
    return c.mode == 2u ? RS_KEY_UNMAPPED : c.mode == 1u ? rs_key(r.tid, c.pos) : rs_key(r.tid, r.pos);
}

__device__ __forceinline__ uint32_t sw_bucket(const SortWinArgs &a, uint64_t key) {
    const uint32_t r = (uint32_t)(key >> 32);
    if (r >= a.n_ref) return a.n_buckets - 1u;
    return a.first[r] + min((uint32_t)key >> SW_SHIFT, a.nb[r] - 1u);
}

// Thread per record of a TAG_BLOCK block.  Of every record that still leaves: its bytes and 1 into its bucket (summed over
// the wavefront's lanes of one bucket first — integer sums, exact in any order); outside the window it goes as an ejected
// record goes (out_size 0, INFO_BAD); then the block's bytes again, and the records that remain.
template <bool FROM_TAGS>
__global__ __launch_bounds__(TAG_BLOCK) void bam_sortwin_kernel(SortWinArgs a, TagArgs ta, FromTagsArgs fa) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t sz = i < a.n ? a.out_size[i] : 0u;
    uint64_t key = 0;
    bool reset = false;
    if (sz) key = leave_key<FROM_TAGS>(rec_header(a.u + a.rec_off[i]), i, a.clip != 0u, ta, fa, &reset);
    // (reset records are rare: a wavefront that has some adds their number itself — the driver refuses to index a file that ends in them)
    const unsigned long long resets = __ballot(reset);
    if (resets && lane == 0u) atomicAdd((unsigned long long *)&a.counts->pad2, (unsigned long long)__popcll(resets) << 32);
    if (a.table) {  // (uniform)
        const uint32_t b = sz ? sw_bucket(a, key) : 0u;
        bool pending = sz != 0u;
        for (int round = 0; round < SW_WAVE_BUCKETS; round++) {
            const unsigned long long todo = __ballot(pending);
            if (!todo) break;
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t lb = (uint32_t)__shfl((int)b, (int)leader, 64);
            const bool mine = pending && b == lb;
            const unsigned long long peers = __ballot(mine);
            uint64_t s = mine ? (uint64_t)sz : 0ull;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += (uint64_t)__shfl_xor((long long)s, m, 64);
            if (lane == leader) {
                atomicAdd(&a.table[lb], (unsigned long long)s);
                atomicAdd(&a.table[a.n_buckets + lb], (unsigned long long)__popcll(peers));
            }
            pending = pending && !mine;
        }
        if (pending) {
            atomicAdd(&a.table[b], (unsigned long long)sz);
            atomicAdd(&a.table[a.n_buckets + b], 1ull);
        }
    }
    // bytes below bit 40, records outside the window from bit 40, records that remain from bit 52 (a block holds 256)
    uint64_t v = 0;
    if (sz) {
        if (key < a.lo || key > a.hi) {
            a.out_size[i] = 0u;
            a.info[i] |= INFO_BAD;
            v = 1ull << 40;
        } else {
            v = (uint64_t)sz | (1ull << 52);
            if (a.leave_key) a.leave_key[i] = key;
        }
    }
    const uint64_t t = block_sum_256(v);
    if (threadIdx.x == 0) {
        a.blk_sums[blockIdx.x] = t & ((1ull << 40) - 1ull);
        const uint32_t n_out = (uint32_t)(t >> 40) & 0xfffu, n_in = (uint32_t)(t >> 52);
        if (n_out) atomicAdd(&a.counts->pad1, n_out);
        if (n_in) atomicAdd((unsigned long long *)&a.counts->pad2, (unsigned long long)n_in);
    }
}

// Behind recstore_append_kernel, under FADEHIP_BAM_CLIP: the append reads an item's key from the record as it lies in the arena,
// and a reset record lies there zero-filled (refID 0, pos 0) while it leaves as an unmapped one (§3.8h).  Thread per slot: the
// item of every record that remains — found as the append found it, one item per slot of 36 bytes or more — takes the key the
// window was decided by.  One item per slot: the rewrite kernels write exactly one record of out_size = block_size + 4 bytes
// into a slot, so recstore_slot counts 1 where this kernel does; a main-output slot of two records does not exist, and if one
// ever did the host's check of the sorted bytes against the arena (fadehip_recstore_sort) would still hold, the order would not.
__global__ __launch_bounds__(TAG_BLOCK) void bam_sortwin_rekey_kernel(RecAppendArgs a, const uint64_t *leave_key) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const uint32_t c = i < a.n && a.x_size[i] >= 36u ? 1u : 0u;
    uint64_t tot;
    const uint32_t k = a.cnt_base[blockIdx.x] + (uint32_t)block_scan_256(c, &tot);
    if (c && k < a.n_items) a.s.key[a.item0 + k] = leave_key[i];
}

}  // namespace bam
}  // namespace fadehip
