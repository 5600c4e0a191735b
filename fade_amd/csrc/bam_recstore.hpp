// bam_recstore.hpp — a store of BAM records resident in HBM: fadehip_recstore_* (DESIGN.md §3.8l).  Records are added in
// any order over a whole run, sorted once by coordinate, and drained in final order through the compressor and the index
// stage — what a sorted, indexed `fade extract` output needs, whose records lie at their artifact alignments and so in an
// order that has nothing to do with the input's.
//
//   arena   the records, block_size first, back to back in the order they were added
//   items   per record: key | offset in the arena | size, written by recstore_append_kernel behind the kernel that wrote the
//           records.  The key is bam_resort.hpp's, (refID as u32) << 32 | (pos + 1 as
//           u32), read from the record's own bytes: refID -1 sorts last
//   sort    bam_resort.hpp's stable LSD radix sort (histogram, scan and scatter kernels as they stand) over the items' keys
//           and numbers, then its cut (W all ones: everything leaves) and offsets kernels: msrc / msize / dst are the
//           records' places in the arena, their sizes and their offsets in final order
//   drain   records [j0, j1) of the final order, cut on the host from dst (host/recstore_host.hpp), gathered into staging
//           bytes — the compressor's input — with their offsets from the drain's first byte, the index stage's `at`
//
// The host hands out every call's byte range and item range (fadehip_bam.hip), in call order and before anything of the call
// is launched: no kernel here reserves anything, and the order of the items does not depend on which stream runs first.
// All kernels here are new; a run without a store launches none of them.
#pragma once
#include "bam_device.hpp"
#include "bam_resort.hpp"

namespace fadehip {
namespace bam {

struct RecStoreRef {
    uint8_t *arena;
    uint64_t *key, *off;  // [items]
    uint32_t *size;       // [items]
};

// What a call appended: n slots, each of which built one record, two (the two sides of one read, one behind the other) or
// none.  Slot i's x_size[i] bytes lie at arena + base + blk_base[i / TAG_BLOCK] + the sizes of the block's slots in front —
// where bam_extract_write_kernel and bam_tags_extract_write_kernel put them, and where fadehip_recstore_add_batch copies the
// caller's.  The slots' records become items item0 .. item0 + n_items - 1, compacted, in slot order; the host has counted
// them before (n_items), and an item beyond that count is never written.
struct RecAppendArgs {
    RecStoreRef s;
    uint64_t base, item0;
    uint32_t n, n_items;
    const uint32_t *x_size;    // [n]
    const uint64_t *blk_base;  // [blocks of TAG_BLOCK slots]
    uint32_t *cnt_sums, *cnt_base;  // [blocks] items of a block, and of the blocks in front
};

// a slot's place in the arena and the records it holds: the first record's block_size says whether a second one follows
__device__ __forceinline__ uint32_t recstore_slot(const RecAppendArgs &a, uint32_t i, uint64_t *at) {
    const uint64_t sz = i < a.n ? (uint64_t)a.x_size[i] : 0ull;
    uint64_t tot;
    *at = a.base + a.blk_base[blockIdx.x] + block_scan_256(sz, &tot);
    if (sz < 36u) return 0u;
    return (uint64_t)ld32(a.s.arena + *at) + 4u < sz ? 2u : 1u;
}

// thread per slot, behind the kernel that wrote the records: the items of every block
__global__ __launch_bounds__(TAG_BLOCK) void recstore_count_kernel(RecAppendArgs a) {
    uint64_t at;
    const uint32_t c = recstore_slot(a, blockIdx.x * TAG_BLOCK + threadIdx.x, &at);
    __syncthreads();
    const uint64_t t = block_sum_256(c);
    if (threadIdx.x == 0) a.cnt_sums[blockIdx.x] = (uint32_t)t;
}

__global__ __launch_bounds__(1024) void recstore_count_scan_kernel(RecAppendArgs a, uint32_t n_blocks) {
    scan_block_sums<uint32_t, false>(a.cnt_sums, a.cnt_base, n_blocks, (uint32_t *)nullptr);
}

// Thread per slot: key (from the record as it lies in the arena), offset and size of the one or two items it built.
__global__ __launch_bounds__(TAG_BLOCK) void recstore_append_kernel(RecAppendArgs a) {
    uint64_t at, tot;
    const uint32_t c = recstore_slot(a, blockIdx.x * TAG_BLOCK + threadIdx.x, &at);
    __syncthreads();
    uint32_t k = a.cnt_base[blockIdx.x] + (uint32_t)block_scan_256(c, &tot);
    const uint64_t end = at + (c ? a.x_size[blockIdx.x * TAG_BLOCK + threadIdx.x] : 0u);
    for (uint32_t q = 0; q < c && k < a.n_items; q++, k++) {
        const uint8_t *p = a.s.arena + at;
        const uint32_t sz = q + 1u == c ? (uint32_t)(end - at) : ld32(p) + 4u;  // (the slot's last record ends where the slot does)
        a.s.key[a.item0 + k] = rs_key(ld32s(p + 4), ld32s(p + 8));
        a.s.off[a.item0 + k] = at;
        a.s.size[a.item0 + k] = sz;
        at += sz;
    }
}

// In front of the sort (a.key0, a.isrc and a.isize are the store's own arrays): the item numbers, and the ctl the resort
// kernels read — n items, none held over, W all ones so that the cut lets everything leave.
__global__ __launch_bounds__(256) void recstore_sort_begin_kernel(ResortArgs a, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        a.ctl->W = ~0ull;
        a.ctl->emit_bytes = 0;
        a.ctl->total_bytes = 0;
        a.ctl->bad = 0;
        a.ctl->n_in = n;
        a.ctl->n_emit = 0;
        a.ctl->n_held_in = 0;
        a.ctl->pad = 0;
    }
    if (i < n) a.idx0[i] = i;
}

struct RecGatherArgs {
    const uint8_t *arena;
    const uint64_t *msrc, *dst;  // in final order: where a record lies in the arena; [n_all + 1] offsets in final order
    const uint32_t *msize;
    uint32_t j0, n;              // the drain: records j0 .. j0 + n - 1 of the final order
    uint8_t *out;                // the staging bytes
    uint64_t *at;                // [n + 1] the records' offsets in them, at[n] behind the last
};

// The drain's records from the arena into the staging bytes: sixteen lanes per record, (unaligned) dwords as
// bam_resort_move_kernel.
__global__ __launch_bounds__(256) void recstore_gather_kernel(RecGatherArgs a) {
    const uint32_t j = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
    if (j >= a.n) return;
    const uint64_t d0 = a.dst[a.j0], d = a.dst[a.j0 + j] - d0;
    copy16(a.out + d, a.arena + a.msrc[a.j0 + j], a.msize[a.j0 + j], sl);
    if (sl == 0u) {
        a.at[j] = d;
        if (j + 1u == a.n) a.at[a.n] = a.dst[a.j0 + a.n] - d0;
    }
}

}  // namespace bam
}  // namespace fadehip
