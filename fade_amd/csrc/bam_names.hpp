// bam_names.hpp — a set of read names resident in HBM: fadehip_nameset_*, FADEHIP_BAM_COLLECT_NAMES and
// FADEHIP_BAM_EJECT_NAMED (`fade out --fragments`).  One pass over an annotated file adds the names of its artifact calls, a
// second writes every record whose name is not in the set — whole fragments leave, whatever the order of the input.
//
// The set is exact.  Two names are equal when l_read_name and every name byte are (same_name's rule); the hash decides where
// to look, never whether two names are equal, and two different names with one hash are two entries.
//
//   arena   entries of [l_read_name][name bytes], each starting at a multiple of four and padded with zeros to one: the
//           insert kernel compares through agent-scope atomic loads (see there), which want naturally aligned dwords — so an
//           entry is whole dwords, needs no slack behind it, and takes at most 256 bytes (never more than its record)
//   table   a power of two of 64-bit slots, 0: empty, else (tag << 40) | (1 + the entry's arena offset), tag the hash's top
//           24 bits; linear probing; the host keeps the load at or below 1/2 after any add
//   ctrl    arena bytes handed out | distinct names | error flag (NS_ERR_*), three u64
//
// The host sizes table and arena from bounds it has before a launch (new names <= the call's records, new bytes <= min(256
// x records, the call's record bytes)), and grows them — rehash kernel, arena moved — only while nothing else of the set
// runs.  A kernel that finds the table or the arena full all the same raises the error flag, and the call fails.
#pragma once
#include "bam_device.hpp"

namespace fadehip {
namespace bam {

enum : int { NS_USED = 0, NS_COUNT = 1, NS_ERR = 2 };
enum : unsigned long long { NS_ERR_ARENA = 1, NS_ERR_TABLE = 2 };
constexpr uint64_t NS_OFF_MASK = (1ull << 40) - 1ull;

struct NameSetRef {
    unsigned long long *table;
    uint64_t mask;             // slots - 1
    uint8_t *arena;
    uint64_t arena_cap;
    unsigned long long *ctrl;  // NS_USED, NS_COUNT, NS_ERR
    uint32_t hash_bits;        // FADEHIP_NAMESET_HASH_BITS: the hash is cut to its low bits before any use
};

struct NameArgs {
    NameSetRef s;
    const uint8_t *u;
    const uint32_t *off32;         // the file path: rec_off ...
    const uint64_t *off64;         // ... the batch calls: in_off (the one that is not null)
    uint32_t n;                    // records (the file path: at most; counts_in says how many there are)
    const ChunkCounts *counts_in;  // the file path: n_records; nullptr: n
    const uint8_t *pick;           // insert: record i adds its name when pick[i] & pick_mask; nullptr: every record
    uint32_t pick_mask;
    uint8_t *hit;                  // look-up: [n]
    // bam_eject_named_kernel: what the decision goes into (bam_eject_apply_kernel's arrays)
    uint32_t *out_size, *info;
    uint64_t *blk_sums;
    ChunkCounts *counts;           // n_ejected
};

struct NameRehashArgs {
    const unsigned long long *old_table;
    uint64_t old_slots;
    NameSetRef s;  // the new table
    uint32_t key_extra;  // key bytes behind the name: 0 for names, 1 for the mate map's segment byte (bam_mates.hpp)
};

__device__ __forceinline__ const uint8_t *name_rec(const NameArgs &a, uint32_t i) { return a.u + (a.off32 ? (uint64_t)a.off32[i] : a.off64[i]); }
__device__ __forceinline__ uint32_t name_count(const NameArgs &a) { return a.counts_in ? min(a.n, a.counts_in->n_records) : a.n; }

// dword j of a record's entry, L = 1 + l_read_name bytes long: the length byte, then the name, zeros behind it.  Unaligned
// dword loads as same_name's, the last one masked; they reach up to three bytes behind the name (bytes of the record when
// l_read_name fits block_size, which the callers have checked).
__device__ __forceinline__ uint32_t name_dword(const uint8_t *p, uint32_t j, uint32_t L) {
    uint32_t x = j ? ld32(p + 35u + 4u * j) : (ld32(p + 36u) << 8) | (L - 1u);
    if (4u * j + 4u > L) x &= 0xffffffffu >> (8u * (4u * j + 4u - L));
    return x;
}

__device__ __forceinline__ uint64_t name_hash_step(uint64_t h, uint32_t x) {
    h = (h ^ x) * 0x9e3779b97f4a7c15ull;
    return h ^ (h >> 29);
}
__device__ __forceinline__ uint64_t name_hash_end(uint64_t h, uint32_t bits) {
    h ^= h >> 32;
    h *= 0xd6e8feb86659fd93ull;
    h ^= h >> 32;
    return bits >= 64u ? h : bits == 0u ? 0ull : h & ((1ull << bits) - 1ull);
}
constexpr uint64_t NS_HASH_SEED = 0xcbf29ce484222325ull;
__device__ __forceinline__ uint64_t name_hash(const uint8_t *p, uint32_t L, uint32_t bits) {
    uint64_t h = NS_HASH_SEED;
    for (uint32_t j = 0; 4u * j < L; j++) h = name_hash_step(h, name_dword(p, j, L));
    return name_hash_end(h, bits);
}

// Is the entry at e the record's name?  PAST_L1: the entry may have been written by another CU during this launch, and the
// vector L1 is not coherent — a neighbouring entry of the same line may have been read before, so every dword is loaded
// past L1 (an agent-scope atomic load: L2-served).  The first dword holds the length: entries of another length end there.
template <bool PAST_L1>
__device__ __forceinline__ bool name_is(const uint8_t *p, uint32_t L, const uint32_t *e) {
    for (uint32_t j = 0; 4u * j < L; j++) {
        const uint32_t x = PAST_L1 ? __hip_atomic_load(e + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : e[j];
        if (x != name_dword(p, j, L)) return false;
    }
    return true;
}

// Thread per record; only picked records insert.
//   1  arena bytes are reserved with one atomic per wave: a prefix over the wave's sizes, the total added by one lane
//      (a wave without a picked record — seen by ballot — adds nothing)
//   2  the entry is written, 3 __threadfence(), 4 it is published with a 64-bit atomicCAS on an empty slot
//   5  a thread that loses the CAS, or finds a used slot, compares names (past L1, see name_is): equal is a duplicate — its
//      reserved bytes stay dead; unequal probes the next slot
// An entry is counted once, on the successful CAS, per wave.  A full arena or a probe that comes round raises the error flag.
__global__ __launch_bounds__(TAG_BLOCK) void bam_names_insert_kernel(NameArgs a) {
    const uint32_t n = name_count(a);
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint8_t *p = nullptr;
    uint32_t L = 0, sz = 0;
    if (i < n && (!a.pick || (a.pick[i] & a.pick_mask))) {
        p = name_rec(a, i);
        L = 1u + p[12];
        sz = (L + 3u) & ~3u;
    }
    if (!__ballot(sz != 0u)) return;  // (uniform)
    uint32_t inc = sz;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += o;
    }
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(&a.s.ctrl[NS_USED], (unsigned long long)inc);
    base = (unsigned long long)__shfl((long long)base, 63, 64);
    bool won = false;
    if (sz) {
        const uint64_t off = base + inc - sz;
        if (off + sz > a.s.arena_cap || off + sz > NS_OFF_MASK) {
            atomicOr(&a.s.ctrl[NS_ERR], NS_ERR_ARENA);
        } else {
            uint32_t *e = reinterpret_cast<uint32_t *>(a.s.arena + off);
            uint64_t h = NS_HASH_SEED;
            for (uint32_t j = 0; 4u * j < L; j++) {
                const uint32_t x = name_dword(p, j, L);
                e[j] = x;
                h = name_hash_step(h, x);
            }
            h = name_hash_end(h, a.s.hash_bits);
            __threadfence();
            const uint64_t tag = h >> 40, val = (tag << 40) | (off + 1ull);
            uint64_t idx = h & a.s.mask, probes = 0;
            for (; probes <= a.s.mask; probes++, idx = (idx + 1ull) & a.s.mask) {
                unsigned long long cur = __hip_atomic_load(&a.s.table[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!cur) {
                    cur = atomicCAS(&a.s.table[idx], 0ull, (unsigned long long)val);
                    if (!cur) {
                        won = true;
                        break;
                    }
                }
                if ((cur >> 40) == tag && name_is<true>(p, L, reinterpret_cast<const uint32_t *>(a.s.arena + ((cur & NS_OFF_MASK) - 1ull)))) break;
            }
            if (probes > a.s.mask) atomicOr(&a.s.ctrl[NS_ERR], NS_ERR_TABLE);
        }
    }
    const unsigned long long w = __ballot(won);
    if (w && lane == (int)__builtin_ctzll(w)) atomicAdd(&a.s.ctrl[NS_COUNT], (unsigned long long)__builtin_popcountll(w));
}

// Is the record's name in the set?  A later launch than any insert: plain loads.  The load of at most 1/2 leaves an empty
// slot on every probe sequence; a probe that comes round all the same raises the error flag.
__device__ __forceinline__ bool name_find(const NameSetRef &s, const uint8_t *p) {
    const uint32_t L = 1u + p[12];
    const uint64_t h = name_hash(p, L, s.hash_bits), tag = h >> 40;
    uint64_t idx = h & s.mask;
    for (uint64_t probes = 0; probes <= s.mask; probes++, idx = (idx + 1ull) & s.mask) {
        const unsigned long long cur = s.table[idx];
        if (!cur) return false;
        if ((cur >> 40) == tag && name_is<false>(p, L, reinterpret_cast<const uint32_t *>(s.arena + ((cur & NS_OFF_MASK) - 1ull)))) return true;
    }
    atomicOr(&s.ctrl[NS_ERR], NS_ERR_TABLE);
    return false;
}

// thread per record: hit[i] = 1 when the record's name is in the set
__global__ __launch_bounds__(TAG_BLOCK) void bam_names_lookup_kernel(NameArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (i >= name_count(a)) return;
    a.hit[i] = name_find(a.s, name_rec(a, i)) ? 1 : 0;
}

// FADEHIP_BAM_EJECT_NAMED, thread per record: the look-up, applied as bam_eject_apply_kernel applies its decision — a record
// whose name is in the set gets out_size 0 and INFO_BAD, and the block's bytes are summed again, in front of
// bam_tag_scan_kernel
__global__ __launch_bounds__(TAG_BLOCK) void bam_eject_named_kernel(NameArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;  // bytes, and the number of ejected records above bit 40
    if (i < name_count(a)) {
        if (name_find(a.s, name_rec(a, i))) {
            a.out_size[i] = 0u;
            a.info[i] |= INFO_BAD;
            sz = 1ull << 40;
        } else sz = a.out_size[i];
    }
    const uint64_t t = block_sum_256(sz);
    if (threadIdx.x == 0) {
        a.blk_sums[blockIdx.x] = t & ((1ull << 40) - 1ull);
        if (t >> 40) atomicAdd(&a.counts->n_ejected, (uint32_t)(t >> 40));
    }
}

// Thread per slot of the old table: a used slot hashes its key again from the arena and claims an empty slot of the new
// table (no duplicates can occur).  Runs alone: nothing else of the set is in flight (see fadehip_bam.hip).
__global__ __launch_bounds__(TAG_BLOCK) void bam_names_rehash_kernel(NameRehashArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (k >= a.old_slots) return;
    const unsigned long long cur = a.old_table[k];
    if (!cur) return;
    const uint32_t *e = reinterpret_cast<const uint32_t *>(a.s.arena + ((cur & NS_OFF_MASK) - 1ull));
    const uint32_t L = 1u + (e[0] & 0xffu) + a.key_extra;
    uint64_t h = NS_HASH_SEED;
    for (uint32_t j = 0; 4u * j < L; j++) h = name_hash_step(h, e[j]);
    h = name_hash_end(h, a.s.hash_bits);
    const unsigned long long val = ((h >> 40) << 40) | (cur & NS_OFF_MASK);
    uint64_t idx = h & a.s.mask;
    for (uint64_t probes = 0; probes <= a.s.mask; probes++, idx = (idx + 1ull) & a.s.mask)
        if (!atomicCAS(&a.s.table[idx], 0ull, val)) return;
    atomicOr(&a.s.ctrl[NS_ERR], NS_ERR_TABLE);
}

}  // namespace bam
}  // namespace fadehip
