// bam_mates.hpp — a map from (read name, segment) to where that record ends up once `fade out -c` has clipped it:
// fadehip_mateset_*, fadehip_mates_fix_batch, FADEHIP_BAM_COLLECT_MATES / FADEHIP_BAM_FIX_MATES (`fade out -c --fix-mates`).
// One pass stores the placement of every primary paired-end record it is told to, a later one clips the records as `fade
// out -c` does and then sets each record's mate fields (next_refID, next_pos, tlen, flags 0x8 / 0x20 and the first MC:Z
// field) from the placement stored under its mate's key.  The rule is stated in tests/mates_model.py and in DESIGN.md §3.8k;
// the device is held to it byte for byte.
//
// The map has the shape of the name set (bam_names.hpp) and shares its table, hash, growth and error flag:
//
//   key     [l_read_name][name bytes][segment = flag & 0xC0], padded with zeros to whole dwords: at most 65 dwords
//   entry   the key, then the placement: MV_DWORDS fixed dwords — flags (kind, reverse, and the ambiguous bit a second insert
//           under the key sets), refID, pos, the 5' end (i64), the bytes of text — then the leaving CIGAR as SAM text, padded
//           to a dword
//   ctrl    NS_USED | NS_COUNT | NS_ERR as the name set's, then MS_AMBIG: entries that carry the ambiguous bit
//
// The host's bound on the arena bytes one record can add, taken before the launch:
//   key 4 * 65 + fixed 4 * MV_DWORDS + text 11 * (n_cigar_op + 2) + 3 of padding
// — an op's length has 28 bits, so at most nine digits and the op's letter (eleven is on the safe side), and a clip adds at
// most two H ops.  fadehip_mateset_add_batch sums it over the records that insert; the file path, which does not read the
// records on the host, takes 312 bytes per record (260 + 24 + 3 + 22, rounded up) and 3 bytes per record byte of the call
// (11 for each CIGAR op, of four bytes).  A kernel that finds the arena or the table full all the same raises the error
// flag, and the call fails.
#pragma once
#include "bam_names.hpp"

namespace fadehip {
namespace bam {

enum : int { MS_AMBIG = 3 };
enum : uint32_t { MV_KIND = 3u, MV_MAPPED = 0u, MV_UNMAPPED = 1u, MV_RESET = 2u, MV_REVERSE = 4u, MV_AMBIGUOUS = 0x80000000u };
enum : uint32_t { MV_FLAGS = 0, MV_TID = 1, MV_POS = 2, MV_FIVE = 3, MV_TEXT_LEN = 5, MV_DWORDS = 6 };
constexpr uint32_t MATE_KEY_BYTES_MAX = 4u * 65u;

// what the plan kernel leaves the write kernel of one record
struct MateFix {
    uint32_t state;          // fixed[]: 0 untouched, 1 fixed, 2 the mate's key is ambiguous
    uint32_t flag;           // state 1: the flag as it leaves
    int32_t next_tid, next_pos, tlen;
    uint32_t mc_at, mc_old;  // the first MC:Z field: where its tag starts (relative to the record), its bytes; mc_old 0: none
    uint32_t mc_new;         // bytes of the field that takes its place, 0: it goes
    uint64_t text;           // where the new value lies in the arena
};

struct MateArgs {
    NameSetRef s;
    const uint8_t *u;
    const uint32_t *off32;            // the file path: rec_off ...
    const uint64_t *off64;            // ... the batch calls: in_off (the one that is not null)
    uint32_t n;                       // records (the file path: at most; counts_in says how many there are)
    const ChunkCounts *counts_in;     // the file path: n_records; nullptr: n
    const uint8_t *rs;                // [n]
    const uint32_t *trim_l, *trim_r;  // [n] reference bases
    const uint8_t *pick;              // insert: [n] or nullptr (every primary paired-end record)
    // the plan kernel of the file path: what the decision goes into (bam_eject_named_kernel's arrays)
    const uint32_t *info;
    uint64_t *blk_sums;
    unsigned long long *n_mates;      // records fixed | records whose mate's key is ambiguous << 32
    MateFix *fix;                     // [n]
    uint32_t *out_size;               // [n]
    const uint64_t *out_off;          // [n]
    uint8_t *out;
};

__device__ __forceinline__ const uint8_t *mate_rec(const MateArgs &a, uint32_t i) { return a.u + (a.off32 ? (uint64_t)a.off32[i] : a.off64[i]); }
__device__ __forceinline__ uint32_t mate_count(const MateArgs &a) { return a.counts_in ? min(a.n, a.counts_in->n_records) : a.n; }
__device__ __forceinline__ bool paired_end(uint32_t flag) { return (flag & 1u) && ((flag & 0xC0u) == 0x40u || (flag & 0xC0u) == 0x80u); }

// dword j of a record's key: name_dword's dwords over the 1 + l_read_name bytes Ln, the segment byte behind them
__device__ __forceinline__ uint32_t mate_key_dword(const uint8_t *p, uint32_t j, uint32_t Ln, uint32_t seg) {
    uint32_t x = 4u * j < Ln ? name_dword(p, j, Ln) : 0u;
    if ((Ln >> 2) == j) x |= seg << (8u * (Ln & 3u));
    return x;
}
__device__ __forceinline__ uint32_t mate_key_dwords(uint32_t Ln) { return (Ln + 4u) >> 2; }

template <bool PAST_L1>
__device__ __forceinline__ bool mate_key_is(const uint8_t *p, uint32_t Ln, uint32_t seg, const uint32_t *e) {
    const uint32_t kd = mate_key_dwords(Ln);
    for (uint32_t j = 0; j < kd; j++) {
        const uint32_t x = PAST_L1 ? __hip_atomic_load(e + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : e[j];
        if (x != mate_key_dword(p, j, Ln, seg)) return false;
    }
    return true;
}

// The placement of a record as it leaves under plan c: kind and reverse, refID, pos, the 5' end, the bytes its CIGAR takes
// as SAM text.  A reset record has a kind and nothing else.
struct Placement {
    uint32_t flags;
    int32_t tid, pos;
    int64_t five;
    uint32_t ncig, text_len;
};
__device__ __forceinline__ uint32_t leaving_op(const RecHdr &r, const ClipPlan &c, uint32_t j) { return c.mode ? clip_op(r, c, j) : ld32(r.p + r.cig_off + 4u * j); }
__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
    uint32_t d = 1;
    for (uint32_t t = 10u; d < 10u && v >= t; t *= 10u) d++;  // (t reaches 10^9 at d = 9 and is not multiplied again: v < 2^28)
    return d;
}
__device__ __forceinline__ Placement placement(const RecHdr &r, const ClipPlan &c) {
    Placement v;
    v.flags = MV_RESET;
    v.tid = v.pos = 0;
    v.five = 0;
    v.ncig = v.text_len = 0;
    if (c.mode == 2u) return v;
    v.ncig = c.mode ? c.ncig : r.ncig;
    uint64_t ref = 0;
    for (uint32_t j = 0; j < v.ncig; j++) {
        const uint32_t op = leaving_op(r, c, j);
        if (FADEHIP_OP_CONSUMES_REF(op & 15u)) ref += op >> 4;
        v.text_len += dec_digits(op >> 4) + 1u;
    }
    const bool reverse = (r.flag & 0x10u) != 0;
    v.flags = ((r.flag & 4u) ? MV_UNMAPPED : MV_MAPPED) | (reverse ? MV_REVERSE : 0u);
    v.tid = r.tid;
    v.pos = c.mode ? c.pos : r.pos;
    const int64_t end = (int64_t)v.pos + (int64_t)(ref ? ref : 1ull);
    v.five = reverse ? end - 1 : (int64_t)v.pos;
    return v;
}
// the leaving CIGAR as SAM text, v.text_len bytes
__device__ __forceinline__ void leaving_text(const RecHdr &r, const ClipPlan &c, const Placement &v, uint8_t *t) {
    for (uint32_t j = 0; j < v.ncig; j++) {
        const uint32_t op = leaving_op(r, c, j), nd = dec_digits(op >> 4);
        uint32_t len = op >> 4;
        for (uint32_t k = nd; k-- > 0u; len /= 10u) t[k] = (uint8_t)('0' + len % 10u);
        t[nd] = (uint8_t)"MIDNSHP=XB??????"[op & 15u];
        t += nd + 1u;
    }
}

// Thread per record; a picked primary paired-end record inserts its placement under its key.  bam_names_insert_kernel's
// protocol, step for step:
//   1  arena bytes are reserved with one atomic per wave: a prefix over the wave's sizes, the total added by one lane
//   2  the entry is written whole — key and placement, 3 __threadfence(), 4 it is published with a 64-bit atomicCAS
//   5  a thread that loses the CAS, or finds a used slot, compares keys past L1 (agent-scope atomic loads, see name_is):
//      unequal probes on; equal sets the ambiguous bit in the entry's flag dword with one atomicOr — whatever the two
//      placements are and whichever came first, so the outcome does not depend on the order of the threads — and its
//      reserved bytes stay dead.  The thread whose atomicOr set the bit counts the entry into ctrl[MS_AMBIG].
__global__ __launch_bounds__(TAG_BLOCK) void bam_mates_insert_kernel(MateArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    RecHdr r;
    ClipPlan c;
    Placement v;
    uint32_t Ln = 0, kd = 0, sz = 0;
    if (i < mate_count(a) && (!a.pick || a.pick[i])) {
        r = rec_header(mate_rec(a, i));
        if (paired_end(r.flag) && !(r.flag & 0x900u)) {
            c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
            v = placement(r, c);
            Ln = 1u + r.lname;
            kd = mate_key_dwords(Ln);
            sz = 4u * (kd + MV_DWORDS) + ((v.text_len + 3u) & ~3u);
        }
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
            const uint32_t seg = r.flag & 0xC0u;
            uint32_t *e = reinterpret_cast<uint32_t *>(a.s.arena + off);
            uint64_t h = NS_HASH_SEED;
            for (uint32_t j = 0; j < kd; j++) {
                const uint32_t x = mate_key_dword(r.p, j, Ln, seg);
                e[j] = x;
                h = name_hash_step(h, x);
            }
            h = name_hash_end(h, a.s.hash_bits);
            uint32_t *ev = e + kd;
            ev[MV_FLAGS] = v.flags;
            ev[MV_TID] = (uint32_t)v.tid;
            ev[MV_POS] = (uint32_t)v.pos;
            ev[MV_FIVE] = (uint32_t)(uint64_t)v.five;
            ev[MV_FIVE + 1] = (uint32_t)((uint64_t)v.five >> 32);
            ev[MV_TEXT_LEN] = v.text_len;
            leaving_text(r, c, v, reinterpret_cast<uint8_t *>(ev + MV_DWORDS));
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
                if ((cur >> 40) != tag) continue;
                uint32_t *o = reinterpret_cast<uint32_t *>(a.s.arena + ((cur & NS_OFF_MASK) - 1ull));
                if (!mate_key_is<true>(r.p, Ln, seg, o)) continue;
                if (!(atomicOr(o + kd + MV_FLAGS, MV_AMBIGUOUS) & MV_AMBIGUOUS)) atomicAdd(&a.s.ctrl[MS_AMBIG], 1ull);
                break;
            }
            if (probes > a.s.mask) atomicOr(&a.s.ctrl[NS_ERR], NS_ERR_TABLE);
        }
    }
    const unsigned long long w = __ballot(won);
    if (w && lane == (int)__builtin_ctzll(w)) atomicAdd(&a.s.ctrl[NS_COUNT], (unsigned long long)__builtin_popcountll(w));
}

// The placement stored under (the record's name, seg), or nullptr.  A later launch than any insert: plain loads (name_find).
__device__ __forceinline__ const uint32_t *mate_find(const NameSetRef &s, const uint8_t *p, uint32_t seg) {
    const uint32_t Ln = 1u + p[12], kd = mate_key_dwords(Ln);
    uint64_t h = NS_HASH_SEED;
    for (uint32_t j = 0; j < kd; j++) h = name_hash_step(h, mate_key_dword(p, j, Ln, seg));
    h = name_hash_end(h, s.hash_bits);
    const uint64_t tag = h >> 40;
    uint64_t idx = h & s.mask;
    for (uint64_t probes = 0; probes <= s.mask; probes++, idx = (idx + 1ull) & s.mask) {
        const unsigned long long cur = s.table[idx];
        if (!cur) return nullptr;
        if ((cur >> 40) != tag) continue;
        const uint32_t *e = reinterpret_cast<const uint32_t *>(s.arena + ((cur & NS_OFF_MASK) - 1ull));
        if (mate_key_is<false>(p, Ln, seg, e)) return e + kd;
    }
    atomicOr(&s.ctrl[NS_ERR], NS_ERR_TABLE);
    return nullptr;
}

// The rule for one record that leaves under plan c: what the write needs into f, the record's bytes as it leaves returned.
__device__ __forceinline__ uint32_t mate_plan(const NameSetRef &s, const RecHdr &r, const ClipPlan &c, MateFix &f) {
    const uint32_t size = c.mode == 2u ? c.pre : c.mode == 1u ? c.pre + (r.end - r.aux_off) : r.end;
    f = MateFix{};
    if (c.mode == 2u || !paired_end(r.flag)) return size;  // (a reset record leaves with flag 0)
    const uint32_t *v = mate_find(s, r.p, (r.flag & 0xC0u) ^ 0xC0u);
    if (!v) return size;
    if (v[MV_FLAGS] & MV_AMBIGUOUS) {
        f.state = 2;
        return size;
    }
    f.state = 1;
    const Placement own = placement(r, c);
    const uint32_t kind = v[MV_FLAGS] & MV_KIND;
    uint32_t text_len = 0;
    if (kind == MV_RESET) {
        f.flag = (r.flag | 0x8u) & ~0x22u;
        f.next_tid = own.tid;
        f.next_pos = own.pos;
        f.tlen = 0;
    } else {
        f.flag = (r.flag & ~0x28u) | ((v[MV_FLAGS] & MV_REVERSE) ? 0x20u : 0u) | (kind == MV_UNMAPPED ? 0x8u : 0u);
        f.next_tid = (int32_t)v[MV_TID];
        f.next_pos = (int32_t)v[MV_POS];
        f.tlen = 0;
        if (!(r.flag & 4u) && kind == MV_MAPPED && own.tid >= 0 && f.next_tid == own.tid) {
            const int64_t d = (int64_t)((uint64_t)v[MV_FIVE] | ((uint64_t)v[MV_FIVE + 1] << 32)) - own.five;
            f.tlen = (int32_t)(d >= 0 ? d + 1 : d - 1);
        }
        if (kind == MV_MAPPED) text_len = v[MV_TEXT_LEN];
    }
    // the first aux field MC of type Z: the walk ends at a field that is not whole
    for (uint32_t q = r.aux_off; q + 3u <= r.end;) {
        const uint32_t fs = aux_field_size(r.p, q + 2u, r.end);
        if (!fs) break;
        if (r.p[q] == 'M' && r.p[q + 1u] == 'C' && r.p[q + 2u] == 'Z') {
            f.mc_at = q;
            f.mc_old = 2u + fs;
            f.mc_new = text_len ? 4u + text_len : 0u;
            f.text = (uint64_t)(reinterpret_cast<const uint8_t *>(v + MV_DWORDS) - s.arena);
            break;
        }
        q += 2u + fs;
    }
    return size - f.mc_old + f.mc_new;
}

// The record as it leaves, by its sixteen lanes: the head as clip_batch_write_kernel writes it, the fixed fields of a fixed
// record patched by the lanes that wrote their dwords (lane k writes dword k of the head on either path, a head has at
// least 37 bytes), the aux bytes in up to three pieces — in front of MC, the new MC, behind it.
__device__ __forceinline__ void mate_write(const NameSetRef &s, const RecHdr &r, const ClipPlan &c, const MateFix &f, uint32_t out_size, uint8_t *dst, uint32_t sl) {
    const uint32_t pre = c.mode ? c.pre : r.aux_off;
    if (c.mode) clip_write_head(r, c, dst, out_size - 4u, sl);
    else copy16(dst, r.p, r.aux_off, sl);
    if (c.mode == 2u) return;
    if (f.state == 1u) {
        u32u *d = reinterpret_cast<u32u *>(dst);
        if (sl == 0u) d[0] = out_size - 4u;
        if (sl == 4u) d[4] = ((c.mode ? c.ncig : r.ncig) & 0xffffu) | (f.flag << 16);
        if (sl == 6u) d[6] = (uint32_t)f.next_tid;
        if (sl == 7u) d[7] = (uint32_t)f.next_pos;
        if (sl == 8u) d[8] = (uint32_t)f.tlen;
    }
    if (f.state != 1u || !f.mc_old) {
        copy16(dst + pre, r.p + r.aux_off, r.end - r.aux_off, sl);
        return;
    }
    const uint32_t before = f.mc_at - r.aux_off, behind = f.mc_at + f.mc_old;
    copy16(dst + pre, r.p + r.aux_off, before, sl);
    uint8_t *m = dst + pre + before;
    const uint8_t *text = s.arena + f.text;
    for (uint32_t q = sl; q < f.mc_new; q += 16u) m[q] = q == 0u ? 'M' : q == 1u ? 'C' : q == 2u ? 'Z' : q + 1u == f.mc_new ? 0 : text[q - 3u];
    copy16(m + f.mc_new, r.p + behind, r.end - behind, sl);
}

// FADEHIP_BAM_FIX_MATES, thread per record behind the stage kernel and in front of bam_tag_scan_kernel: the rule's plan for
// every record that leaves, its out_size corrected by what MC gains or loses, the block's bytes summed again (as
// bam_eject_named_kernel does), the records fixed and the ones with an ambiguous mate counted into the call's counts
__global__ __launch_bounds__(TAG_BLOCK) void bam_mates_plan_kernel(MateArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    uint64_t sz = 0;  // bytes, the fixed records above bit 40, the ambiguous ones above bit 52
    if (i < mate_count(a)) {
        MateFix f = MateFix{};
        uint32_t out = a.out_size[i];
        if (!(a.info[i] & INFO_BAD)) {
            const RecHdr r = rec_header(mate_rec(a, i));
            const ClipPlan c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
            out = mate_plan(a.s, r, c, f);
            a.out_size[i] = out;
        }
        a.fix[i] = f;
        sz = (uint64_t)out | (f.state == 1u ? 1ull << 40 : 0ull) | (f.state == 2u ? 1ull << 52 : 0ull);
    }
    const uint64_t t = block_sum_256(sz);
    if (threadIdx.x == 0) {
        a.blk_sums[blockIdx.x] = t & ((1ull << 40) - 1ull);
        const unsigned long long fixed = (t >> 40) & 0xfffull, ambiguous = t >> 52;
        if (fixed | ambiguous) atomicAdd(a.n_mates, fixed | (ambiguous << 32));
    }
}

// ---- fadehip_mates_fix_batch: thread per record, then sixteen lanes per record (clip_batch_size_kernel / _write_kernel)
__global__ __launch_bounds__(256) void mates_batch_plan_kernel(MateArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const RecHdr r = rec_header(mate_rec(a, i));
    const ClipPlan c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
    MateFix f;
    a.out_size[i] = mate_plan(a.s, r, c, f);
    a.fix[i] = f;
}
__global__ __launch_bounds__(256) void mates_batch_write_kernel(MateArgs a) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
    if (i >= a.n) return;
    const RecHdr r = rec_header(mate_rec(a, i));
    const ClipPlan c = clip_plan(r, a.rs[i], a.trim_l[i], a.trim_r[i]);
    mate_write(a.s, r, c, a.fix[i], a.out_size[i], a.out + a.out_off[i], sl);
}

}  // namespace bam
}  // namespace fadehip
