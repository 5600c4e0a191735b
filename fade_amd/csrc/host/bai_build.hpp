// bai_build.hpp — the host's part of --write-index: the calls' index entries (fadehip_index_call, as the
// device stage of bam_index.hpp leaves them) become one .bai (SAM specification §5.2).  Plain C++, no device: the library
// wraps it as fadehip_bai_*, host/selftest/bai_selftest.cpp holds it to the hand cases of tests/bai_model.py.
//
//   add     rebases the call's virtual offsets by the file offset of its first member and appends per reference: chunks in
//           file order per bin, linear entries first writer wins, the reference runs' bounds and counts
//   finish  same-block merge of a bin's chunks, back-fill of the windows without an entry, pseudo-bin 37450, n_no_coor
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../../include/fadehip.h"

namespace fadehip {
namespace bai {

constexpr uint32_t PSEUDO_BIN = 37450, MAX_BIN = 37449, MAX_WINDOWS = 1u << 15;

struct Chunk { uint64_t beg, end; };
struct Ref {
    std::map<uint32_t, std::vector<Chunk>> bins;
    std::vector<uint64_t> lin;   // per window: the offset, or NONE
    bool any = false;
    uint64_t off_beg = 0, off_end = 0, n_mapped = 0, n_unmapped = 0;
};
constexpr uint64_t NONE = ~0ull;

struct Builder {
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0, last_key = 0;
    int64_t n_records = 0;
    bool have_key = false;
    std::vector<uint8_t> bytes;
    std::string err;

    explicit Builder(int32_t n_ref) : refs((size_t)(n_ref > 0 ? n_ref : 0)) {}

    int fail(const char *fmt, long long a = 0, long long b = 0) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, a, b);
        err = buf;
        return FADEHIP_E_INVALID;
    }

    // What of a call could not be appended is found before anything is: a failed add leaves the builder as it was.
    int add(uint64_t base, const fadehip_index_call *c) {
        if (!c) return fail("bai: call is NULL");
        if (c->n_chunks < 0 || c->n_linear < 0 || c->n_refs < 0 || c->n_records < 0) return fail("bai: negative count");
        if ((c->n_chunks && !c->chunks) || (c->n_linear && !c->linear) || (c->n_refs && !c->refs)) return fail("bai: NULL array");
        if (base >> 48) return fail("bai: file offset beyond 2^48");
        const int64_t n_ref = (int64_t)refs.size();
        for (int64_t k = 0; k < c->n_chunks; k++)
            if (c->chunks[k].tid < 0 || c->chunks[k].tid >= n_ref || c->chunks[k].bin > MAX_BIN)
                return fail("bai: chunk %lld names reference or bin out of range", (long long)k);
        for (int64_t k = 0; k < c->n_linear; k++)
            if (c->linear[k].tid < 0 || c->linear[k].tid >= n_ref || c->linear[k].window >= MAX_WINDOWS)
                return fail("bai: linear entry %lld names reference or window out of range", (long long)k);
        for (int64_t k = 0; k < c->n_refs; k++)
            if (c->refs[k].tid < -1 || c->refs[k].tid >= n_ref) return fail("bai: reference run %lld names reference %lld", (long long)k, (long long)c->refs[k].tid);
        if (c->n_records && have_key && c->first_key < last_key)
            return fail("bam stream: record %lld: not in coordinate order (--write-index needs coordinate-sorted output)", (long long)n_records);
        const uint64_t add16 = base << 16;
        for (int64_t k = 0; k < c->n_chunks; k++) {
            const fadehip_index_chunk &x = c->chunks[k];
            refs[(size_t)x.tid].bins[x.bin].push_back(Chunk{x.beg + add16, x.end + add16});
        }
        for (int64_t k = 0; k < c->n_linear; k++) {
            const fadehip_index_linear &x = c->linear[k];
            std::vector<uint64_t> &lin = refs[(size_t)x.tid].lin;
            if (lin.size() <= x.window) lin.resize((size_t)x.window + 1, NONE);
            if (lin[x.window] == NONE) lin[x.window] = x.off + add16;
        }
        for (int64_t k = 0; k < c->n_refs; k++) {
            const fadehip_index_ref &x = c->refs[k];
            if (x.tid < 0) {
                n_no_coor += x.n_mapped + x.n_unmapped;
                continue;
            }
            Ref &r = refs[(size_t)x.tid];
            if (!r.any) r.off_beg = x.off_beg + add16;
            r.any = true;
            r.off_end = x.off_end + add16;
            r.n_mapped += x.n_mapped;
            r.n_unmapped += x.n_unmapped;
        }
        if (c->n_records) {
            last_key = c->last_key;
            have_key = true;
        }
        n_records += c->n_records;
        return 0;
    }

    void put(const void *p, size_t n) { bytes.insert(bytes.end(), (const uint8_t *)p, (const uint8_t *)p + n); }
    void put32(uint32_t v) { put(&v, 4); }
    void put64(uint64_t v) { put(&v, 8); }

    int finish(const uint8_t **out, size_t *n) {
        if (!out || !n) return fail("bai: NULL argument");
        bytes.clear();
        put("BAI\1", 4);
        put32((uint32_t)refs.size());
        std::vector<Chunk> merged;
        for (const Ref &r : refs) {
            if (!r.any) {
                put32(0);
                put32(0);
                continue;
            }
            put32((uint32_t)r.bins.size() + 1u);
            for (const auto &kv : r.bins) {
                merged.clear();
                for (const Chunk &c : kv.second) {
                    if (!merged.empty() && (merged.back().end >> 16) >= (c.beg >> 16)) merged.back().end = c.end;
                    else merged.push_back(c);
                }
                put32(kv.first);
                put32((uint32_t)merged.size());
                for (const Chunk &c : merged) {
                    put64(c.beg);
                    put64(c.end);
                }
            }
            put32(PSEUDO_BIN);
            put32(2);
            put64(r.off_beg);
            put64(r.off_end);
            put64(r.n_mapped);
            put64(r.n_unmapped);
            put32((uint32_t)r.lin.size());  // (the last window always has an entry: resize follows one)
            const size_t at = bytes.size();
            bytes.resize(at + 8 * r.lin.size());
            uint64_t next = 0;
            for (size_t w = r.lin.size(); w-- > 0;) {
                if (r.lin[w] != NONE) next = r.lin[w];
                memcpy(&bytes[at + 8 * w], &next, 8);
            }
        }
        put64(n_no_coor);
        *out = bytes.data();
        *n = bytes.size();
        return 0;
    }
};

}  // namespace bai
}  // namespace fadehip
