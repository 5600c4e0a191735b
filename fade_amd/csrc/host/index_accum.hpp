// index_accum.hpp — what the two index builders of the host share (host/bai_build.hpp, host/csi_build.hpp; DESIGN.md §3.8j,
// §3.8p): the calls' index entries (fadehip_index_call, as the device stage of bam_index.hpp leaves them) appended per
// reference, the same-block merge of a bin's chunks, and the bytes a finish hands out.  Plain C++, no device.
//
//   add     rebases the call's virtual offsets by the file offset of its first member and appends per reference: chunks in
//           file order per bin, linear entries first writer wins, the reference runs' bounds and counts
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../../include/fadehip.h"

namespace fadehip {
namespace index_accum {

struct Chunk { uint64_t beg, end; };
struct Ref {
    std::map<uint32_t, std::vector<Chunk>> bins;
    std::vector<uint64_t> lin;   // per window: the offset, or NONE
    bool any = false;
    uint64_t off_beg = 0, off_end = 0, n_mapped = 0, n_unmapped = 0;
};
constexpr uint64_t NONE = ~0ull;

struct Accum {
    const char *what;            // "bai" or "csi": how the messages begin
    uint32_t max_bin;            // the largest bin number a chunk may name
    uint64_t max_windows;        // windows a reference has
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0, last_key = 0;
    int64_t n_records = 0;
    bool have_key = false;
    std::vector<uint8_t> bytes;
    std::string err;

    Accum(const char *w, int32_t n_ref, uint32_t mb, uint64_t mw) : what(w), max_bin(mb), max_windows(mw), refs((size_t)(n_ref > 0 ? n_ref : 0)) {}

    int fail(const char *fmt, long long a = 0, long long b = 0) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, a, b);
        err = std::string(what) + ": " + buf;
        return FADEHIP_E_INVALID;
    }

    // What of a call could not be appended is found before anything is: a failed add leaves the builder as it was.
    int add(uint64_t base, const fadehip_index_call *c) {
        if (!c) return fail("call is NULL");
        if (c->n_chunks < 0 || c->n_linear < 0 || c->n_refs < 0 || c->n_records < 0) return fail("negative count");
        if ((c->n_chunks && !c->chunks) || (c->n_linear && !c->linear) || (c->n_refs && !c->refs)) return fail("NULL array");
        if (base >> 48) return fail("file offset beyond 2^48");
        const int64_t n_ref = (int64_t)refs.size();
        for (int64_t k = 0; k < c->n_chunks; k++)
            if (c->chunks[k].tid < 0 || c->chunks[k].tid >= n_ref || c->chunks[k].bin > max_bin)
                return fail("chunk %lld names reference or bin out of range", (long long)k);
        for (int64_t k = 0; k < c->n_linear; k++)
            if (c->linear[k].tid < 0 || c->linear[k].tid >= n_ref || c->linear[k].window >= max_windows)
                return fail("linear entry %lld names reference or window out of range", (long long)k);
        for (int64_t k = 0; k < c->n_refs; k++)
            if (c->refs[k].tid < -1 || c->refs[k].tid >= n_ref) return fail("reference run %lld names reference %lld", (long long)k, (long long)c->refs[k].tid);
        if (c->n_records && have_key && c->first_key < last_key) {
            char buf[160];
            snprintf(buf, sizeof buf, "bam stream: record %lld: not in coordinate order (--write-index needs coordinate-sorted output)", (long long)n_records);
            err = buf;
            return FADEHIP_E_INVALID;
        }
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

    // a bin's chunks, in file order, with every chunk merged into the one before while it begins in the block that one ends in
    static void merge(const std::vector<Chunk> &in, std::vector<Chunk> &merged) {
        merged.clear();
        for (const Chunk &c : in) {
            if (!merged.empty() && (merged.back().end >> 16) >= (c.beg >> 16)) merged.back().end = c.end;
            else merged.push_back(c);
        }
    }
};

}  // namespace index_accum
}  // namespace fadehip
