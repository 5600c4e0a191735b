// bai_build.hpp — the host's part of --write-index: the calls' index entries (fadehip_index_call, as the
// device stage of bam_index.hpp leaves them) become one .bai (SAM specification §5.2).  Plain C++, no device: the library
// wraps it as fadehip_bai_*, host/selftest/bai_selftest.cpp holds it to the hand cases of tests/bai_model.py.
//
//   add     host/index_accum.hpp's, shared with host/csi_build.hpp: per reference, chunks in file order per bin, linear
//           entries first writer wins, the reference runs' bounds and counts
//   finish  same-block merge of a bin's chunks, back-fill of the windows without an entry, pseudo-bin 37450, n_no_coor
#pragma once
#include "index_accum.hpp"

namespace fadehip {
namespace bai {

constexpr uint32_t PSEUDO_BIN = 37450, MAX_BIN = 37449, MAX_WINDOWS = 1u << 15;

using index_accum::Chunk;
using index_accum::NONE;
using index_accum::Ref;

struct Builder : index_accum::Accum {
    explicit Builder(int32_t n_ref) : Accum("bai", n_ref, MAX_BIN, MAX_WINDOWS) {}

    int finish(const uint8_t **out, size_t *n) {
        if (!out || !n) return fail("NULL argument");
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
                merge(kv.second, merged);
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
