// csi_build.hpp — the host's part of --write-index --csi: the calls' index entries (fadehip_index_call, as
// the device stage of bam_index.hpp leaves them under a geometry) become the payload of one .csi (CSI version 1).  Plain C++,
// no device: the library wraps it as fadehip_csi_*, host/selftest/csi_selftest.cpp holds it to tests/csi_model.py.
//
//   add     host/index_accum.hpp's, shared with host/bai_build.hpp
//   finish  same-block merge of a bin's chunks; per bin its loffset — a CSI file has no linear index, so the linear entries
//           are back-filled here, as a .bai's are, and a bin takes the value at its first window (0 when that window lies
//           behind the last one with a value); the pseudo-bin behind the bins; n_no_coor.  The payload is uncompressed: the
//           writer puts it into BGZF members
#pragma once
#include "index_accum.hpp"

namespace fadehip {
namespace csi {

using index_accum::Chunk;
using index_accum::NONE;
using index_accum::Ref;

inline bool valid_geometry(int32_t min_shift, int32_t depth) { return min_shift >= 4 && depth >= 1 && depth <= 8 && min_shift + 3 * depth <= 32; }
// level l begins at bin (8^l - 1) / 7; the bins of levels 0 .. depth are numbered below first_bin(depth + 1)
inline uint32_t first_bin(int32_t level) { return (uint32_t)(((1ull << (3 * level)) - 1) / 7); }
inline uint32_t pseudo_bin(int32_t depth) { return first_bin(depth + 1) + 1u; }

struct Builder : index_accum::Accum {
    int32_t min_shift, depth;

    // (a geometry that is not valid is the caller's to refuse: fadehip_csi_create does)
    Builder(int32_t n_ref, int32_t ms, int32_t d) : Accum("csi", n_ref, first_bin(d + 1) - 1u, 1ull << (3 * d)), min_shift(ms), depth(d) {}

    // the first window of bin b: the k-th bin of level l begins at window k << 3 (depth - l)
    uint64_t first_window(uint32_t b) const {
        int32_t level = depth;
        while (b < first_bin(level)) level--;
        return (uint64_t)(b - first_bin(level)) << (3 * (depth - level));
    }

    int finish(const uint8_t **out, size_t *n) {
        if (!out || !n) return fail("NULL argument");
        bytes.clear();
        put("CSI\1", 4);
        put32((uint32_t)min_shift);
        put32((uint32_t)depth);
        put32(0);  // l_aux
        put32((uint32_t)refs.size());
        std::vector<Chunk> merged;
        std::vector<uint64_t> filled;
        for (const Ref &r : refs) {
            if (!r.any) {
                put32(0);
                continue;
            }
            filled.resize(r.lin.size());
            uint64_t next = 0;
            for (size_t w = r.lin.size(); w-- > 0;) {
                if (r.lin[w] != NONE) next = r.lin[w];
                filled[w] = next;
            }
            put32((uint32_t)r.bins.size() + 1u);
            for (const auto &kv : r.bins) {
                merge(kv.second, merged);
                const uint64_t w = first_window(kv.first);
                put32(kv.first);
                put64(w < filled.size() ? filled[w] : 0);
                put32((uint32_t)merged.size());
                for (const Chunk &c : merged) {
                    put64(c.beg);
                    put64(c.end);
                }
            }
            put32(pseudo_bin(depth));
            put64(0);
            put32(2);
            put64(r.off_beg);
            put64(r.off_end);
            put64(r.n_mapped);
            put64(r.n_unmapped);
        }
        put64(n_no_coor);
        *out = bytes.data();
        *n = bytes.size();
        return 0;
    }
};

}  // namespace csi
}  // namespace fadehip
