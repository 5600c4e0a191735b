// recstore_host.hpp — the host-only parts of the sorted extract (tests/recstore_model.py states both rules
// in Python): where a drain of the record store ends, and the header text of a coordinate-sorted file.  No device, no
// library call: build/recstore_selftest runs both under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

namespace fadehip {
namespace recstore {

// dst[0 .. n]: the records' offsets in final order, dst[n] behind the last.  The drain that begins at record j0 < n ends in
// front of the returned record: the longest run whose bytes total at most max_payload, and one record when even that is more.
inline size_t drain_cut(const uint64_t *dst, size_t n, size_t j0, uint64_t max_payload) {
    const uint64_t lim = max_payload > UINT64_MAX - dst[j0] ? UINT64_MAX : dst[j0] + max_payload;
    const size_t j1 = (size_t)(std::upper_bound(dst + j0 + 1, dst + n + 1, lim) - dst) - 1;  // the last j with dst[j] <= lim
    return std::max(j1, j0 + 1);
}

// The header text with SO:coordinate on its @HD line: an SO: value is replaced, an @HD line without one gains the field at
// its end, and a text without an @HD line gets "@HD\tVN:1.6\tSO:coordinate" in front.  (@HD is the first line when present.)
inline std::string header_sorted(const std::string &text) {
    static const char so[] = "SO:coordinate";
    if (text.compare(0, 3, "@HD") != 0 || (text.size() > 3 && text[3] != '\t' && text[3] != '\n')) return std::string("@HD\tVN:1.6\t") + so + "\n" + text;
    size_t eol = text.find('\n');
    if (eol == std::string::npos) eol = text.size();
    std::string line = text.substr(0, eol), out;
    bool done = false;
    size_t at = 0;
    while (at <= line.size()) {
        size_t tab = line.find('\t', at);
        if (tab == std::string::npos) tab = line.size();
        const std::string f = line.substr(at, tab - at);
        if (at) out += '\t';
        if (f.compare(0, 3, "SO:") == 0) {
            if (!done) out += so;
            else out.pop_back();  // (a second SO: field goes, with its tab)
            done = true;
        } else out += f;
        at = tab + 1;
    }
    if (!done) out += std::string("\t") + so;
    return out + text.substr(eol);
}

}  // namespace recstore
}  // namespace fadehip
