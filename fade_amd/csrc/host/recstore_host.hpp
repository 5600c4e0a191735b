// recstore_host.hpp — the host-only parts of the sorted extract (tests/recstore_model.py states both rules
// in Python): where a drain of the record store ends, and the header text of a coordinate-sorted file.  No device, no
// library call: build/recstore_selftest runs both under ASan + UBSan.  Behind them the buckets and windows of the sorted main
// output (§3.8n; tests/sorted_out_model.py), which build/sortwin_selftest runs the same way.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

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

// ---- the sorted main output's windows (tests/sorted_out_model.py states the rule in Python).  The key space
// — bam_resort.hpp's (refID as u32) << 32 | (pos + 1 as u32) — is cut into buckets of 2^SORTWIN_SHIFT positions: reference r
// has nb[r] = ((len[r] + 1) >> SHIFT) + 1 of them from first[r], and one more bucket, the last, takes refID -1 and every
// refID outside the header.  bucket() is monotone in the key and total: a pos beyond the contig falls into the contig's last.
constexpr uint32_t SORTWIN_SHIFT = 16;
constexpr uint64_t SORTWIN_ITEM_COST = 64;  // per record, beside its bytes: the item and sort arrays (57 bytes, §3.8l)

struct BucketLayout {
    std::vector<uint32_t> first, nb;  // [n_ref]
    uint32_t n_buckets = 1;
};

// false: more buckets than 32 bits number (no BAM header comes near it)
inline bool bucket_layout(const uint32_t *ref_len, size_t n_ref, BucketLayout &out) {
    out.first.assign(n_ref, 0);
    out.nb.assign(n_ref, 0);
    uint64_t at = 0;
    for (size_t r = 0; r < n_ref; r++) {
        out.first[r] = (uint32_t)at;
        out.nb[r] = (uint32_t)((((uint64_t)ref_len[r] + 1) >> SORTWIN_SHIFT) + 1);
        at += out.nb[r];
        if (at >= UINT32_MAX) return false;
    }
    out.n_buckets = (uint32_t)at + 1;
    return true;
}

inline uint32_t bucket_of(const BucketLayout &l, uint64_t key) {
    const uint64_t r = key >> 32;
    if (r >= l.nb.size()) return l.n_buckets - 1;
    return l.first[(size_t)r] + std::min((uint32_t)key >> SORTWIN_SHIFT, l.nb[(size_t)r] - 1);
}

// the keys of bucket b, both ends inclusive; *ref: its reference, -1 for the last bucket
inline void bucket_range(const BucketLayout &l, uint32_t b, uint64_t *lo, uint64_t *hi, int64_t *ref = nullptr) {
    if (b + 1 >= l.n_buckets) {
        *lo = (uint64_t)l.nb.size() << 32;
        *hi = ~(uint64_t)0;
        if (ref) *ref = -1;
        return;
    }
    const size_t r = (size_t)(std::upper_bound(l.first.begin(), l.first.end(), b) - l.first.begin()) - 1;
    const uint32_t j = b - l.first[r];
    *lo = ((uint64_t)r << 32) | ((uint64_t)j << SORTWIN_SHIFT);
    *hi = ((uint64_t)r << 32) | (j + 1 == l.nb[r] ? (uint64_t)0xffffffffu : (((uint64_t)j + 1) << SORTWIN_SHIFT) - 1);
    if (ref) *ref = (int64_t)r;
}

inline uint64_t sortwin_cost(uint64_t bytes, uint64_t records) { return bytes + SORTWIN_ITEM_COST * records; }

struct SortWindow {
    uint32_t b0, b1;          // buckets b0 .. b1 - 1
    uint64_t bytes, records;  // what they hold
};

// The windows: runs of consecutive buckets whose cost is at most `budget`, chosen greedily front to back; together they
// cover every bucket (one window when nothing was measured).  A bucket that holds nothing joins the window it lies in.
// -1: done; else the first bucket that alone costs more than the budget (nothing of `out` is to be used then).
inline int64_t choose_windows(const uint64_t *bytes, const uint64_t *records, uint32_t n_buckets, uint64_t budget, std::vector<SortWindow> &out) {
    out.clear();
    SortWindow w = {0, 0, 0, 0};
    for (uint32_t b = 0; b < n_buckets; b++) {
        if (sortwin_cost(bytes[b], records[b]) > budget) return (int64_t)b;
        if (sortwin_cost(w.bytes + bytes[b], w.records + records[b]) > budget) {
            w.b1 = b;
            out.push_back(w);
            w = {b, b, 0, 0};
        }
        w.bytes += bytes[b];
        w.records += records[b];
    }
    w.b1 = n_buckets;
    out.push_back(w);
    return -1;
}

}  // namespace recstore
}  // namespace fadehip
