// sortwin_selftest — host/recstore_host.hpp's buckets and windows on the hand cases of tests/test_sorted_out_model.py and
// against a plain loop over random tables (CPU only; the Makefile builds it with ASan + UBSan).
#include "../recstore_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace fadehip::recstore;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                 \
        }                                                            \
    } while (0)

static uint64_t key(int32_t tid, int32_t pos) { return ((uint64_t)(uint32_t)tid << 32) | (uint32_t)(pos + 1); }

// the rule as tests/sorted_out_model.py states it, every window's cost summed from scratch
static int64_t windows_loop(const std::vector<uint64_t> &bytes, const std::vector<uint64_t> &recs, uint64_t budget, std::vector<std::pair<uint32_t, uint32_t>> &out) {
    out.clear();
    const uint32_t n = (uint32_t)bytes.size();
    for (uint32_t b = 0; b < n; b++)
        if (bytes[b] + 64 * recs[b] > budget) return b;
    uint32_t b0 = 0;
    while (b0 < n) {
        uint32_t e = b0;
        for (;;) {
            if (e == n) break;
            uint64_t c = 0;
            for (uint32_t b = b0; b <= e; b++) c += bytes[b] + 64 * recs[b];
            if (c > budget) break;
            e++;
        }
        out.emplace_back(b0, e);
        b0 = e;
    }
    if (out.empty()) out.emplace_back(0u, n);
    return -1;
}

int main() {
    {
        // contigs: 200,000 bases (4 buckets), 10 bases (1), 65,535 (2), 65,534 (1), 0 (1); then the last bucket
        const uint32_t len[] = {200000, 10, 65535, 65534, 0};
        BucketLayout l;
        CHECK(bucket_layout(len, 5, l));
        CHECK((l.nb == std::vector<uint32_t>{4, 1, 2, 1, 1}));
        CHECK((l.first == std::vector<uint32_t>{0, 4, 5, 7, 8}));
        CHECK(l.n_buckets == 10);
        CHECK(bucket_of(l, key(0, -1)) == 0);
        CHECK(bucket_of(l, key(0, 65534)) == 0);   // pos + 1 = 65535
        CHECK(bucket_of(l, key(0, 65535)) == 1);   // pos + 1 = 65536
        CHECK(bucket_of(l, key(0, 199999)) == 3);
        CHECK(bucket_of(l, key(0, 2000000000)) == 3);  // beyond the contig: its last bucket
        CHECK(bucket_of(l, key(0, -2)) == 3);          // (pos + 1 as u32 is all ones)
        CHECK(bucket_of(l, key(1, 0)) == 4);
        CHECK(bucket_of(l, key(1, 70000)) == 4);       // a contig shorter than one bucket
        CHECK(bucket_of(l, key(2, 65534)) == 5);
        CHECK(bucket_of(l, key(2, 65535)) == 6);
        CHECK(bucket_of(l, key(3, 65535)) == 7);
        CHECK(bucket_of(l, key(4, 5)) == 8);
        CHECK(bucket_of(l, key(-1, -1)) == 9);
        CHECK(bucket_of(l, key(-1, 77)) == 9);         // refID -1 with a pos
        CHECK(bucket_of(l, key(5, 0)) == 9);           // a refID outside the header
        CHECK(bucket_of(l, ~(uint64_t)0) == 9);
        uint64_t lo, hi;
        int64_t ref;
        bucket_range(l, 0, &lo, &hi, &ref);
        CHECK(lo == 0 && hi == 65535 && ref == 0);
        bucket_range(l, 1, &lo, &hi, &ref);
        CHECK(lo == 65536 && hi == 131071 && ref == 0);
        bucket_range(l, 3, &lo, &hi, &ref);
        CHECK(lo == 3 * 65536 && hi == 0xffffffffull && ref == 0);
        bucket_range(l, 4, &lo, &hi, &ref);
        CHECK(lo == (1ull << 32) && hi == ((1ull << 32) | 0xffffffffull) && ref == 1);
        bucket_range(l, 6, &lo, &hi, &ref);
        CHECK(lo == ((2ull << 32) | 65536) && hi == ((2ull << 32) | 0xffffffffull) && ref == 2);
        bucket_range(l, 9, &lo, &hi, &ref);
        CHECK(lo == (5ull << 32) && hi == ~(uint64_t)0 && ref == -1);
        // every bucket's range maps back to it, and the ranges abut
        uint64_t next = 0;
        for (uint32_t b = 0; b < l.n_buckets; b++) {
            bucket_range(l, b, &lo, &hi);
            CHECK(lo == next && bucket_of(l, lo) == b && bucket_of(l, hi) == b);
            next = hi + 1;
        }
        CHECK(next == 0);
        BucketLayout none;
        CHECK(bucket_layout(nullptr, 0, none) && none.n_buckets == 1 && bucket_of(none, key(0, 5)) == 0);
        bucket_range(none, 0, &lo, &hi, &ref);
        CHECK(lo == 0 && hi == ~(uint64_t)0 && ref == -1);
        const uint32_t big[] = {0xffffffffu};
        BucketLayout lb;
        CHECK(bucket_layout(big, 1, lb) && lb.nb[0] == 65537 && bucket_of(lb, key(0, -2)) == 65535);
    }
    {
        // bytes / records per bucket; cost = bytes + 64 records
        const std::vector<uint64_t> by = {100, 0, 0, 300, 0, 136, 0}, rc = {1, 0, 0, 2, 0, 1, 0};
        std::vector<SortWindow> w;
        CHECK(choose_windows(by.data(), rc.data(), 7, 1000, w) == -1 && w.size() == 1 && w[0].b0 == 0 && w[0].b1 == 7 && w[0].bytes == 536 && w[0].records == 4);
        // 164 | 428 | 200: the empty buckets between them stay with the window in front
        CHECK(choose_windows(by.data(), rc.data(), 7, 428, w) == -1 && w.size() == 3);
        CHECK(w[0].b0 == 0 && w[0].b1 == 3 && w[1].b0 == 3 && w[1].b1 == 5 && w[2].b0 == 5 && w[2].b1 == 7);
        CHECK(w[1].bytes == 300 && w[1].records == 2);
        CHECK(choose_windows(by.data(), rc.data(), 7, 592, w) == -1 && w.size() == 2 && w[0].b1 == 5 && w[1].b0 == 5);
        CHECK(choose_windows(by.data(), rc.data(), 7, 591, w) == -1 && w.size() == 3);
        CHECK(choose_windows(by.data(), rc.data(), 7, 427, w) == 3);   // bucket 3 alone is over
        CHECK(choose_windows(by.data(), rc.data(), 7, 0, w) == 0);
        const std::vector<uint64_t> z(4, 0);
        CHECK(choose_windows(z.data(), z.data(), 4, 0, w) == -1 && w.size() == 1 && w[0].b0 == 0 && w[0].b1 == 4);
    }
    std::mt19937_64 rng(11);
    for (int round = 0; round < 3000; round++) {
        const uint32_t n = 1 + (uint32_t)(rng() % 30);
        std::vector<uint64_t> by(n), rc(n);
        for (uint32_t b = 0; b < n; b++) {
            rc[b] = rng() % 3 == 0 ? 0 : rng() % 20;
            by[b] = rc[b] * (36 + rng() % 400);
        }
        uint64_t total = 0, most = 0;
        for (uint32_t b = 0; b < n; b++) {
            total += by[b] + 64 * rc[b];
            most = std::max(most, by[b] + 64 * rc[b]);
        }
        const uint64_t budget = round % 4 == 0 ? most : round % 4 == 1 ? most + rng() % (total - most + 1) : rng() % (total + 50);
        std::vector<SortWindow> w;
        std::vector<std::pair<uint32_t, uint32_t>> want;
        const int64_t bad = choose_windows(by.data(), rc.data(), n, budget, w);
        CHECK(bad == windows_loop(by, rc, budget, want));
        if (bad >= 0) continue;
        CHECK(w.size() == want.size());
        for (size_t k = 0; k < w.size() && k < want.size(); k++) {
            CHECK(w[k].b0 == want[k].first && w[k].b1 == want[k].second);
            uint64_t sb = 0, sr = 0;
            for (uint32_t b = w[k].b0; b < w[k].b1; b++) sb += by[b], sr += rc[b];
            CHECK(sb == w[k].bytes && sr == w[k].records && sortwin_cost(sb, sr) <= budget);
        }
        CHECK(w.front().b0 == 0 && w.back().b1 == n);
    }
    if (fails) return 1;
    puts("sortwin_selftest ok");
    return 0;
}
