// recstore_selftest — host/recstore_host.hpp on the hand cases of tests/test_recstore_model.py and against a plain loop over
// random sizes (CPU only; the Makefile builds it with ASan + UBSan).
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

static std::vector<uint64_t> offsets(const std::vector<uint64_t> &sizes) {
    std::vector<uint64_t> d(sizes.size() + 1, 0);
    for (size_t k = 0; k < sizes.size(); k++) d[k + 1] = d[k] + sizes[k];
    return d;
}

// the rule as tests/recstore_model.py states it
static size_t cut_loop(const std::vector<uint64_t> &sizes, size_t j0, uint64_t max_payload) {
    size_t j = j0;
    uint64_t total = 0;
    while (j < sizes.size() && total + sizes[j] <= max_payload) total += sizes[j++];
    return j > j0 ? j : j0 + 1;
}

int main() {
    {
        const std::vector<uint64_t> sizes = {10, 10, 50, 10, 10, 10}, d = offsets(sizes);
        const size_t n = sizes.size();
        CHECK(drain_cut(d.data(), n, 0, 20) == 2);
        CHECK(drain_cut(d.data(), n, 0, 29) == 2);
        CHECK(drain_cut(d.data(), n, 0, 1) == 1);
        CHECK(drain_cut(d.data(), n, 2, 20) == 3);
        CHECK(drain_cut(d.data(), n, 2, 60) == 4);
        CHECK(drain_cut(d.data(), n, 3, 1000) == 6);
        CHECK(drain_cut(d.data(), n, 5, 0) == 6);
        CHECK(drain_cut(d.data(), n, 0, UINT64_MAX) == 6);
        CHECK(drain_cut(d.data(), n, 4, UINT64_MAX) == 6);
    }
    std::mt19937_64 rng(7);
    for (int round = 0; round < 2000; round++) {
        std::vector<uint64_t> sizes(1 + rng() % 40);
        for (auto &s : sizes) s = 36 + rng() % (round % 3 ? 300 : 70000);
        const std::vector<uint64_t> d = offsets(sizes);
        const uint64_t mp = round % 5 == 0 ? rng() % 8 : rng() % (d.back() + 100);
        for (size_t j0 = 0; j0 < sizes.size(); j0++) CHECK(drain_cut(d.data(), sizes.size(), j0, mp) == cut_loop(sizes, j0, mp));
    }
    const std::string sq = "@SQ\tSN:c0\tLN:100\n";
    CHECK(header_sorted("@HD\tVN:1.5\tSO:unsorted\n" + sq) == "@HD\tVN:1.5\tSO:coordinate\n" + sq);
    CHECK(header_sorted("@HD\tVN:1.4\tSO:queryname\tGO:query\n" + sq) == "@HD\tVN:1.4\tSO:coordinate\tGO:query\n" + sq);
    CHECK(header_sorted("@HD\tVN:1.6\n" + sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq);
    CHECK(header_sorted(sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq);
    CHECK(header_sorted("") == "@HD\tVN:1.6\tSO:coordinate\n");
    CHECK(header_sorted("@HDX\tVN:1\n") == "@HD\tVN:1.6\tSO:coordinate\n@HDX\tVN:1\n");
    CHECK(header_sorted("@HD\tVN:1.6") == "@HD\tVN:1.6\tSO:coordinate");
    CHECK(header_sorted("@HD") == "@HD\tSO:coordinate");
    CHECK(header_sorted("@HD\tSO:a\tSO:b\tX:1\n") == "@HD\tSO:coordinate\tX:1\n");
    CHECK(header_sorted("@HD\tVN:1.6\tSO:unknown") == "@HD\tVN:1.6\tSO:coordinate");
    if (fails) return 1;
    puts("recstore_selftest ok");
    return 0;
}
