// csi_selftest — host/csi_build.hpp, the host's part of --write-index --csi, on the CPU (ASan + UBSan build; no device, no
// library).
//
//   csi_selftest          hand cases of the rule tests/csi_model.py states (expected bytes written out here), and random
//                         sorted record sets under several geometries cut into calls at random places: every split gives
//                         the payload of the whole
//   csi_selftest FILE     the calls FILE describes -> the payload as one line of hex on stdout (tests/test_csi_selftest.py
//                         holds it to the model's bytes).  Lines: "R n_ref min_shift depth" | "C base n_records first_key
//                         last_key" | "c tid bin beg end" | "l tid window off" | "r tid off_beg off_end n_mapped n_unmapped"
//                         | "E" (add the call; a refusal prints "ERR code message") | "F" (finish)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../csi_build.hpp"

using fadehip::csi::Builder;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                         \
        }                                                                       \
    } while (0)

struct Rec {
    int32_t tid, pos;
    uint32_t flag;
    uint64_t reflen, u, v;
};

struct Call {
    std::vector<fadehip_index_chunk> chunks;
    std::vector<fadehip_index_linear> linear;
    std::vector<fadehip_index_ref> refs;
    fadehip_index_call c;
    void seal(int64_t n, uint64_t k0, uint64_t k1) {
        c.chunks = chunks.data();
        c.linear = linear.data();
        c.refs = refs.data();
        c.n_chunks = (int64_t)chunks.size();
        c.n_linear = (int64_t)linear.size();
        c.n_refs = (int64_t)refs.size();
        c.n_records = n;
        c.first_key = k0;
        c.last_key = k1;
    }
};

// the deepest bin that holds [beg, end), level by level from the leaves
uint32_t reg2bin(uint64_t beg, uint64_t end, int min_shift, int depth) {
    end--;
    for (int level = depth, s = min_shift; level > 0; level--, s += 3)
        if (beg >> s == end >> s) return fadehip::csi::first_bin(level) + (uint32_t)(beg >> s);
    return 0;
}
uint64_t key_of(const Rec &r) { return ((uint64_t)(uint32_t)r.tid << 32) | (uint32_t)(r.pos + 1); }

// the device stage's rule over records [lo, hi) under a geometry, serially
void per_call(const std::vector<Rec> &recs, size_t lo, size_t hi, int min_shift, int depth, Call &out) {
    out.chunks.clear();
    out.linear.clear();
    out.refs.clear();
    int64_t run_max = -1;
    uint32_t last_bin = ~0u;
    for (size_t i = lo; i < hi; i++) {
        const Rec &r = recs[i];
        const bool mapped = !(r.flag & 4u);
        const uint64_t beg = r.pos > 0 ? (uint64_t)r.pos : 0, end = beg + (mapped && r.reflen ? r.reflen : 1);
        if (i == lo || recs[i - 1].tid != r.tid) {
            out.refs.push_back(fadehip_index_ref{r.tid, 0, r.u, r.v, 0, 0});
            run_max = -1;
            last_bin = ~0u;
        }
        out.refs.back().off_end = r.v;
        (mapped ? out.refs.back().n_mapped : out.refs.back().n_unmapped)++;
        if (r.tid < 0) continue;
        const uint32_t b = reg2bin(beg, end, min_shift, depth);
        if (b != last_bin) out.chunks.push_back(fadehip_index_chunk{r.tid, b, r.u, r.v});
        last_bin = b;
        out.chunks.back().end = r.v;
        if (mapped) {
            const int64_t w0 = (int64_t)(beg >> min_shift), w1 = (int64_t)((end - 1) >> min_shift);
            for (int64_t w = std::max(w0, run_max + 1); w <= w1; w++) out.linear.push_back(fadehip_index_linear{r.tid, (uint32_t)w, r.u});
            run_max = std::max(run_max, w1);
        }
    }
    out.seal((int64_t)(hi - lo), hi > lo ? key_of(recs[lo]) : 0, hi > lo ? key_of(recs[hi - 1]) : 0);
}

std::vector<uint8_t> finish(Builder &b) {
    const uint8_t *p = nullptr;
    size_t n = 0;
    CHECK(b.finish(&p, &n) == 0);
    return std::vector<uint8_t>(p, p + n);
}

uint32_t rd32(const std::vector<uint8_t> &v, size_t at) {
    uint32_t x;
    memcpy(&x, &v[at], 4);
    return x;
}
uint64_t rd64(const std::vector<uint8_t> &v, size_t at) {
    uint64_t x;
    memcpy(&x, &v[at], 8);
    return x;
}

void hand_cases() {
    CHECK(fadehip::csi::pseudo_bin(5) == 37450 && fadehip::csi::pseudo_bin(6) == 299594 && fadehip::csi::first_bin(5) == 4681);
    CHECK(fadehip::csi::valid_geometry(14, 6) && fadehip::csi::valid_geometry(4, 1) && !fadehip::csi::valid_geometry(3, 2) && !fadehip::csi::valid_geometry(14, 7) &&
          !fadehip::csi::valid_geometry(4, 9) && !fadehip::csi::valid_geometry(14, 0));
    {  // no record at all: the magic, the geometry, l_aux, n_ref empty references, n_no_coor
        Builder b(2, 14, 6);
        const std::vector<uint8_t> v = finish(b);
        CHECK(v.size() == 20 + 2 * 4 + 8);
        CHECK(memcmp(v.data(), "CSI\1", 4) == 0 && rd32(v, 4) == 14 && rd32(v, 8) == 6 && rd32(v, 12) == 0 && rd32(v, 16) == 2 && rd64(v, 28) == 0);
    }
    {  // (4, 2): a bin whose first window is empty takes the next window's value; a bin behind the last window takes 0
        std::vector<Rec> r = {{0, 33, 0, 20, 100, 200}, {0, 85, 4, 0, 200, 300}, {0, 100, 0, 5, 300, 400}, {0, 970, 4, 0, 400, 500}, {-1, -1, 4, 0, 500, 600}};
        Call c;
        per_call(r, 0, r.size(), 4, 2, c);
        CHECK(c.chunks.size() == 4 && c.linear.size() == 3 && c.refs.size() == 2);
        Builder b(1, 4, 2);
        CHECK(b.add(0, &c.c) == 0);
        const std::vector<uint8_t> v = finish(b);
        size_t at = 20;
        CHECK(rd32(v, at) == 5);  // bins 1, 14, 15, 69 and the pseudo-bin
        at += 4;
        const uint32_t bins[4] = {1, 14, 15, 69};
        const uint64_t loff[4] = {100, 300, 300, 0}, beg[4] = {100, 200, 300, 400};
        for (int k = 0; k < 4; k++) {
            CHECK(rd32(v, at) == bins[k] && rd64(v, at + 4) == loff[k] && rd32(v, at + 12) == 1 && rd64(v, at + 16) == beg[k] && rd64(v, at + 24) == beg[k] + 100);
            at += 32;
        }
        CHECK(rd32(v, at) == 74 && rd64(v, at + 4) == 0 && rd32(v, at + 12) == 2);  // ((1 << 9) - 1) / 7 + 1
        CHECK(rd64(v, at + 16) == 100 && rd64(v, at + 24) == 500 && rd64(v, at + 32) == 2 && rd64(v, at + 40) == 2);
        at += 48;
        CHECK(rd64(v, at) == 1 && at + 8 == v.size());
    }
    {  // chunks of one bin merge while the next begins in the block the one before ends in; the base is added
        Call c;
        c.chunks = {{0, 37449, 0x0, 0x50}, {0, 37449, 0x90, 0x10010}, {0, 37449, 0x10020, 0x10030}, {0, 37449, 0x20000, 0x20010}};
        c.refs = {{0, 0, 0, 0x20010, 4, 0}};
        c.linear = {{0, 0, 0x0}};
        c.seal(4, 1, 4);
        Builder b(1, 14, 6);
        CHECK(b.add(100, &c.c) == 0);
        const std::vector<uint8_t> v = finish(b);
        const uint64_t s = 100ull << 16;
        CHECK(rd32(v, 24) == 37449 && rd64(v, 28) == s && rd32(v, 36) == 2);
        CHECK(rd64(v, 40) == s && rd64(v, 48) == s + 0x10030 && rd64(v, 56) == s + 0x20000 && rd64(v, 64) == s + 0x20010);
    }
    {  // keys between calls; what is out of range; a refused call leaves the builder as it was
        Call a, d;
        a.linear = {{0, 3, 0x10}};
        a.refs = {{0, 0, 0x10, 0x20, 1, 0}};
        a.chunks = {{0, 9 + 3, 0x10, 0x20}};
        a.seal(1, 50, 50);
        d = a;
        d.seal(1, 49, 70);
        Builder b(1, 4, 2);
        CHECK(b.add(0, &a.c) == 0);
        const std::vector<uint8_t> before = finish(b);
        CHECK(b.add(0, &d.c) == FADEHIP_E_INVALID);
        CHECK(b.err == "bam stream: record 1: not in coordinate order (--write-index needs coordinate-sorted output)");
        CHECK(finish(b) == before);
        Call bad = a;
        bad.chunks[0].bin = 73;  // (4, 2) has bins 0 .. 72
        bad.seal(1, 80, 80);
        CHECK(b.add(0, &bad.c) == FADEHIP_E_INVALID && b.err == "csi: chunk 0 names reference or bin out of range" && finish(b) == before);
        bad = a;
        bad.linear[0].window = 64;  // ... and windows 0 .. 63
        bad.seal(1, 80, 80);
        CHECK(b.add(0, &bad.c) == FADEHIP_E_INVALID && finish(b) == before);
        CHECK(b.add(0, nullptr) == FADEHIP_E_INVALID);
    }
}

void random_splits() {
    std::mt19937_64 rng(7);
    const int geo[4][2] = {{4, 2}, {6, 3}, {14, 5}, {14, 6}};
    for (int round = 0; round < 40; round++) {
        const int min_shift = geo[round % 4][0], depth = geo[round % 4][1];
        const uint64_t limit = 1ull << (min_shift + 3 * depth), win = 1ull << min_shift;
        std::vector<Rec> recs;
        const int n_ref = 1 + (int)(rng() % 4);
        uint64_t file = 0;
        const uint64_t block = round % 2 ? 0x7f00 : 0x400;
        auto voff = [&](uint64_t p) { return ((p / block * (block / 2 + 26)) << 16) | (p % block); };
        for (int tid = 0; tid < n_ref; tid++) {
            if (rng() % 4 == 0) continue;
            uint64_t pos = round % 8 == 3 ? (1ull << 29) - 5 * win : 0;  // ((14, 6): across BAI's limit)
            const int n = (int)(rng() % 300);
            const uint64_t step = std::max<uint64_t>(std::min<uint64_t>(limit / 600, 2 * win), 1);
            for (int k = 0; k < n; k++) {
                const uint64_t lens[] = {0, 1, win / 4, win, 2 * win + 1, 9 * win};
                const uint64_t size = 40 + rng() % 300;
                if (pos >= limit || pos >= 0x7fffffffull) break;
                const uint64_t len = std::min<uint64_t>(lens[rng() % 6], limit - pos);
                recs.push_back(Rec{tid, (int32_t)pos, rng() % 20 ? 0u : 4u, len, voff(file), voff(file + size)});
                file += size;
                pos += rng() % 4 ? rng() % (step / 2 + 1) : rng() % (2 * step);
            }
        }
        for (int k = (int)(rng() % 5); k > 0; k--) {
            recs.push_back(Rec{-1, -1, 4, 0, voff(file), voff(file + 60)});
            file += 60;
        }
        Call c;
        Builder whole(n_ref, min_shift, depth);
        per_call(recs, 0, recs.size(), min_shift, depth, c);
        CHECK(whole.add(0, &c.c) == 0);
        const std::vector<uint8_t> want = finish(whole);
        for (int split = 0; split < 8; split++) {
            Builder b(n_ref, min_shift, depth);
            size_t at = 0;
            while (at < recs.size() || rng() % 3 == 0) {
                const size_t take = rng() % 4 == 0 ? 0 : std::min<size_t>(recs.size() - at, rng() % 200);
                per_call(recs, at, at + take, min_shift, depth, c);
                CHECK(b.add(0, &c.c) == 0);
                at += take;
                if (at >= recs.size() && rng() % 2) break;
            }
            CHECK(at == recs.size() && finish(b) == want);
        }
    }
}

int from_file(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    Builder *b = nullptr;
    Call c;
    uint64_t base = 0;
    char line[512];
    while (fgets(line, sizeof line, f)) {
        long long a0, a1, a2;
        unsigned long long q0, q1, q2, q3;
        if (sscanf(line, "R %lld %lld %lld", &a0, &a1, &a2) == 3) {
            delete b;
            b = nullptr;
            if (!fadehip::csi::valid_geometry((int32_t)a1, (int32_t)a2)) {
                fprintf(stderr, "geometry (%lld, %lld) is not valid\n", a1, a2);
                fclose(f);
                return 4;
            }
            b = new Builder((int32_t)a0, (int32_t)a1, (int32_t)a2);
        } else if (sscanf(line, "C %llu %lld %llu %llu", &q0, &a0, &q1, &q2) == 4) {
            c = Call();
            base = q0;
            c.seal(a0, q1, q2);
        } else if (sscanf(line, "c %lld %lld %llu %llu", &a0, &a1, &q0, &q1) == 4) {
            c.chunks.push_back(fadehip_index_chunk{(int32_t)a0, (uint32_t)a1, q0, q1});
        } else if (sscanf(line, "l %lld %lld %llu", &a0, &a1, &q0) == 3) {
            c.linear.push_back(fadehip_index_linear{(int32_t)a0, (uint32_t)a1, q0});
        } else if (sscanf(line, "r %lld %llu %llu %llu %llu", &a0, &q0, &q1, &q2, &q3) == 5) {
            c.refs.push_back(fadehip_index_ref{(int32_t)a0, 0, q0, q1, q2, q3});
        } else if (line[0] == 'E' && b) {
            c.seal(c.c.n_records, c.c.first_key, c.c.last_key);
            const int rc = b->add(base, &c.c);
            if (rc) printf("ERR %d %s\n", rc, b->err.c_str());
        } else if (line[0] == 'F' && b) {
            const uint8_t *p = nullptr;
            size_t n = 0;
            if (b->finish(&p, &n)) {
                delete b;
                fclose(f);
                return 3;
            }
            for (size_t k = 0; k < n; k++) printf("%02x", p[k]);
            printf("\n");
        }
    }
    delete b;
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1) return from_file(argv[1]);
    hand_cases();
    random_splits();
    if (g_failed) {
        fprintf(stderr, "csi_selftest: %d checks failed\n", g_failed);
        return 1;
    }
    printf("csi_selftest ok\n");
    return 0;
}
