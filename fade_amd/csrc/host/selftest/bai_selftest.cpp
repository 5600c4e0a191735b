// bai_selftest — host/bai_build.hpp, the host's part of --write-index, on the CPU (ASan + UBSan build; no device, no library).
//
//   bai_selftest          hand cases of the rule tests/bai_model.py states (expected bytes written out here), and random
//                         sorted record sets cut into calls at random places: every split gives the bytes of the whole
//   bai_selftest FILE     the calls FILE describes -> the .bai as one line of hex on stdout (tests/test_bai_selftest.py holds
//                         it to the model's bytes).  Lines: "R n_ref" | "C base n_records first_key last_key" |
//                         "c tid bin beg end" | "l tid window off" | "r tid off_beg off_end n_mapped n_unmapped" | "E" (add
//                         the call; a refusal prints "ERR code message") | "F" (finish)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../bai_build.hpp"

using fadehip::bai::Builder;

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

uint32_t reg2bin(uint64_t beg, uint64_t end) {
    end--;
    if (beg >> 14 == end >> 14) return 4681u + (uint32_t)(beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (uint32_t)(beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (uint32_t)(beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (uint32_t)(beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (uint32_t)(beg >> 26);
    return 0;
}
uint64_t key_of(const Rec &r) { return ((uint64_t)(uint32_t)r.tid << 32) | (uint32_t)(r.pos + 1); }

// the device stage's rule over records [lo, hi), serially (what bam_index.hpp computes with scans)
void per_call(const std::vector<Rec> &recs, size_t lo, size_t hi, Call &out) {
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
        const uint32_t b = reg2bin(beg, end);
        if (b != last_bin) out.chunks.push_back(fadehip_index_chunk{r.tid, b, r.u, r.v});
        last_bin = b;
        out.chunks.back().end = r.v;
        if (mapped) {
            const int64_t w0 = (int64_t)(beg >> 14), w1 = (int64_t)((end - 1) >> 14);
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
    {  // no record at all: the magic, n_ref empty references, n_no_coor
        Builder b(2);
        const std::vector<uint8_t> v = finish(b);
        CHECK(v.size() == 8 + 2 * 8 + 8);
        CHECK(memcmp(v.data(), "BAI\1", 4) == 0 && rd32(v, 4) == 2 && rd64(v, 24) == 0);
    }
    {  // one reference, two bins, a window without a record, an unmapped tail; the reference in between stays empty
        std::vector<Rec> r = {{1, 10, 0, 50, 0x10000, 0x10064}, {1, 40000, 4, 0, 0x10064, 0x100c8}, {1, 40001, 0, 5, 0x100c8, 0x20000}, {-1, -1, 4, 0, 0x20000, 0x20010}};
        Call c;
        per_call(r, 0, r.size(), c);
        CHECK(c.chunks.size() == 2 && c.linear.size() == 2 && c.refs.size() == 2);
        Builder b(3);
        CHECK(b.add(0, &c.c) == 0);
        const std::vector<uint8_t> v = finish(b);
        size_t at = 8;
        CHECK(rd32(v, at) == 0 && rd32(v, at + 4) == 0);  // reference 0
        at += 8;
        CHECK(rd32(v, at) == 3);  // bins 4681, 4683 and the pseudo-bin
        at += 4;
        CHECK(rd32(v, at) == 4681 && rd32(v, at + 4) == 1 && rd64(v, at + 8) == 0x10000 && rd64(v, at + 16) == 0x10064);
        at += 24;
        CHECK(rd32(v, at) == 4683 && rd32(v, at + 4) == 1 && rd64(v, at + 8) == 0x10064 && rd64(v, at + 16) == 0x20000);
        at += 24;
        CHECK(rd32(v, at) == 37450 && rd32(v, at + 4) == 2 && rd64(v, at + 8) == 0x10000 && rd64(v, at + 16) == 0x20000 && rd64(v, at + 24) == 2 && rd64(v, at + 32) == 1);
        at += 40;
        CHECK(rd32(v, at) == 3);  // windows 0 .. 2; window 1 takes window 2's offset
        CHECK(rd64(v, at + 4) == 0x10000 && rd64(v, at + 12) == 0x100c8 && rd64(v, at + 20) == 0x100c8);
        at += 4 + 24;
        CHECK(rd32(v, at) == 0 && rd32(v, at + 4) == 0);  // reference 2
        at += 8;
        CHECK(rd64(v, at) == 1 && at + 8 == v.size());
    }
    {  // chunks of one bin merge while the next begins in the block the one before ends in; the base is added
        Call c;
        c.chunks = {{0, 4681, 0x0, 0x50}, {0, 4681, 0x90, 0x10010}, {0, 4681, 0x10020, 0x10030}, {0, 4681, 0x20000, 0x20010}};
        c.refs = {{0, 0, 0, 0x20010, 4, 0}};
        c.linear = {{0, 0, 0}};
        c.seal(4, 1, 4);
        Builder b(1);
        CHECK(b.add(100, &c.c) == 0);
        const std::vector<uint8_t> v = finish(b);
        const uint64_t s = 100ull << 16;
        CHECK(rd32(v, 12) == 4681 && rd32(v, 16) == 2);
        CHECK(rd64(v, 20) == s && rd64(v, 28) == s + 0x10030 && rd64(v, 36) == s + 0x20000 && rd64(v, 44) == s + 0x20010);
    }
    {  // first writer wins; keys between calls; a refused call leaves the builder as it was
        Call a, d;
        a.linear = {{0, 3, 0x10}};
        a.refs = {{0, 0, 0x10, 0x20, 1, 0}};
        a.chunks = {{0, 4684, 0x10, 0x20}};
        a.seal(1, 50000, 50000);
        d = a;
        d.linear = {{0, 3, 0x999}, {0, 4, 0x30}};
        d.seal(1, 49999, 70000);
        Builder b(1);
        CHECK(b.add(0, &a.c) == 0);
        const std::vector<uint8_t> before = finish(b);
        CHECK(b.add(0, &d.c) == FADEHIP_E_INVALID);
        CHECK(b.err == "bam stream: record 1: not in coordinate order (--write-index needs coordinate-sorted output)");
        CHECK(finish(b) == before);
        d.seal(1, 50000, 70000);
        CHECK(b.add(0, &d.c) == 0);
        const std::vector<uint8_t> v = finish(b);
        // bins: 4684 (one merged chunk) + pseudo; then n_intv 5: windows 0 .. 3 -> 0x10, 4 -> 0x30
        const size_t at = 8 + 4 + 24 + 40;
        CHECK(rd32(v, at) == 5 && rd64(v, at + 4) == 0x10 && rd64(v, at + 4 + 24) == 0x10 && rd64(v, at + 4 + 32) == 0x30);
        Call bad = a;
        bad.chunks[0].tid = 1;
        bad.seal(1, 80000, 80000);
        CHECK(b.add(0, &bad.c) == FADEHIP_E_INVALID && finish(b) == v);
        CHECK(b.add(0, nullptr) == FADEHIP_E_INVALID);
    }
}

void random_splits() {
    std::mt19937_64 rng(7);
    for (int round = 0; round < 40; round++) {
        std::vector<Rec> recs;
        const int n_ref = 1 + (int)(rng() % 4);
        uint64_t file = 0;
        const uint64_t block = round % 2 ? 0x7f00 : 0x400;
        auto voff = [&](uint64_t p) { return ((p / block * (block / 2 + 26)) << 16) | (p % block); };
        for (int tid = 0; tid < n_ref; tid++) {
            if (rng() % 4 == 0) continue;
            int32_t pos = rng() % 3 ? 0 : -1;
            const int n = (int)(rng() % 300);
            for (int k = 0; k < n; k++) {
                const uint64_t lens[] = {0, 1, 80, 150, 20000, 130000};
                const uint64_t size = 40 + rng() % 300;
                recs.push_back(Rec{tid, pos, rng() % 20 ? 0u : 4u, lens[rng() % 6], voff(file), voff(file + size)});
                file += size;
                pos += (int32_t)(rng() % 4 ? rng() % 50 : rng() % 30000);
            }
        }
        for (int k = (int)(rng() % 5); k > 0; k--) {
            recs.push_back(Rec{-1, -1, 4, 0, voff(file), voff(file + 60)});
            file += 60;
        }
        Call c;
        Builder whole(n_ref);
        per_call(recs, 0, recs.size(), c);
        CHECK(whole.add(0, &c.c) == 0);
        const std::vector<uint8_t> want = finish(whole);
        for (int split = 0; split < 8; split++) {
            Builder b(n_ref);
            size_t at = 0;
            while (at < recs.size() || rng() % 3 == 0) {
                const size_t take = rng() % 4 == 0 ? 0 : std::min<size_t>(recs.size() - at, rng() % 200);
                per_call(recs, at, at + take, c);
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
        long long a0, a1;
        unsigned long long q0, q1, q2, q3;
        if (sscanf(line, "R %lld", &a0) == 1) {
            delete b;
            b = new Builder((int32_t)a0);
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
            if (b->finish(&p, &n)) return 3;
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
        fprintf(stderr, "bai_selftest: %d checks failed\n", g_failed);
        return 1;
    }
    printf("bai_selftest ok\n");
    return 0;
}
