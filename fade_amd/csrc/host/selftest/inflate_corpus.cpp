// inflate_corpus.cpp — host/inflate_fast.hpp against a corpus of hand-built DEFLATE streams (tests/deflate_cases.py writes
// the file, zlib decided every verdict and every byte in it).  CPU only; ASan + UBSan build.
//
//   inflate_corpus corpus.bin
//
// File: "FCRP", u32 n, then per case u32 name_len, name, u32 raw_len, raw, u32 valid, u32 payload_len, payload (little
// endian).  For an invalid case the payload is the one its member's trailer would claim: only its length is used.
// Per case: FastInflate::inflate into a buffer of exactly the payload's size between two guard regions; for valid cases
// the same with out_len one less and one more (both must fail); FastInflate::inflate2 with the case as stream A and as
// stream B against itself, the previous case and a stored-only stream, and for valid cases against itself and the stored-only
// stream with the case's out_len one less and one more (must fail).  One line per failing case, then a count.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../inflate_fast.hpp"

using htsl::FastInflate;

struct Case {
    std::string name;
    std::vector<uint8_t> raw, payload;
    bool valid;
};

static constexpr size_t GUARD = 64;
static constexpr uint8_t GUARD_BYTE = 0xa5, FILL_BYTE = 0xee;

// an output buffer of exactly n bytes with guard bytes on both sides
struct Guarded {
    std::vector<uint8_t> mem;
    size_t n;
    explicit Guarded(size_t n_) : mem(n_ + 2 * GUARD, GUARD_BYTE), n(n_) { memset(mem.data() + GUARD, FILL_BYTE, n); }
    uint8_t *out() { return mem.data() + GUARD; }
    bool guards_intact() const {
        for (size_t i = 0; i < GUARD; i++)
            if (mem[i] != GUARD_BYTE || mem[GUARD + n + i] != GUARD_BYTE) return false;
        return true;
    }
    bool equals(const std::vector<uint8_t> &want) const { return want.size() == n && (n == 0 || memcmp(mem.data() + GUARD, want.data(), n) == 0); }
};

// the input in an allocation of its own size (ASan sees any read beyond it)
struct Input {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Input(const std::vector<uint8_t> &v) : p(new uint8_t[v.size() ? v.size() : 1]), n(v.size()) {
        if (n) memcpy(p.get(), v.data(), n);
    }
};

static bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
static bool read_bytes(FILE *f, std::vector<uint8_t> &v) {
    uint32_t n;
    if (!read_u32(f, n)) return false;
    v.resize(n);
    return n == 0 || fread(v.data(), 1, n, f) == n;
}

static FastInflate g_a, g_b;  // kept across cases, as the reader's thread-local pair is
static int g_fail_lines = 0;

static void fail(const Case &c, const char *what, const char *detail = "") {
    printf("FAIL %s: %s%s\n", c.name.c_str(), what, detail);
    g_fail_lines++;
}

// inflate() with out_len; returns 1 = true and (if check) the right bytes, 0 = false, -1 = true with wrong bytes or a guard hit
static int run_one(const Case &c, size_t out_len, bool check_bytes) {
    Input in(c.raw);
    Guarded g(out_len);
    const bool ok = g_a.inflate(in.p.get(), in.n, g.out(), out_len);
    if (!g.guards_intact()) return -1;
    if (!ok) return 0;
    if (check_bytes && !g.equals(c.payload)) return -1;
    return 1;
}

static bool check_single(const Case &c) {
    bool good = true;
    const int r = run_one(c, c.payload.size(), c.valid);
    if (r < 0) { fail(c, "inflate: wrong bytes or a write outside the output"); good = false; }
    else if (c.valid && r == 0) { fail(c, "inflate refuses a stream zlib inflates"); good = false; }
    else if (!c.valid && r == 1) { fail(c, "inflate takes a stream zlib refuses"); good = false; }
    if (c.valid) {
        if (c.payload.size() > 0 && run_one(c, c.payload.size() - 1, false) != 0) { fail(c, "inflate with out_len one less does not fail cleanly"); good = false; }
        if (run_one(c, c.payload.size() + 1, false) != 0) { fail(c, "inflate with out_len one more does not fail cleanly"); good = false; }
    }
    return good;
}

static bool check_pair(const Case &c, const Case &partner, bool c_is_a, const char *which) {
    const Case &ca = c_is_a ? c : partner, &cb = c_is_a ? partner : c;
    Input ia(ca.raw), ib(cb.raw);
    Guarded ga(ca.payload.size()), gb(cb.payload.size());
    const bool ok = FastInflate::inflate2(g_a, ia.p.get(), ia.n, ga.out(), ga.n, g_b, ib.p.get(), ib.n, gb.out(), gb.n);
    char detail[160];
    snprintf(detail, sizeof detail, " (as stream %c, partner %s: %s)", c_is_a ? 'A' : 'B', which, partner.name.c_str());
    if (!ga.guards_intact() || !gb.guards_intact()) { fail(c, "inflate2 wrote outside an output", detail); return false; }
    const bool want = ca.valid && cb.valid;
    if (ok != want) { fail(c, want ? "inflate2 refuses two valid streams" : "inflate2 takes a pair with an invalid stream", detail); return false; }
    if (ok && (!ga.equals(ca.payload) || !gb.equals(cb.payload))) { fail(c, "inflate2: wrong bytes", detail); return false; }
    return true;
}

// inflate2 with the case's out_len one less / one more (delta), the partner's right: must fail and stay inside both outputs
static bool check_pair_wrong_size(const Case &c, const Case &partner, bool c_is_a, int delta, const char *which) {
    if (delta < 0 && c.payload.empty()) return true;
    Input ic(c.raw), ip(partner.raw);
    Guarded gc(c.payload.size() + delta), gp(partner.payload.size());
    const bool ok = c_is_a ? FastInflate::inflate2(g_a, ic.p.get(), ic.n, gc.out(), gc.n, g_b, ip.p.get(), ip.n, gp.out(), gp.n)
                           : FastInflate::inflate2(g_a, ip.p.get(), ip.n, gp.out(), gp.n, g_b, ic.p.get(), ic.n, gc.out(), gc.n);
    if (ok || !gc.guards_intact() || !gp.guards_intact()) {
        char detail[160];
        snprintf(detail, sizeof detail, " (as stream %c, partner %s)", c_is_a ? 'A' : 'B', which);
        fail(c, delta < 0 ? "inflate2 with out_len one less does not fail cleanly" : "inflate2 with out_len one more does not fail cleanly", detail);
        return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: inflate_corpus corpus.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    uint32_t n;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "FCRP", 4) != 0 || !read_u32(f, n)) { fprintf(stderr, "not a corpus file\n"); return 2; }
    std::vector<Case> cases(n);
    for (auto &c : cases) {
        std::vector<uint8_t> name;
        uint32_t valid;
        if (!read_bytes(f, name) || !read_bytes(f, c.raw) || !read_u32(f, valid) || !read_bytes(f, c.payload)) { fprintf(stderr, "corpus file cut short\n"); return 2; }
        c.name.assign(name.begin(), name.end());
        c.valid = valid != 0;
    }
    fclose(f);
    // the stored-only partner: one final stored block of 100 bytes
    Case stored;
    stored.name = "(stored only)";
    stored.valid = true;
    stored.raw = {0x01, 100, 0, (uint8_t)~100, 0xff};
    for (int i = 0; i < 100; i++) { stored.raw.push_back((uint8_t)(i * 7)); stored.payload.push_back((uint8_t)(i * 7)); }
    size_t failed = 0, n_valid = 0, n_invalid = 0, n_pairs = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        const Case &c = cases[i];
        (c.valid ? n_valid : n_invalid)++;
        bool good = check_single(c);
        const Case &prev = cases[i ? i - 1 : cases.size() - 1];
        for (int as_a = 0; as_a < 2; as_a++) {
            good &= check_pair(c, c, as_a != 0, "itself");
            good &= check_pair(c, prev, as_a != 0, "the previous case");
            good &= check_pair(c, stored, as_a != 0, "stored only");
            n_pairs += 3;
            if (c.valid)
                for (int delta = -1; delta <= 1; delta += 2) {
                    good &= check_pair_wrong_size(c, c, as_a != 0, delta, "itself");
                    good &= check_pair_wrong_size(c, stored, as_a != 0, delta, "stored only");
                }
        }
        if (!good) failed++;
    }
    printf("inflate_corpus: %zu valid and %zu invalid cases, %zu pairs through inflate2: %zu failures\n", n_valid, n_invalid, n_pairs, failed);
    return failed ? 1 : 0;
}
