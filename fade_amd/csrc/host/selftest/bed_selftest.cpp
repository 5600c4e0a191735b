// bed_selftest — host/bed_lite.hpp on hand-written BED files: every rule of its header, every error with its line, and every
// file fed whole, byte by byte and split at every single position, always with the same result (CPU only; the Makefile
// builds it with ASan + UBSan).  With a path argument: that file parsed in reads of 4096 bytes, its names and intervals
// printed ("N name" lines, then "I chrom start end"), or "ERR message" — what tests/test_bed_selftest.py compares.
#include "../bed_lite.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

using namespace fadehip::bed;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                 \
        }                                                            \
    } while (0)

typedef std::tuple<int32_t, int64_t, int64_t> Iv;
struct Result {
    bool ok = false;
    std::string err;
    std::vector<std::string> names;
    std::vector<Iv> ivs;
    size_t max_piece = 0, pieces = 0;
    bool names_ahead = true;  // every piece's chrom ids were below names().size() when the sink saw it
    // (of a parse that fails, how many whole pieces the sink saw before depends on the piece size: the error alone counts)
    bool operator==(const Result &o) const { return ok == o.ok && err == o.err && (!ok || (names == o.names && ivs == o.ivs)); }
};

// the text in the parts [0, cuts[0]), [cuts[0], cuts[1]), ...
static Result parse(const std::string &text, const std::vector<size_t> &cuts, size_t piece) {
    Result r;
    Parser *self = nullptr;
    Parser p([&](const int32_t *c, const int64_t *s, const int64_t *e, size_t n, std::string &) {
        for (size_t k = 0; k < n; k++) {
            r.ivs.emplace_back(c[k], s[k], e[k]);
            if ((size_t)c[k] >= self->names().size()) r.names_ahead = false;
        }
        r.max_piece = std::max(r.max_piece, n);
        r.pieces++;
        return true;
    }, piece);
    self = &p;
    size_t at = 0;
    bool ok = true;
    for (size_t c : cuts) {
        ok = ok && p.feed(text.data() + at, c - at);
        at = c;
    }
    ok = ok && p.feed(text.data() + at, text.size() - at);
    ok = p.finish() && ok;
    r.ok = ok;
    r.err = p.error();
    r.names = p.names();
    return r;
}

// whole, byte by byte, and split at every single position: one result
static Result every_way(const std::string &text, size_t piece = 3) {
    const Result whole = parse(text, {}, piece);
    std::vector<size_t> all;
    for (size_t k = 1; k < text.size(); k++) all.push_back(k);
    CHECK(parse(text, all, piece) == whole);
    for (size_t k = 0; k <= text.size(); k++) CHECK(parse(text, {k}, piece) == whole);
    CHECK(parse(text, {}, 1) == whole);
    CHECK(parse(text, {}, 1000000) == whole);
    CHECK(whole.names_ahead && whole.max_piece <= piece);
    return whole;
}

static void good(const std::string &text, const std::vector<std::string> &names, const std::vector<Iv> &ivs) {
    const Result r = every_way(text);
    CHECK(r.ok && r.err.empty());
    CHECK(r.names == names);
    CHECK(r.ivs == ivs);
    if (!(r.ok && r.names == names && r.ivs == ivs)) fprintf(stderr, "  in: %s (%s)\n", text.c_str(), r.err.c_str());
}

static void bad(const std::string &text, const std::string &err) {
    const Result r = every_way(text);
    CHECK(!r.ok);
    CHECK(r.err == err);
    if (r.ok || r.err != err) fprintf(stderr, "  in: %s\n  got: %s\n  want: %s\n", text.c_str(), r.err.c_str(), err.c_str());
}

static int print_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        printf("ERR cannot open %s\n", path);
        return 0;
    }
    std::vector<Iv> ivs;
    Parser p([&](const int32_t *c, const int64_t *s, const int64_t *e, size_t n, std::string &) {
        for (size_t k = 0; k < n; k++) ivs.emplace_back(c[k], s[k], e[k]);
        return true;
    });
    char buf[4096];
    size_t n;
    bool ok = true;
    while (ok && (n = fread(buf, 1, sizeof buf, f)) > 0) ok = p.feed(buf, n);
    fclose(f);
    ok = ok && p.finish();
    if (!ok) {
        printf("ERR %s\n", p.error().c_str());
        return 0;
    }
    for (const std::string &nm : p.names()) printf("N %s\n", nm.c_str());
    for (const Iv &v : ivs) printf("I %d %lld %lld\n", std::get<0>(v), (long long)std::get<1>(v), (long long)std::get<2>(v));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return print_file(argv[1]);
    // lines, '\r', a last line without its '\n'
    good("", {}, {});
    good("\n\n", {}, {});
    good("chr1\t0\t1\n", {"chr1"}, {Iv{0, 0, 1}});
    good("chr1\t0\t1", {"chr1"}, {Iv{0, 0, 1}});
    good("chr1\t5\t10\r\nchr2\t7\t9\r\n", {"chr1", "chr2"}, {Iv{0, 5, 10}, Iv{1, 7, 9}});
    good("chr1\t5\t10\r", {"chr1"}, {Iv{0, 5, 10}});
    good("\r\nchr1\t5\t10\n\r\n", {"chr1"}, {Iv{0, 5, 10}});
    // skipped lines
    good("#chrom\tstart\tend\ntrack name=rmsk\nbrowser position chr1:1-2\n\nchr1\t5\t10\n#\n", {"chr1"}, {Iv{0, 5, 10}});
    good("tracks\tare\tskipped\nbrowserX\t1\t2\nchr1\t5\t10\n", {"chr1"}, {Iv{0, 5, 10}});
    good("trac\t1\t2\nbrowse\t3\t4\n", {"trac", "browse"}, {Iv{0, 1, 2}, Iv{1, 3, 4}});
    // further fields are ignored, whatever they hold; names as they stand, ids in order of first appearance
    good("chr1\t5\t10\tAluY\t0\t+\nchr1\t5\t10\t\nchr1\t1\t2\t\t\t\n", {"chr1"}, {Iv{0, 5, 10}, Iv{0, 5, 10}, Iv{0, 1, 2}});
    good("b\t1\t2\na\t1\t2\nb\t3\t4\nchr 1\t1\t2\n a\t1\t2\n", {"b", "a", "chr 1", " a"}, {Iv{0, 1, 2}, Iv{1, 1, 2}, Iv{0, 3, 4}, Iv{2, 1, 2}, Iv{3, 1, 2}});
    good("c\t007\t0010\n", {"c"}, {Iv{0, 7, 10}});
    // the bounds
    good("c\t0\t2147483647\nc\t2147483646\t2147483647\n", {"c"}, {Iv{0, 0, 2147483647}, Iv{0, 2147483646, 2147483647}});
    bad("c\t0\t2147483648\n", "line 1: end is beyond 2^31 - 1");
    bad("c\t0\t99999999999999999999999999\n", "line 1: end is beyond 2^31 - 1");
    bad("c\t1\t2\nc\t5\t5\n", "line 2: start is not below end");
    bad("c\t1\t2\n\nc\t6\t5\n", "line 3: start is not below end");
    bad("c\t99999999999999999999\t5\n", "line 1: start is not below end");
    // the name
    const std::string n255(255, 'n'), n256(256, 'n');
    good(n255 + "\t1\t2\n", {n255}, {Iv{0, 1, 2}});
    bad(n256 + "\t1\t2\n", "line 1: the name is longer than 255 bytes");
    bad("c\t1\t2\n\t1\t2\n", "line 2: the name is empty");
    // the numbers: decimal digits only
    bad("c\t-1\t2\n", "line 1: start is not a number of decimal digits");
    bad("c\t+1\t2\n", "line 1: start is not a number of decimal digits");
    bad("c\t\t2\n", "line 1: start is not a number of decimal digits");
    bad("c\t1 \t2\n", "line 1: start is not a number of decimal digits");
    bad("c\t1\t2x\n", "line 1: end is not a number of decimal digits");
    bad("c\t1\t\n", "line 1: end is not a number of decimal digits");
    bad("c\t1\t2 \n", "line 1: end is not a number of decimal digits");
    bad("c\t1\t1e3\n", "line 1: end is not a number of decimal digits");
    bad("#x\nc\t1\t2\r\r\n", "line 2: end is not a number of decimal digits");  // (only the '\r' in front of '\n' is dropped)
    bad("c\t1\r\t2\n", "line 1: start is not a number of decimal digits");
    // the fields
    bad("c\t1\n", "line 1: fewer than three tab-separated fields");
    bad("c 1 2\n", "line 1: fewer than three tab-separated fields");
    bad("c\t1\t2\nchr1", "line 2: fewer than three tab-separated fields");
    bad("c\t1\t2\n\n#\nx\n", "line 4: fewer than three tab-separated fields");
    // an error stops the parse: what follows is not looked at
    bad("c\t1\t2\nc\t2\t1\nc\tx\ty\n", "line 2: start is not below end");
    // long lines: only the first KEEP bytes are held
    good("c\t1\t2\t" + std::string(3 * KEEP, 'x') + "\nd\t3\t4\n", {"c", "d"}, {Iv{0, 1, 2}, Iv{1, 3, 4}});
    good("#" + std::string(2 * KEEP, '#') + "\nc\t1\t2\n", {"c"}, {Iv{0, 1, 2}});
    for (size_t pad : {KEEP - 7, KEEP - 6, KEEP - 5}) {  // the third field ends before and at the last held byte (pad + 5 bytes)
        const std::string z(pad - n255.size(), '0');
        good(n255 + "\t" + z + "1\t22\n", {n255}, {Iv{0, 1, 22}});
        good(n255 + "\t" + z + "1\t22\r\n", {n255}, {Iv{0, 1, 22}});
        good(n255 + "\t" + z + "1\t22\tmore\r\n", {n255}, {Iv{0, 1, 22}});
        good(n255 + "\t" + z + "1\t22\t\r", {n255}, {Iv{0, 1, 22}});
    }
    {  // ... and one byte behind it
        const std::string z(KEEP - 4 - n255.size(), '0');
        bad(n255 + "\t" + z + "1\t22\n", "line 1: the first three fields take more than 512 bytes");
        bad("x\t1\t2\n" + n255 + "\t" + z + "1\t22\tmore\r\n", "line 2: the first three fields take more than 512 bytes");
    }
    bad("c\t1\t" + std::string(KEEP, '0') + "2\n", "line 1: the first three fields take more than 512 bytes");
    bad("c\t" + std::string(KEEP, '0') + "1\t2\n", "line 1: the first three fields take more than 512 bytes");
    // the pieces: bounded, in order
    {
        std::string text;
        std::vector<Iv> want;
        for (int k = 0; k < 10; k++) {
            text += "c" + std::to_string(k % 3) + "\t" + std::to_string(k) + "\t" + std::to_string(k + 5) + "\n";
            want.emplace_back(k % 3, k, k + 5);
        }
        good(text, {"c0", "c1", "c2"}, want);
        const Result r = parse(text, {}, 4);
        CHECK(r.pieces == 3 && r.max_piece == 4);
    }
    // a sink that refuses stops the parse with its message
    {
        Parser p([](const int32_t *, const int64_t *, const int64_t *, size_t, std::string &why) {
            why = "the sink said no";
            return false;
        }, 2);
        const std::string text = "c\t1\t2\nc\t3\t4\nc\t5\t6\n";
        CHECK(!p.feed(text.data(), text.size()) && p.error() == "the sink said no");
        CHECK(!p.finish() && !p.feed("x", 1));
    }
    // compressed files are refused by name
    CHECK(path_refusal("rmsk.bed").empty() && path_refusal("gz").empty() && path_refusal("a.gz.bed").empty());
    CHECK(path_refusal("rmsk.bed.gz").find("rmsk.bed.gz") != std::string::npos && !path_refusal("x.bgz").empty() && !path_refusal(".gz").empty());
    if (fails) return 1;
    puts("bed_selftest ok");
    return 0;
}
