// bgzf_feed_selftest — host/bgzf_feed.hpp, the file-path drivers' input side, on small BGZF files built here with zlib's
// deflate (CPU only; the Makefile builds it with ASan + UBSan).  The arbiter is walk() below: one member after the other,
// zlib's inflate and crc32.  Every buffer the feeder writes into has exactly the size the drivers promise it, so a byte
// too many is the sanitizer's.
#include "../bgzf_feed.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace htsl;
typedef std::vector<uint8_t> Bytes;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                 \
        }                                                            \
    } while (0)

// ------------------------------------------------------------------ building members
static Bytes payload(size_t n, unsigned seed) {  // (half text-like, half noise: Huffman blocks with matches and literals)
    Bytes p(n);
    for (size_t i = 0; i < n; i++) p[i] = (i & 8) ? (uint8_t)("ACGT"[(i * 7 + seed) & 3]) : (uint8_t)((i * 2654435761u + seed * 40503u) >> 13);
    return p;
}
static Bytes raw_deflate(const Bytes &p) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    Bytes out(deflateBound(&zs, (uLong)p.size()) + 16);
    uint8_t none = 0;
    zs.next_in = p.empty() ? &none : const_cast<uint8_t *>(p.data());
    zs.avail_in = (uInt)p.size();
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}
static void put16(Bytes &b, size_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffff); put16(b, v >> 16); }
// a member around p; `before` / `behind`: another extra subfield ('X','Y', three bytes) in front of / behind BC
static Bytes member(const Bytes &p, bool before = false, bool behind = false) {
    const Bytes z = raw_deflate(p);
    const size_t xlen = 6 + (before ? 7 : 0) + (behind ? 7 : 0), bs = 12 + xlen + z.size() + 8;
    Bytes m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
    put16(m, xlen);
    const Bytes other = {'X', 'Y', 3, 0, 1, 2, 3};
    if (before) m.insert(m.end(), other.begin(), other.end());
    m.insert(m.end(), {'B', 'C', 2, 0});
    put16(m, bs - 1);
    if (behind) m.insert(m.end(), other.begin(), other.end());
    m.insert(m.end(), z.begin(), z.end());
    put32(m, (uint32_t)crc32(crc32(0, nullptr, 0), p.empty() ? nullptr : p.data(), (uInt)p.size()));
    put32(m, (uint32_t)p.size());
    return m;
}
static const Bytes EOF_MARKER = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static Bytes cat(const std::vector<Bytes> &parts) {
    Bytes all;
    for (const Bytes &p : parts) all.insert(all.end(), p.begin(), p.end());
    return all;
}

struct TmpFile {  // the bytes as a file: the feeder reads with pread
    FILE *f;
    explicit TmpFile(const Bytes &b) : f(tmpfile()) {
        if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size()) || fflush(f) != 0) abort();
    }
    ~TmpFile() { fclose(f); }
    int fd() const { return fileno(f); }
};

// ------------------------------------------------------------------ the arbiter: a sequential walk with zlib
struct Walked { std::vector<Mem> ms; Bytes data; bool ok = true; };  // (Mem::off: file offsets here)
static bool zlib_member_ok(const uint8_t *z, size_t zn, uint32_t isz, uint32_t crc, Bytes &out) {
    Bytes buf(isz + 1);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) abort();
    zs.next_in = const_cast<uint8_t *>(z);
    zs.avail_in = (uInt)zn;
    zs.next_out = buf.data();
    zs.avail_out = (uInt)buf.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == isz && (uint32_t)crc32(crc32(0, nullptr, 0), buf.data(), isz) == crc;
    inflateEnd(&zs);
    if (ok) out.insert(out.end(), buf.begin(), buf.begin() + isz);
    return ok;
}
static Walked walk(const Bytes &file) {
    Walked r;
    for (size_t at = 0; at < file.size();) {
        const uint8_t *m = file.data() + at;
        if (file.size() - at < 18 || m[0] != 0x1f || m[1] != 0x8b || !(m[3] & 4)) abort();  // (the sweep's files are whole)
        const size_t xlen = m[10] + 256u * m[11];
        size_t bs = 0;
        for (size_t x = 12; x < 12 + xlen; x += 4 + m[x + 2] + 256u * m[x + 3])
            if (m[x] == 'B' && m[x + 1] == 'C') bs = m[x + 4] + 256u * m[x + 5] + 1;
        if (!bs || at + bs > file.size()) abort();
        uint32_t crc, isz;
        memcpy(&crc, m + bs - 8, 4);
        memcpy(&isz, m + bs - 4, 4);
        r.ms.push_back(Mem{at, bs, 12 + xlen, isz});
        if (!zlib_member_ok(m + 12 + xlen, bs - 12 - xlen - 8, isz, crc, r.data)) r.ok = false;
        at += bs;
    }
    return r;
}

// ------------------------------------------------------------------ the feeder, driven as the drivers drive it
struct Fed {
    std::vector<Mem> ms;  // (off: file offsets)
    Bytes data;
    std::vector<int> last;  // per batch
    std::string err;        // an exception's text, or "inflate" where inflate_batch said no
};
enum Batches { BY_CHUNK, ONE_EACH };  // ONE_EACH: the harness hands inflate_batch one member at a time
static const std::string PATH = "in.bam";
static Fed feed(const Bytes &file, size_t ccap, size_t chunk, Batches how = BY_CHUNK, size_t head = 65536 + 64, uint64_t read_end = UINT64_MAX) {
    static Pool pool(3);
    Fed r;
    TmpFile tf(file);
    Bytes base(head + ccap);
    MemberCutter cutter;
    std::vector<Mem> ms;
    uint64_t at = 0;
    bool eof = false;
    try {
        while (!eof) {
            const uint64_t cb_off = at - cutter.tail.size();
            const size_t got = read_fill(tf.fd(), base.data() + head, ccap, &at, read_end, &eof, PATH);
            CHECK(got <= ccap && (got == ccap || eof));
            const MemberCutter::Cut cut = cutter.cut(base.data(), head, got, eof, ms, PATH);
            CHECK(cut.cb + cut.w + cutter.tail.size() == base.data() + head + got);
            for (const Mem &m : ms) r.ms.push_back(Mem{(size_t)cb_off + m.off, m.size, m.hl, m.isz});
            size_t m0 = 0;
            do {
                size_t total = 0, m1 = take_batch(ms, m0, chunk, &total);
                if (how == BY_CHUNK) {  // as many members as fit, and not one more
                    size_t sum = 0;
                    for (size_t j = m0; j < m1; j++) sum += ms[j].isz;
                    CHECK(sum == total && total <= chunk && (m1 == ms.size() || total + ms[m1].isz > chunk));
                } else if (m0 < ms.size()) {
                    m1 = m0 + 1;
                    total = ms[m0].isz;
                }
                Bytes dst(total);
                if (!inflate_batch(pool, cut.cb, ms, m0, m1, dst.data())) { r.err = "inflate"; return r; }
                r.data.insert(r.data.end(), dst.begin(), dst.end());
                r.last.push_back(eof && m1 == ms.size());
                m0 = m1;
            } while (m0 < ms.size());
        }
    } catch (const std::exception &e) {
        r.err = e.what();
    }
    return r;
}
static bool same(const std::vector<Mem> &a, const std::vector<Mem> &b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k].off != b[k].off || a[k].size != b[k].size || a[k].hl != b[k].hl || a[k].isz != b[k].isz) return false;
    return true;
}
static bool only_the_last_is_last(const std::vector<int> &last) {
    if (last.empty() || !last.back()) return false;
    for (size_t k = 0; k + 1 < last.size(); k++)
        if (last[k]) return false;
    return true;
}
// the read sizes a refusal is shown at: byte by byte, an odd size, everything at once
static std::vector<size_t> some_ccaps(const Bytes &file) { return {1, 13, file.size() + 1}; }
static void refused(const Bytes &file, const std::string &text, int line) {
    for (size_t ccap : some_ccaps(file)) {
        const Fed r = feed(file, ccap, 1 << 20);
        if (r.err != text) { fprintf(stderr, "line %d, ccap %zu: \"%s\" in the place of \"%s\"\n", line, ccap, r.err.c_str(), text.c_str()); fails++; }
    }
}
#define REFUSED(file, text) refused(file, text, __LINE__)

static void cut_sweep() {
    // six members and the end-of-file marker: an empty one in the middle, one with a subfield behind BC, one with a subfield in front
    const Bytes file = cat({member(payload(300, 1)), member(payload(290, 2)), member(Bytes()), member(payload(150, 3), false, true),
                            member(payload(160, 4), true, false), member(payload(1, 5)), EOF_MARKER});
    const Walked w = walk(file);
    CHECK(w.ok && w.ms.size() == 7 && w.data.size() == 300 + 290 + 150 + 160 + 1);
    // chunk 300: [300] [290, 0] [150] [160, 1, 0] where a read holds them all — single members, a pair with an empty one, three;
    // one batch for everything; and every member a batch of its own (an empty member always fits the batch in front of it,
    // so take_batch alone never gives that)
    const struct { size_t chunk; Batches how; } modes[] = {{300, BY_CHUNK}, {1 << 20, BY_CHUNK}, {300, ONE_EACH}};
    for (const auto &mode : modes)
        for (size_t ccap = 1; ccap <= file.size() + 1; ccap++) {
            const Fed r = feed(file, ccap, mode.chunk, mode.how);
            if (!r.err.empty() || r.data != w.data || !same(r.ms, w.ms) || !only_the_last_is_last(r.last)) {
                fprintf(stderr, "cut sweep: chunk %zu, mode %d, ccap %zu: %s\n", mode.chunk, (int)mode.how, ccap, r.err.empty() ? "differs from the walk" : r.err.c_str());
                fails++;
            }
        }
    {  // everything in one read: the batches are the ones named above
        CHECK(feed(file, file.size() + 1, 300).last == std::vector<int>({0, 0, 0, 1}));
        CHECK(feed(file, file.size() + 1, 1 << 20).last == std::vector<int>({1}));
        // (a read that is filled to its last byte has not seen the end of the file: the next one does, and brings an empty last batch)
        CHECK(feed(file, file.size(), 1 << 20).last == std::vector<int>({0, 1}));
    }
    {  // a range that ends in front of the fourth member (a lane's read_end): the first three, and the last batch is last
        const Fed r = feed(file, 64, 300, BY_CHUNK, 65536 + 64, w.ms[3].off);
        CHECK(r.err.empty() && r.ms.size() == 3 && r.data == Bytes(w.data.begin(), w.data.begin() + 590) && only_the_last_is_last(r.last));
    }
    // the carry has `head` bytes: a member that does not fit them is refused, one that just fits is not
    CHECK(feed(file, 10, 1 << 20, BY_CHUNK, 64).err == "BGZF member larger than 64 KiB in " + PATH);
    size_t longest = 0;
    for (const Mem &m : w.ms) longest = std::max(longest, m.size);
    CHECK(feed(file, 1, 1 << 20, BY_CHUNK, longest - 1).err.empty());
    CHECK(feed(file, 1, 1 << 20, BY_CHUNK, longest - 2).err == "BGZF member larger than 64 KiB in " + PATH);
}

static void member_headers_and_first_record() {
    const Bytes h1 = member(payload(100, 6)), h2 = member(payload(50, 7)), r3 = member(payload(80, 8)), r4 = member(payload(60, 9));
    const Bytes file = cat({h1, h2, r3, r4, EOF_MARKER});
    const Walked w = walk(file);
    TmpFile tf(file);
    for (const Mem &m : w.ms) {
        uint32_t bs = 0, isz = 99;
        CHECK(bgzf_member_at(tf.fd(), m.off, &bs, &isz) == MemberAt::OK && bs == m.size && isz == m.isz);
    }
    uint32_t bs = 0, isz = 0;
    CHECK(bgzf_member_at(tf.fd(), file.size(), &bs, &isz) == MemberAt::NO_HEADER);
    CHECK(bgzf_member_at(tf.fd(), file.size() - 17, &bs, &isz) == MemberAt::NO_HEADER);
    CHECK(bgzf_member_at(tf.fd(), 1, &bs, &isz) == MemberAt::NOT_BGZF);
    uint64_t coff = 99;
    uint32_t first = 99;
    // the header ends exactly where the first member ends: the record is at offset 0 of the second member
    CHECK(locate_first_record(tf.fd(), file.size(), 100, &coff, &first) && coff == w.ms[1].off && first == 0);
    CHECK(locate_first_record(tf.fd(), file.size(), 40, &coff, &first) && coff == 0 && first == 40);
    CHECK(locate_first_record(tf.fd(), file.size(), 170, &coff, &first) && coff == w.ms[2].off && first == 20);
    CHECK(locate_first_record(tf.fd(), file.size(), 0, &coff, &first) && coff == 0 && first == 0);
    {  // header members only: the walk stops at the file's last member, the record would start behind its payload
        const Bytes only = cat({h1, h2});
        TmpFile t2(only);
        CHECK(locate_first_record(t2.fd(), only.size(), 150, &coff, &first) && coff == h1.size() && first == 50);
        CHECK(!locate_first_record(t2.fd(), only.size(), 100 + 65537, &coff, &first));  // (no payload has that offset)
        CHECK(locate_first_record(t2.fd(), only.size(), 100 + 65536, &coff, &first) && coff == h1.size() && first == 65536);
        const Bytes marked = cat({h1, h2, EOF_MARKER});
        TmpFile t3(marked);
        CHECK(locate_first_record(t3.fd(), marked.size(), 150, &coff, &first) && coff == h1.size() + h2.size() && first == 0);
    }
    {  // what the 18-byte read does not take: another subfield first, no FEXTRA, no magic; and files that end too early
        const Bytes other_first = cat({member(payload(100, 6), true, false), h2, EOF_MARKER});
        TmpFile t2(other_first);
        CHECK(bgzf_member_at(t2.fd(), 0, &bs, &isz) == MemberAt::NOT_BGZF && !locate_first_record(t2.fd(), other_first.size(), 40, &coff, &first));
        Bytes bad = file;
        bad[3] = 0;
        TmpFile t3(bad);
        CHECK(bgzf_member_at(t3.fd(), 0, &bs, &isz) == MemberAt::NOT_BGZF && !locate_first_record(t3.fd(), bad.size(), 40, &coff, &first));
        bad = file;
        bad[1] = 0x8c;
        TmpFile t4(bad);
        CHECK(bgzf_member_at(t4.fd(), 0, &bs, &isz) == MemberAt::NOT_BGZF && !locate_first_record(t4.fd(), bad.size(), 40, &coff, &first));
        for (size_t n : {(size_t)0, (size_t)17}) {
            const Bytes shorter(file.begin(), file.begin() + n);
            TmpFile t5(shorter);
            CHECK(bgzf_member_at(t5.fd(), 0, &bs, &isz) == MemberAt::NO_HEADER && !locate_first_record(t5.fd(), n, 40, &coff, &first));
        }
        const Bytes no_trailer(file.begin(), file.begin() + h1.size() - 1);  // the first member's ISIZE is not all there
        TmpFile t6(no_trailer);
        CHECK(bgzf_member_at(t6.fd(), 0, &bs, &isz) == MemberAt::NO_TRAILER && bs == h1.size() && isz == 0);
        CHECK(bgzf_member_at(t6.fd(), 0, &bs, nullptr) == MemberAt::OK && bs == h1.size());  // (not asked for: not read)
        CHECK(!locate_first_record(t6.fd(), no_trailer.size(), 40, &coff, &first));
    }
}

static void refusals() {
    const Bytes a = member(payload(200, 10)), b = member(payload(120, 11)), c = member(payload(90, 12));
    const Bytes file = cat({a, b, c, EOF_MARKER});
    const size_t bo = a.size();  // where b starts
    REFUSED(file, "");           // (the file itself is taken)
    Bytes f = file;
    f[bo] = 0x1e;
    REFUSED(f, "not a BGZF member in " + PATH);
    f = file;
    f[bo + 12] = 'X';  // the only subfield is not BC
    REFUSED(f, "BGZF member without a usable BC subfield in " + PATH);
    f = file;
    f[bo + 14] = 3;  // BC with a length that is not 2 (the walk then steps one byte too far and ends)
    REFUSED(f, "BGZF member without a usable BC subfield in " + PATH);
    f = file;
    f[bo + 10] = 5;  // xlen cuts BC's value off
    REFUSED(f, "BGZF member without a usable BC subfield in " + PATH);
    f = file;
    f[bo + 16] = 12 + 6 + 9 - 1;  // BSIZE: one byte less than a header, an empty stored block's two bytes and the trailer
    f[bo + 17] = 0;
    REFUSED(f, "BGZF member without a usable BC subfield in " + PATH);
    f = file;
    f[bo + b.size() - 4] = 1, f[bo + b.size() - 3] = 0, f[bo + b.size() - 2] = 1, f[bo + b.size() - 1] = 0;  // ISIZE 65537
    REFUSED(f, "corrupt BGZF block (ISIZE beyond 64 KiB) in " + PATH);
    f[bo + b.size() - 4] = 0;  // ISIZE 65536 is a size a block may claim: this one does not inflate to it
    REFUSED(f, "inflate");
    // a file that ends inside b: in its 18-byte header after 1, 2, ... 17 bytes — all seventeen are fewer than the scan looks
    // at, whatever they hold — and in its body
    for (size_t k = 1; k <= 17; k++) {
        REFUSED(Bytes(file.begin(), file.begin() + bo + k), "the file ends inside a BGZF member: " + PATH);
        Bytes junk(file.begin(), file.begin() + bo + k);
        for (size_t i = bo; i < junk.size(); i++) junk[i] = 0xff;
        REFUSED(junk, "the file ends inside a BGZF member: " + PATH);
    }
    REFUSED(Bytes(file.begin(), file.begin() + bo), "");  // (between two members: nothing is missing that the feeder could know of)
    for (size_t k : {(size_t)18, (size_t)19, b.size() / 2, b.size() - 8, b.size() - 1}) REFUSED(Bytes(file.begin(), file.begin() + bo + k), "the file ends inside a BGZF member: " + PATH);
    f = Bytes(file.begin(), file.begin() + bo + 40);  // xlen claims more than the file holds
    f[bo + 10] = 0xff, f[bo + 11] = 0xff;
    REFUSED(f, "the file ends inside a BGZF member: " + PATH);
    f = file;  // xlen larger than the subfields are: BC is found as before, the stream is taken to start 14 bytes late
    f[bo + 10] = 20;
    REFUSED(f, "inflate");
    // bits: every single one of b's DEFLATE stream and CRC32 flipped in turn; the verdict is zlib's (a flip in the stream's
    // last padding bits changes nothing, and both say so)
    const Walked whole = walk(file);
    size_t caught = 0;
    for (size_t bit = 8 * 18; bit < 8 * (b.size() - 4); bit++) {
        f = file;
        f[bo + bit / 8] ^= (uint8_t)(1u << (bit % 8));
        const bool zlib_ok = walk(f).ok;
        const Fed r = feed(f, f.size() + 1, 1 << 20);
        if ((r.err == "inflate") == zlib_ok || (zlib_ok && r.data != whole.data)) { fprintf(stderr, "bit %zu of the second member: zlib says %d, the feeder \"%s\"\n", bit, (int)zlib_ok, r.err.c_str()); fails++; }
        caught += !zlib_ok;
        if (bit >= 8 * (b.size() - 8)) CHECK(!zlib_ok);  // the CRC32's bits, all of them
    }
    CHECK(caught >= 8 * (b.size() - 22) - 8);  // (all but padding bits)
    f = file;
    f[bo + 18 + 10] ^= 0x10;  // the pinned ones: a bit of the stream, a bit of the CRC32, byte by byte as well
    REFUSED(f, "inflate");
    f = file;
    f[bo + b.size() - 7] ^= 0x01;
    REFUSED(f, "inflate");
    f = file;  // ISIZE 0 over a stream that is not empty: with its own CRC32, and with the CRC32 of no bytes
    memset(&f[bo + b.size() - 4], 0, 4);
    REFUSED(f, "inflate");
    memset(&f[bo + b.size() - 8], 0, 8);
    REFUSED(f, "inflate");
    f = cat({a, member(Bytes()), c});  // an empty member whose CRC32 field is not zero
    f[bo + 28 - 8] = 1;
    REFUSED(f, "inflate");
}

static void extract_records() {
    std::vector<Rec> recs(3);
    Bytes x;
    put32(x, 32);
    for (int i = 0; i < 32; i++) x.push_back((uint8_t)i);
    put32(x, 40);
    for (int i = 0; i < 40; i++) x.push_back((uint8_t)(100 + i));
    split_extract_records(x.data(), x.size(), recs);
    CHECK(recs.size() == 2 && recs[0].d == Bytes(x.begin() + 4, x.begin() + 36) && recs[1].d == Bytes(x.begin() + 40, x.end()));
    split_extract_records(nullptr, 0, recs);
    CHECK(recs.empty());
    auto refuses = [&](const Bytes &in) {
        try {
            split_extract_records(in.data(), in.size(), recs);
        } catch (const std::exception &e) {
            return std::string(e.what()) == "the device's extract records are not whole";
        }
        return false;
    };
    CHECK(refuses(Bytes(x.begin(), x.end() - 1)));  // the last record one byte short
    Bytes small;
    put32(small, 31);
    small.resize(4 + 31);
    CHECK(refuses(small));
    Bytes huge = x;
    put32(huge, 0xffffffffu);  // (a size no sum may wrap around on)
    CHECK(refuses(huge));
}

int main() {
    cut_sweep();
    member_headers_and_first_record();
    refusals();
    extract_records();
    if (fails) return 1;
    puts("bgzf_feed_selftest ok");
    return 0;
}
