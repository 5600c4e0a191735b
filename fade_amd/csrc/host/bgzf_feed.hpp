// bgzf_feed.hpp — the input side of the file-path drivers (`fade annotate -b`, `fade out / extract / stats --gpus 1`): a BAM
// file's BGZF members from disk into the buffers of the device stream's calls.  Plain functions over bytes the file gave:
// where the first record lies, the pread that fills a buffer, the members of a buffer (one cut by the end of a read is
// completed in front of the next), the batch that fills a call, its payloads inflated and checked on the pool, a call's
// extract records split.  The threads, queues and buffers are the drivers' own.  Host only (no device header):
// build/bgzf_feed_selftest holds it to zlib and a sequential walk under ASan + UBSan.
#pragma once
#include <unistd.h>

#include "hts_lite.hpp"

namespace htsl {

// ------------------------------------------------------------------ a member's header, read at a file offset
// The 18 bytes a BGZF member starts with when BC is its first extra subfield, and (isize != nullptr) its ISIZE trailer.
// NOT_BGZF: not 1f 8b, FEXTRA unset, or another subfield first — the host reader still takes that, so the drivers fall back.
enum class MemberAt { OK, NO_HEADER, NOT_BGZF, NO_TRAILER };
inline MemberAt bgzf_member_at(int fd, uint64_t at, uint32_t *bsize, uint32_t *isize) {
    uint8_t h[18], t[4];
    if (pread(fd, h, 18, (off_t)at) != 18) return MemberAt::NO_HEADER;
    if (h[0] != 0x1f || h[1] != 0x8b || !(h[3] & 4) || h[12] != 'B' || h[13] != 'C') return MemberAt::NOT_BGZF;
    *bsize = (uint32_t)(h[16] | (h[17] << 8)) + 1u;
    if (!isize) return MemberAt::OK;
    *isize = 0;
    if (pread(fd, t, 4, (off_t)(at + *bsize - 4)) != 4) return MemberAt::NO_TRAILER;
    *isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    return MemberAt::OK;
}

// The member that holds the first record behind hdr_bytes of BAM header, and the record's offset in its payload: offset 0
// of the next member when the header ends with a member, the file's last member (at whatever offset) when no other is left.
// false: a member the function above does not take, or an offset no payload can have.
inline bool locate_first_record(int fd, uint64_t file_size, size_t hdr_bytes, uint64_t *coff, uint32_t *first_rec) {
    uint64_t at = 0, cum = 0;
    for (;;) {
        uint32_t bs, isz;
        if (bgzf_member_at(fd, at, &bs, &isz) != MemberAt::OK) return false;
        if (cum + isz > hdr_bytes || at + bs >= file_size) break;
        cum += isz;
        at += bs;
    }
    if (hdr_bytes - cum > 65536) return false;
    *coff = at;
    *first_rec = (uint32_t)(hdr_bytes - cum);
    return true;
}

// ------------------------------------------------------------------ reading and cutting
// pread into dst until cap bytes are there or the file (or the range: read_end) has no more; *at moves along
inline size_t read_fill(int fd, uint8_t *dst, size_t cap, uint64_t *at, uint64_t read_end, bool *eof, const std::string &path) {
    size_t got = 0;
    while (got < cap) {
        const size_t want = (size_t)std::min<uint64_t>(cap - got, read_end - *at);
        const ssize_t r = want ? pread(fd, dst + got, want, (off_t)*at) : 0;
        if (r < 0) throw std::runtime_error("read error on " + path);
        if (r == 0) { *eof = true; break; }
        got += (size_t)r;
        *at += (uint64_t)r;
    }
    return got;
}

// the members of buf[0, got): (offset, size, header length, ISIZE); stops in front of one that is not whole
struct Mem { size_t off, size, hl; uint32_t isz; };
inline size_t scan_members(const uint8_t *buf, size_t got, std::vector<Mem> &ms, const std::string &path) {
    size_t w = 0;
    ms.clear();
    while (w + 18 <= got) {
        const uint8_t *m = buf + w;
        if (m[0] != 0x1f || m[1] != 0x8b) throw std::runtime_error("not a BGZF member in " + path);
        const size_t xlen = (size_t)m[10] | ((size_t)m[11] << 8);
        if (w + 12 + xlen > got) break;
        size_t bs = 0;
        for (size_t x = 12; x + 4 <= 12 + xlen;) {
            const size_t sl = (size_t)m[x + 2] | ((size_t)m[x + 3] << 8);
            if (m[x] == 'B' && m[x + 1] == 'C' && sl == 2 && x + 6 <= 12 + xlen) bs = ((size_t)m[x + 4] | ((size_t)m[x + 5] << 8)) + 1;
            x += 4 + sl;
        }
        if (bs < 12 + xlen + 10) throw std::runtime_error("BGZF member without a usable BC subfield in " + path);
        if (w + bs > got) break;
        uint32_t isz;
        memcpy(&isz, m + bs - 4, 4);
        if (isz > 65536) throw std::runtime_error("corrupt BGZF block (ISIZE beyond 64 KiB) in " + path);
        ms.push_back(Mem{w, bs, 12 + xlen, isz});
        w += bs;
    }
    return w;
}

// Reads end where they end, members where they end: the bytes behind the last whole member of one read (`tail`) are put in
// front of the next.  base[head, head + n) holds the bytes just read and base[0, head) is free for the tail; the members
// of cb[0, w) are whole, ms has them.
struct MemberCutter {
    std::vector<uint8_t> tail;
    struct Cut { uint8_t *cb; size_t w; };
    Cut cut(uint8_t *base, size_t head, size_t n, bool eof, std::vector<Mem> &ms, const std::string &path) {
        if (tail.size() > head) throw std::runtime_error("BGZF member larger than 64 KiB in " + path);
        uint8_t *cb = base + head - tail.size();
        if (!tail.empty()) memcpy(cb, tail.data(), tail.size());
        const size_t got = tail.size() + n;
        const size_t w = scan_members(cb, got, ms, path);
        tail.assign(cb + w, cb + got);
        if (eof && !tail.empty()) throw std::runtime_error("the file ends inside a BGZF member: " + path);
        return Cut{cb, w};
    }
};

// ------------------------------------------------------------------ a call's worth of members, inflated on the pool
// members from m0 on until their payloads fill `chunk` bytes: [m0, m1), *total the payloads' bytes
inline size_t take_batch(const std::vector<Mem> &ms, size_t m0, size_t chunk, size_t *total) {
    size_t m1 = m0;
    *total = 0;
    while (m1 < ms.size() && *total + ms[m1].isz <= chunk) *total += ms[m1++].isz;
    return m1;
}

// The payloads of members [m0, m1) of cb, one behind the other at dst, two members to a task (FastInflate::inflate2).  false:
// a stream is not ISIZE bytes long, its CRC32 (RFC 1952 trailer, as htslib checks it) is another, or an empty member is not one.
inline bool inflate_batch(Pool &pool, const uint8_t *cb, const std::vector<Mem> &ms, size_t m0, size_t m1, uint8_t *dst) {
    std::vector<size_t> ooff(m1 - m0 + 1, 0);
    for (size_t j = m0; j < m1; j++) ooff[j - m0 + 1] = ooff[j - m0] + ms[j].isz;
    std::atomic<bool> bad{false};
    pool.parallel_for((m1 - m0 + 1) / 2, [&](size_t t) {
        static thread_local std::unique_ptr<FastInflate> fi[2];
        if (!fi[0]) { fi[0].reset(new FastInflate()); fi[1].reset(new FastInflate()); }
        const uint8_t *src[2] = {nullptr, nullptr};
        size_t slen[2] = {0, 0}, jj[2] = {0, 0};
        int n = 0;
        for (size_t j = m0 + 2 * t; j < std::min(m1, m0 + 2 * t + 2); j++) {
            if (ms[j].isz == 0) {
                if (ms[j].size < ms[j].hl + 8 || !bgzf_empty_member_ok(cb + ms[j].off + ms[j].hl, ms[j].size - ms[j].hl - 8, cb + ms[j].off + ms[j].size - 8)) bad = true;
                continue;
            }
            src[n] = cb + ms[j].off + ms[j].hl;
            slen[n] = ms[j].size - ms[j].hl - 8;
            jj[n++] = j;
        }
        if (n == 2 && !FastInflate::inflate2(*fi[0], src[0], slen[0], dst + ooff[jj[0] - m0], ms[jj[0]].isz, *fi[1], src[1], slen[1], dst + ooff[jj[1] - m0], ms[jj[1]].isz)) bad = true;
        if (n == 1 && !fi[0]->inflate(src[0], slen[0], dst + ooff[jj[0] - m0], ms[jj[0]].isz)) bad = true;
        for (int q = 0; q < n; q++) {
            uint32_t crc;
            memcpy(&crc, cb + ms[jj[q]].off + ms[jj[q]].size - 8, 4);
            if (crc32_fast(0, dst + ooff[jj[q] - m0], ms[jj[q]].isz) != crc) bad = true;
        }
    }, CPU_INFLATE);
    return !bad;
}

// ------------------------------------------------------------------ a call's extract records
// xp[0, xn): uint32 block_size and record, one behind the other, as the device leaves them
inline void split_extract_records(const uint8_t *xp, size_t xn, std::vector<Rec> &xrecs) {
    xrecs.clear();
    for (size_t at = 0; at + 4 <= xn;) {
        uint32_t bs;
        memcpy(&bs, xp + at, 4);
        if (bs < 32 || at + 4 + bs > xn) throw std::runtime_error("the device's extract records are not whole");
        xrecs.emplace_back();
        xrecs.back().d.assign(xp + at + 4, xp + at + 4 + bs);
        at += 4 + (size_t)bs;
    }
}

}  // namespace htsl
