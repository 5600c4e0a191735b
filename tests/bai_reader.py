"""What a reader of an indexed BAM does, for the tests of --write-index: BGZF members walked with zlib and the BC subfield,
every record's virtual offsets derived from where its bytes lie, and region queries answered by seeking into the file's real
bytes through a .bai (bai_model.query) — held against brute force over all records."""
import bisect
import random
import struct
import zlib

import bai_model as bm


def walk_members(data, base=0):
    """[(file offset, payload)] of a BGZF byte string that begins at file offset `base`."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", at
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        payload = zlib.decompress(data[at + 18:at + bsize - 8], -15)
        assert len(payload) == struct.unpack_from("<I", data, at + bsize - 4)[0]
        out.append((base + at, payload))
        at += bsize
    assert at == len(data)
    return out


class Layout:
    """Uncompressed positions of a member list -> virtual offsets.  A position on a member's first byte belongs to that member;
    the position behind the last byte is the next member's start (an empty member, or `behind`)."""

    def __init__(self, mem, behind):
        self.mem, self.behind = mem, behind
        self.cum = [0]
        for _, p in mem:
            self.cum.append(self.cum[-1] + len(p))
        self.raw = b"".join(p for _, p in mem)

    def voff(self, p):
        if p == self.cum[-1]:
            empty = [off for (off, pl), c in zip(self.mem, self.cum) if c == p and not pl]
            return (empty[0] if empty else self.behind) << 16
        k = bisect.bisect_right(self.cum, p) - 1
        return (self.mem[k][0] << 16) | (p - self.cum[k])


def records_of(layout, first=0):
    """The records in layout.raw[first:] with their virtual offsets: bai_model's record dicts."""
    recs = bm.parse_records(layout.raw[first:])
    for r in recs:
        r["u"] = layout.voff(first + r["at"])
        r["v"] = layout.voff(first + r["at"] + r["size"])
    return recs


def bam_records(data):
    """A whole BAM file's bytes -> (n_ref, records with virtual offsets); the end-of-file marker must be there."""
    mem = walk_members(data)
    assert mem and mem[-1][1] == b"", "no end-of-file marker"
    lay = Layout(mem, len(data))
    raw = lay.raw
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    return n_ref, records_of(lay, at)


class Reader:
    """Seeks into a file's bytes by virtual offset and reads records from there."""

    def __init__(self, data):
        self.data = data
        self.cache = {}

    def member(self, coff):
        if coff not in self.cache:
            bsize = struct.unpack_from("<H", self.data, coff + 16)[0] + 1
            self.cache[coff] = (zlib.decompress(self.data[coff + 18:coff + bsize - 8], -15), coff + bsize)
        return self.cache[coff]

    def records(self, beg, end):
        """(virtual offset, tid, pos, flag, reflen) of the records that start in [beg, end)."""
        coff, within = beg >> 16, beg & 0xffff
        out = []
        while coff < len(self.data):
            payload, nxt = self.member(coff)
            if within >= len(payload):   # (behind the member's last byte: the next member's first)
                coff, within = nxt, within - len(payload)
                continue
            u = (coff << 16) | within
            if u >= end:
                break
            buf, c, w = b"", coff, within

            def take(n):
                nonlocal buf, c, w
                while len(buf) < n:
                    p, nx = self.member(c)
                    buf += p[w:]
                    c, w = nx, 0
            take(4)
            size = 4 + struct.unpack_from("<I", buf, 0)[0]
            take(size)
            rec = bm.parse_records(buf[:size])[0]
            out.append((u, rec["tid"], rec["pos"], rec["flag"], rec["reflen"]))
            # where the next record starts
            within += size
            while coff < len(self.data):
                payload, nxt = self.member(coff)
                if within < len(payload):
                    break
                within -= len(payload)
                coff = nxt
        return out


def regions_of(recs, n_ref, n_random=200, seed=1):
    """The designed regions — around every record's ends, every reg2bin level boundary a record touches — and random ones."""
    rng = random.Random(seed)
    mapped = [r for r in recs if r["tid"] >= 0 and not r["flag"] & 4]
    out = set()
    for r in rng.sample(mapped, min(len(mapped), 60)):
        beg, end = bm.span_of(r)
        out |= {(r["tid"], beg, beg + 1), (r["tid"], end - 1, end), (r["tid"], end, end + 1), (r["tid"], max(beg - 1, 0), beg)}
    for tid in range(n_ref):
        for shift in (14, 17, 20, 23, 26):
            b = 1 << shift
            out |= {(tid, b - 1, b), (tid, b, b + 1), (tid, b - 1, b + 1), (tid, 0, b)}
        out.add((tid, 0, 1 << 29))
    top = max([bm.span_of(r)[1] for r in mapped] + [1]) + 40_000
    for _ in range(n_random):
        beg = rng.randrange(top)
        out.add((rng.randrange(n_ref), beg, beg + rng.choice([1, 50, 3000, 16384, 200_000])))
    return sorted(out)


def check_queries(data, bai_bytes, recs, n_ref, n_random=200):
    """Every region: what the index finds in the file's bytes is exactly what brute force finds (records with flag 4 clear)."""
    bai = bm.read_bai(bai_bytes)
    rd = Reader(data)
    n_hits = 0
    for tid, beg, end in regions_of(recs, n_ref, n_random):
        want = sorted(r["u"] for r in recs if r["tid"] == tid and not r["flag"] & 4 and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg)
        got = set()
        for cb, ce in bm.query(bai, tid, beg, end):
            for u, t, pos, flag, reflen in rd.records(cb, ce):
                r = dict(tid=t, pos=pos, flag=flag, reflen=reflen)
                if t == tid and not flag & 4 and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg:
                    got.add(u)
        assert sorted(got) == want, (tid, beg, end, len(got), len(want))
        n_hits += len(want)
    assert n_hits > 0
    return n_hits
