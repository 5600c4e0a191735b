"""The CSI index of coordinate-sorted output, stated in plain Python: the arbiter of --write-index --csi.

The layout is CSI version 1 (the "CSIv1" document beside the SAM specification); what goes into it is the rule below, the one
of tests/bai_model.py carried from BAI's fixed five levels of 16 kb windows to a geometry.  htslib's choice of a depth and its
folding of sparse deep bins are not reproduced: byte equality with `samtools index -c` is not claimed, and samtools was not
at hand to try a file on.  read_csi() and query() below, written from the layout alone, are what the files are held to.

  geometry (min_shift, depth), 4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32; limit = 2^(min_shift + 3 depth)
  bins     level l = 0 (the root) .. depth has 8^l bins of 2^(min_shift + 3 (depth - l)) positions each, numbered from
           (8^l - 1) / 7; a record's bin is the deepest one that holds [beg, end).  (14, 5) is BAI's reg2bin
  span     as bai_model: beg = max(pos, 0); end = beg + max(reflen, 1), reflen counting as 0 with flag 4
  order    as bai_model; tid >= 0 with end > limit cannot be indexed ('span', naming the record)
  chunks   per maximal run of consecutive records of one (tid, bin); merged at finish as BAI's: prev.v >> 16 >= next.u >> 16
  linear   per call, as bai_model with windows of 2^min_shift positions.  A CSI file has no linear index: the entries are
           what the host derives every bin's loffset from
  loffset  of a bin at level l, k-th of its level: the back-filled linear value at its first window, k << 3 (depth - l) —
           a window without an entry takes the next higher window's value —, 0 when that window lies behind the last window
           that has a value
  pseudo   bin ((1 << (3 depth + 3)) - 1) / 7 + 1 per tid with records, behind its bins: loffset 0, two chunks filled as
           BAI's 37450 (37450 for depth 5, 299594 for depth 6)
  payload  "CSI\\1", min_shift, depth, l_aux = 0, n_ref, the references (n_bin; per bin: bin, loffset, n_chunk, chunks),
           n_no_coor (always written).  The file: the payload in BGZF members, then the end-of-file marker

Why a bin's loffset is a lower bound a reader may cut with (query): in a sorted file the linear values do not decrease with
the window — the record with the smallest offset over window w' either reaches back into a window w < w', and then bounds
w's value from above, or begins behind w, and then every record over w lies in front of it in the file.  A mapped record R
that overlaps [beg, end) covers a window w >= the window of beg >= the first window f of any bin that contains beg, so
u(R) >= linear[w] >= back-filled[f] = loffset; the chunk that holds R ends behind u(R).  So among the bins that contain beg
— the leaf and its ancestors — every existing one's loffset is such a bound, and the largest is the best of them.

It imports nothing from the builder it judges; from bai_model only the record's key and span, the parser and rebase."""
import struct
import zlib

from bai_model import IndexError_, key_of, parse_records, rebase, span_of  # noqa: F401  (parse_records: for the tests)

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_BLOCK = 0xff00


def check_geometry(min_shift, depth):
    return 4 <= min_shift and 1 <= depth <= 8 and min_shift + 3 * depth <= 32


def limit_of(min_shift, depth):
    assert check_geometry(min_shift, depth), (min_shift, depth)
    return 1 << (min_shift + 3 * depth)


def first_bin(level):
    return ((1 << (3 * level)) - 1) // 7


def pseudo_bin(depth):
    return ((1 << (3 * depth + 3)) - 1) // 7 + 1


def reg2bin(beg, end, min_shift, depth):
    """The deepest bin that holds [beg, end) (end <= limit)."""
    end -= 1
    for level in range(depth, 0, -1):
        s = min_shift + 3 * (depth - level)
        if beg >> s == end >> s:
            return first_bin(level) + (beg >> s)
    return 0


def bin_level(b, depth):
    """(level, index within the level) of bin number b."""
    for level in range(depth, -1, -1):
        if b >= first_bin(level):
            return level, b - first_bin(level)
    raise AssertionError(b)


def per_call(recs, min_shift, depth, prev_key=None, first_index=0):
    """What the device stage leaves for the records of one call under the geometry, in stream order: the three dense arrays
    of bai_model.per_call — chunks (tid, bin, u, v), linear (tid, window, u), refs (tid, u, v, n_mapped, n_unmapped), tid -1
    included — and first and last key."""
    limit = limit_of(min_shift, depth)
    bad = []
    front = prev_key
    for i, r in enumerate(recs):
        k = key_of(r)
        if front is not None and k < front:
            bad.append(("order", i))
        if r["tid"] >= 0 and span_of(r)[1] > limit:
            bad.append(("span", i))
        front = k
    if bad:
        kind, i = min(bad, key=lambda b: (b[1], b[0] != "order"))
        raise IndexError_(kind, first_index + i)
    chunks, linear, refs = [], [], []
    last_tid = last_bin = None
    run_max = -1
    for r in recs:
        tid = r["tid"]
        beg, end = span_of(r)
        mapped = not (r["flag"] & 4)
        if tid != last_tid or not refs:
            refs.append([tid, r["u"], r["v"], 0, 0])
            last_bin = None
            run_max = -1
        refs[-1][2] = r["v"]
        refs[-1][3 if mapped else 4] += 1
        last_tid = tid
        if tid < 0:
            continue
        b = reg2bin(beg, end, min_shift, depth)
        if b != last_bin:
            chunks.append([tid, b, r["u"], r["v"]])
            last_bin = b
        chunks[-1][3] = r["v"]
        if mapped:
            w0, w1 = beg >> min_shift, (end - 1) >> min_shift
            for w in range(max(w0, run_max + 1), w1 + 1):
                linear.append((tid, w, r["u"]))
            run_max = max(run_max, w1)
    return dict(chunks=[tuple(c) for c in chunks], linear=linear, refs=[tuple(x) for x in refs], n=len(recs),
                first_key=key_of(recs[0]) if recs else 0, last_key=key_of(recs[-1]) if recs else 0)


class Builder:
    """The host's part: add() the calls in order (offsets rebased by the call's base file offset), finish() the payload."""

    def __init__(self, n_ref, min_shift, depth):
        assert check_geometry(min_shift, depth)
        self.n_ref, self.min_shift, self.depth = n_ref, min_shift, depth
        self.bins = [dict() for _ in range(n_ref)]    # bin -> [[u, v], ...] in file order
        self.lin = [dict() for _ in range(n_ref)]     # window -> offset (first writer wins)
        self.meta = [None] * n_ref                    # [u, v, n_mapped, n_unmapped]
        self.n_no_coor = 0
        self.last_key = None
        self.n_records = 0

    def add(self, base, call):
        if call["n"]:
            if self.last_key is not None and call["first_key"] < self.last_key:
                raise IndexError_("order", self.n_records)
            self.last_key = call["last_key"]
        self.n_records += call["n"]
        for tid, b, u, v in call["chunks"]:
            assert 0 <= tid < self.n_ref and 0 <= b < pseudo_bin(self.depth) - 1
            self.bins[tid].setdefault(b, []).append([rebase(u, base), rebase(v, base)])
        for tid, w, off in call["linear"]:
            assert 0 <= w < 1 << (3 * self.depth)
            self.lin[tid].setdefault(w, rebase(off, base))
        for tid, u, v, nm, nu in call["refs"]:
            if tid < 0:
                self.n_no_coor += nm + nu
                continue
            m = self.meta[tid]
            if m is None:
                self.meta[tid] = [rebase(u, base), rebase(v, base), nm, nu]
            else:
                m[1] = rebase(v, base)
                m[2] += nm
                m[3] += nu

    def loffset(self, tid, b):
        """The back-filled linear value at bin b's first window; 0 behind the last window that has a value."""
        level, k = bin_level(b, self.depth)
        first = k << (3 * (self.depth - level))
        above = [w for w in self.lin[tid] if w >= first]
        return self.lin[tid][min(above)] if above else 0

    def finish(self):
        out = [b"CSI\1", struct.pack("<iiii", self.min_shift, self.depth, 0, self.n_ref)]
        for tid in range(self.n_ref):
            m = self.meta[tid]
            if m is None:
                out.append(struct.pack("<i", 0))
                continue
            bins = self.bins[tid]
            out.append(struct.pack("<i", len(bins) + 1))
            for b in sorted(bins):
                merged = []
                for u, v in bins[b]:
                    if merged and merged[-1][1] >> 16 >= u >> 16:
                        merged[-1][1] = v
                    else:
                        merged.append([u, v])
                out.append(struct.pack("<IQi", b, self.loffset(tid, b), len(merged)))
                out.extend(struct.pack("<QQ", u, v) for u, v in merged)
            out.append(struct.pack("<IQiQQQQ", pseudo_bin(self.depth), 0, 2, m[0], m[1], m[2], m[3]))
        out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)


def build(n_ref, recs, min_shift, depth):
    """The CSI payload of a whole file's records (u, v absolute)."""
    b = Builder(n_ref, min_shift, depth)
    b.add(0, per_call(recs, min_shift, depth))
    return b.finish()


def file_bytes(payload, level=6):
    """The file: the payload in BGZF members of at most 0xff00 payload bytes, then the end-of-file marker."""
    out = []
    for at in range(0, len(payload), BGZF_BLOCK):
        part = payload[at:at + BGZF_BLOCK]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(part) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out) + BGZF_EOF


def payload_of(data):
    """A .csi file's bytes back to the payload: every member inflated and checked, the end-of-file marker required."""
    assert data.endswith(BGZF_EOF), "no end-of-file marker"
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", at
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        part = zlib.decompress(data[at + 18:at + bsize - 8], -15)
        crc, n = struct.unpack_from("<II", data, at + bsize - 8)
        assert (zlib.crc32(part), len(part)) == (crc, n) and n <= BGZF_BLOCK, at
        out.append(part)
        at += bsize
    assert at == len(data)
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ the reader's side
def read_csi(payload):
    """A CSI payload -> dict(min_shift, depth, aux, refs=[dict(bins={bin: (loffset, [(beg, end), ...])}, meta=(u, v, n_mapped,
    n_unmapped) or None)], n_no_coor=int or None).  Every byte must be used."""
    assert payload[:4] == b"CSI\1", payload[:4]
    min_shift, depth, l_aux = struct.unpack_from("<iii", payload, 4)
    assert check_geometry(min_shift, depth), (min_shift, depth)
    aux = payload[16:16 + l_aux]
    o = 16 + l_aux
    n_ref, = struct.unpack_from("<i", payload, o)
    o += 4
    pseudo = pseudo_bin(depth)
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", payload, o)
        o += 4
        bins, meta, last = {}, None, -1
        for _ in range(n_bin):
            b, loffset, n_chunk = struct.unpack_from("<IQi", payload, o)
            o += 16
            chunks = [struct.unpack_from("<QQ", payload, o + 16 * c) for c in range(n_chunk)]
            o += 16 * n_chunk
            assert b > last, (b, last)  # (ascending bin numbers, the pseudo-bin last)
            last = b
            if b == pseudo:
                assert n_chunk == 2 and meta is None and loffset == 0
                meta = chunks[0] + chunks[1]
            else:
                assert b < pseudo - 1 and n_chunk > 0
                bins[b] = (loffset, chunks)
        refs.append(dict(bins=bins, meta=meta))
    n_no_coor = None
    if o < len(payload):
        n_no_coor, = struct.unpack_from("<Q", payload, o)
        o += 8
    assert o == len(payload), (o, len(payload))
    return dict(min_shift=min_shift, depth=depth, aux=aux, refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end, min_shift, depth):
    """Every bin on every level that overlaps [beg, end)."""
    limit = limit_of(min_shift, depth)
    end = min(end, limit)
    if beg >= end:
        return []
    end -= 1
    out = []
    for level in range(depth + 1):
        s = min_shift + 3 * (depth - level)
        out.extend(range(first_bin(level) + (beg >> s), first_bin(level) + (end >> s) + 1))
    return out


def query(csi, tid, beg, end):
    """The chunks a reader has to scan for records of reference tid overlapping [beg, end): the chunks of every bin on every
    level that overlaps the region, less those that end at or in front of min_off — the largest loffset among the existing
    bins that contain beg (the leaf holding beg and its ancestors), 0 if there is none.  Sorted (chunk_beg, chunk_end)."""
    min_shift, depth = csi["min_shift"], csi["depth"]
    ref = csi["refs"][tid]
    min_off = 0
    if beg < limit_of(min_shift, depth):
        for level in range(depth + 1):
            b = first_bin(level) + (beg >> (min_shift + 3 * (depth - level)))
            if b in ref["bins"]:
                min_off = max(min_off, ref["bins"][b][0])
    out = []
    for b in reg2bins(beg, end, min_shift, depth):
        if b in ref["bins"]:
            out.extend((cb, ce) for cb, ce in ref["bins"][b][1] if ce > min_off)
    return sorted(out)
