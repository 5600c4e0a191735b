"""The BAI index of coordinate-sorted output, stated in plain Python: the arbiter of --write-index.

The layout is the SAM specification's §5.2; what goes into it is the rule below, which follows the shape of htslib's
hts_idx_push without its folding of sparse deep bins.  Byte equality with `samtools index` is not claimed.

A record here is a dict: tid, pos, flag, reflen (reference bases of the CIGAR's M, D, N, = and X ops), u, v (the virtual
offsets of its first byte and of the byte behind its last).

  span     beg = max(pos, 0); end = beg + max(reflen, 1), reflen counting as 0 with flag 4; bin = reg2bin(beg, end)
  order    key = (tid as u32) << 32 | (pos + 1 as u32) must not decrease; tid >= 0 with end > 2^29 cannot be indexed
  bins     per tid >= 0: every maximal run of consecutive records of one (tid, bin) is a chunk (u of its first, v of its last);
           at finish, within a bin in file order, a chunk merges into the one before when prev.v >> 16 >= next.u >> 16
  37450    per tid with records: (u of its first record, v of its last), (n_mapped, n_unmapped) by flag 4
  linear   records with flag 4 clear: ioffset[w] = the smallest u over the records whose windows beg >> 14 .. (end - 1) >> 14
           hold w; n_intv = 1 + the largest such w; a window without a record takes the next higher window's value
  trailer  n_no_coor = records with tid < 0, always written

per_call() is what one call of the device stage leaves (offsets relative to the call); Builder is what the host makes of the
calls; build() is both over a whole record list.  read_bai() and query() are written from the specification alone and share
nothing with the builder."""
import struct

MAX_END = 1 << 29
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


class IndexError_(Exception):
    """What fails a call: kind 'order' (FADEHIP_E_INVALID) or 'span' (FADEHIP_E_UNSUPPORTED), and the record's index."""

    def __init__(self, kind, record):
        super().__init__("%s at record %d" % (kind, record))
        self.kind = kind
        self.record = record


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def key_of(r):
    return ((r["tid"] & 0xffffffff) << 32) | ((r["pos"] + 1) & 0xffffffff)


def span_of(r):
    beg = max(r["pos"], 0)
    reflen = 0 if r["flag"] & 4 else r["reflen"]
    return beg, beg + max(reflen, 1)


def parse_records(payload):
    """BAM records (block_size first) back to back -> [(offset, tid, pos, flag, reflen)] and the total."""
    out, o = [], 0
    while o < len(payload):
        bs, tid, pos = struct.unpack_from("<Iii", payload, o)
        lname = payload[o + 12]
        ncig, flag = struct.unpack_from("<HH", payload, o + 16)
        ops = struct.unpack_from("<%dI" % ncig, payload, o + 36 + lname)
        out.append(dict(at=o, tid=tid, pos=pos, flag=flag, reflen=sum(c >> 4 for c in ops if (c & 15) in REF_OPS), size=4 + bs))
        o += 4 + bs
    assert o == len(payload)
    return out


def virtual_offset(p, block, coff, total, behind):
    """Byte position p of a call's uncompressed output cut into blocks of `block` bytes: coff[k] is member k's file offset,
    `behind` the file offset behind the call's last member (what p == total maps to)."""
    if p == total:
        return behind << 16
    return (coff[p // block] << 16) | (p % block)


def per_call(recs, prev_key=None, first_index=0):
    """What the device stage leaves for the records of one call, in stream order: dense chunks (tid, bin, u, v), linear
    entries (tid, window, u), reference runs (tid, u, v, n_mapped, n_unmapped) — tid -1 included —, first and last key."""
    chunks, linear, refs = [], [], []
    bad = []
    front = prev_key
    run_max = {}
    for i, r in enumerate(recs):
        k = key_of(r)
        beg, end = span_of(r)
        if front is not None and k < front:
            bad.append(("order", i))
        if r["tid"] >= 0 and end > MAX_END:
            bad.append(("span", i))
        front = k
    if bad:
        kind, i = min(bad, key=lambda b: (b[1], b[0] != "order"))
        raise IndexError_(kind, first_index + i)
    last_tid = None
    last_bin = None
    for r in recs:
        tid = r["tid"]
        beg, end = span_of(r)
        mapped = not (r["flag"] & 4)
        if tid != last_tid or not refs:
            refs.append([tid, r["u"], r["v"], 0, 0])
            last_bin = None
            run_max[tid] = -1  # (a tid that comes back later in a call would be an order error)
        refs[-1][2] = r["v"]
        refs[-1][3 if mapped else 4] += 1
        last_tid = tid
        if tid < 0:
            continue
        b = reg2bin(beg, end)
        if b != last_bin:
            chunks.append([tid, b, r["u"], r["v"]])
            last_bin = b
        chunks[-1][3] = r["v"]
        if mapped:
            w0, w1 = beg >> 14, (end - 1) >> 14
            for w in range(max(w0, run_max[tid] + 1), w1 + 1):
                linear.append((tid, w, r["u"]))
            run_max[tid] = max(run_max[tid], w1)
    return dict(chunks=[tuple(c) for c in chunks], linear=linear, refs=[tuple(x) for x in refs], n=len(recs),
                first_key=key_of(recs[0]) if recs else 0, last_key=key_of(recs[-1]) if recs else 0)


def rebase(voff, base):
    """A call-relative virtual offset against the file offset of the call's first member."""
    return voff + (base << 16)


class Builder:
    """The host's part: add() the calls in order (offsets rebased by the call's base file offset), finish() the bytes."""

    def __init__(self, n_ref):
        self.n_ref = n_ref
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
            assert 0 <= tid < self.n_ref
            self.bins[tid].setdefault(b, []).append([rebase(u, base), rebase(v, base)])
        for tid, w, off in call["linear"]:
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

    def finish(self):
        out = [b"BAI\1", struct.pack("<i", self.n_ref)]
        for tid in range(self.n_ref):
            m = self.meta[tid]
            if m is None:
                out.append(struct.pack("<ii", 0, 0))
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
                out.append(struct.pack("<Ii", b, len(merged)))
                out.extend(struct.pack("<QQ", u, v) for u, v in merged)
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, m[0], m[1], m[2], m[3]))
            lin = self.lin[tid]
            n_intv = 1 + max(lin) if lin else 0
            vals = [0] * n_intv
            nxt = 0
            for w in range(n_intv - 1, -1, -1):
                nxt = lin.get(w, nxt)
                vals[w] = nxt
            out.append(struct.pack("<i", n_intv))
            out.append(struct.pack("<%dQ" % n_intv, *vals))
        out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)


def build(n_ref, recs):
    """The .bai of a whole file's records (u, v absolute)."""
    b = Builder(n_ref)
    b.add(0, per_call(recs))
    return b.finish()


# ------------------------------------------------------------------------------------------------ the reader's side
def read_bai(data):
    """A .bai's bytes -> dict(refs=[dict(bins={bin: [(beg, end), ...]}, meta=(u, v, n_mapped, n_unmapped) or None,
    ioffset=[...])], n_no_coor=int or None).  Every byte must be used."""
    assert data[:4] == b"BAI\1", data[:4]
    n_ref, = struct.unpack_from("<i", data, 4)
    o = 8
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, o)
        o += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", data, o + 16 * c) for c in range(n_chunk)]
            o += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and meta is None
                meta = chunks[0] + chunks[1]
            else:
                assert b not in bins and b < PSEUDO_BIN - 1
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", data, o)
        o += 4
        ioffset = list(struct.unpack_from("<%dQ" % n_intv, data, o))
        o += 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, ioffset=ioffset))
    n_no_coor = None
    if o < len(data):
        n_no_coor, = struct.unpack_from("<Q", data, o)
        o += 8
    assert o == len(data), (o, len(data))
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    """The specification's reg2bins: every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def query(bai, tid, beg, end):
    """The chunks a reader has to scan for records of reference tid overlapping [beg, end): the candidate bins' chunks whose
    end lies above the linear index's offset for the window of beg, sorted, as (chunk_beg, chunk_end)."""
    ref = bai["refs"][tid]
    lin = ref["ioffset"]
    w = beg >> 14
    min_off = lin[w] if w < len(lin) else 0  # (nothing is known about windows behind the last: no cut-off)
    out = []
    for b in reg2bins(beg, end):
        for cb, ce in ref["bins"].get(b, ()):
            if ce > min_off:
                out.append((cb, ce))
    return sorted(out)
