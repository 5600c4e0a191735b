"""A DEFLATE (RFC 1951) writer for tests.  Not a compressor: a way to say exactly which bits go into a stream, so that the
inflaters (fade_amd/csrc/bgzf_inflate.hpp, host/inflate_fast.hpp, the hts_lite reader) can be shown streams that zlib's
deflate would never write.  The reference for every verdict and every byte is zlib's inflate (`expected`)."""
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


class BitWriter:
    """Bits least significant first (RFC 1951 3.1.1); Huffman codes go in most significant bit first."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bits(self):
        return 8 * len(self.buf) + self.n

    def put(self, value, n):
        assert 0 <= value < (1 << n) or n == 0 and value == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        rev = 0
        for _ in range(n):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.put(rev, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw_bytes(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lens):
    """Code of every symbol from the code lengths (RFC 1951 3.2.2); symbols of length 0 get None.  An over-subscribed
    set still gets numbers (truncated to the length): such a header is what an invalid case wants to write."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(None)
        else:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
    return out


def kraft_left(lens, maxbits=15):
    """Code space left over, in units of 2^-maxbits: 0 complete, > 0 incomplete, < 0 over-subscribed."""
    return (1 << maxbits) - sum(1 << (maxbits - l) for l in lens if l)


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length, the shortest way (258 as code 285)."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    for s in range(27, -1, -1):
        if LBASE[s] <= length:
            return 257 + s, LEXTRA[s], length - LBASE[s]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    for s in range(29, -1, -1):
        if DBASE[s] <= dist:
            return s, DEXTRA[s], dist - DBASE[s]


# ---- code-length sets of a wanted shape
def complete_shape(n_used, longest=None):
    """Sorted lengths of a complete prefix code for n_used symbols whose longest code has `longest` bits (default: as
    flat as possible).  n_used >= longest + 1 and n_used <= 2^longest."""
    assert n_used >= 2
    if longest is None:
        k = (n_used - 1).bit_length()
        short = (1 << k) - n_used
        return [k - 1] * short + [k] * (n_used - short)
    assert longest + 1 <= n_used <= (1 << longest), (n_used, longest)
    lens = list(range(1, longest)) + [longest, longest]  # the chain 1, 2, ..., longest, longest
    while len(lens) < n_used:
        # split the shortest leaf that is not at full depth: one symbol more, still complete
        i = min((l, k) for k, l in enumerate(lens) if l < longest)[1]
        l = lens.pop(i)
        lens += [l + 1, l + 1]
    return sorted(lens)


def assign(n_symbols, symbols_short_first, shape):
    """lens[0..n_symbols): the sorted `shape` handed to the listed symbols, the first listed getting the shortest code."""
    assert len(symbols_short_first) == len(shape) and len(set(symbols_short_first)) == len(shape)
    lens = [0] * n_symbols
    for s, l in zip(symbols_short_first, sorted(shape)):
        lens[s] = l
    return lens


def lone_code(n_symbols, symbol):
    """The one incomplete set zlib takes for literal/length and distance codes: a single code of one bit."""
    lens = [0] * n_symbols
    lens[symbol] = 1
    return lens


def no_code(n_symbols):
    return [0] * n_symbols


# ---- run-length coding of the header's code lengths
def rle_code_lengths(lit_lens, dist_lens, mode):
    """[(symbol, extra value)] for the HLIT + HDIST lengths.  mode "none": never 16 / 17 / 18; "greedy": the longest
    repeat at every step, each alphabet on its own (zlib's way); "long": the same over both alphabets as one run of
    numbers, so that repeats cross the HLIT / HDIST seam (legal: RFC 1951 3.2.7)."""
    if mode == "none":
        return [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    assert mode in ("greedy", "long")
    parts = [list(lit_lens) + list(dist_lens)] if mode == "long" else [list(lit_lens), list(dist_lens)]
    seq = []
    for lens in parts:
        i, prev = 0, None
        while i < len(lens):
            v = lens[i]
            run = 1
            while i + run < len(lens) and lens[i + run] == v:
                run += 1
            if v == 0 and run >= 3:
                r = min(run, 138)
                seq.append((17, r - 3) if r <= 10 else (18, r - 11))
                i += r
                prev = 0
            elif prev is not None and v == prev and run >= 3:
                r = min(run, 6)
                seq.append((16, r - 3))
                i += r
            else:
                seq.append((v, 0))
                i += 1
                prev = v
    return seq


def cl_spans(seq):
    """(start, count) of every item of a code-length sequence, in lengths written."""
    out, k = [], 0
    for sym, extra in seq:
        n = 1 if sym < 16 else (3 + extra if sym in (16, 17) else 11 + extra)
        out.append((k, n))
        k += n
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Stream:
    """One raw DEFLATE stream under construction.  `payload` follows what a correct inflater makes of it."""

    def __init__(self, history=b""):
        self.w = BitWriter()
        self.payload = bytearray(history)
        self.block_starts = []  # bit position of every block header
        self.cl_sequence = None  # of the last dynamic header
        self.hclen = None

    @property
    def bits(self):
        return self.w.bits

    def raw(self):
        return self.w.getvalue()

    def _header(self, final, btype):
        self.block_starts.append(self.w.bits)
        self.w.put(1 if final else 0, 1)
        self.w.put(btype, 2)

    def stored(self, data, final=False, len_field=None, nlen_field=None, body=None):
        """A stored block; len_field / nlen_field / body override what is written (for invalid cases)."""
        data = bytes(data)
        assert len(data) <= 65535
        self._header(final, 0)
        self.w.align()
        ln = len(data) if len_field is None else len_field
        self.w.put(ln, 16)
        self.w.put((ln ^ 0xffff) if nlen_field is None else nlen_field, 16)
        self.w.raw_bytes(data if body is None else body)
        self.payload += data
        return self

    def reserved(self, final=True):
        """BTYPE 3."""
        self._header(final, 3)
        return self

    def _emit(self, tokens, lit_lens, dist_lens, eob):
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        w, out = self.w, self.payload

        def lit_sym(s):
            assert lit_lens[s], "no code for literal/length symbol %d" % s
            w.code(lc[s], lit_lens[s])

        def match(ls, lx, lv, ds, dx, dv):
            lit_sym(ls)
            w.put(lv, lx)
            assert dist_lens[ds], "no code for distance symbol %d" % ds
            w.code(dc[ds], dist_lens[ds])
            w.put(dv, dx)
            if ls - 257 < 29 and ds < 30:
                length, dist = LBASE[ls - 257] + lv, DBASE[ds] + dv
                if dist > len(out):  # (an invalid case: what an inflater would copy is not defined)
                    out.extend(bytes(length))
                elif dist >= length:
                    out.extend(out[len(out) - dist:len(out) - dist + length])
                else:
                    piece = bytes(out[len(out) - dist:])
                    out.extend((piece * (length // dist + 1))[:length])

        for t in tokens:
            if isinstance(t, int):
                lit_sym(t)
                out.append(t)
            elif t[0] == "sym":  # a bare literal/length symbol, nothing behind it
                lit_sym(t[1])
            elif t[0] == "bits":  # anything
                w.put(t[1], t[2])
            elif len(t) == 2:
                ls, lx, lv = length_symbol(t[0])
                ds, dx, dv = dist_symbol(t[1])
                match(ls, lx, lv, ds, dx, dv)
            else:
                ls, lv, ds, dv = t
                match(ls, LEXTRA[ls - 257] if ls - 257 < 29 else 0, lv, ds, DEXTRA[ds] if ds < 30 else 0, dv)
        if eob:
            lit_sym(256)

    def fixed(self, tokens, final=False, eob=True):
        self._header(final, 1)
        self._emit(tokens, FIXED_LIT_LENS, FIXED_DIST_LENS, eob)
        return self

    def dynamic(self, tokens, final, lit_lens, dist_lens, cl_lens=None, hclen=None, cl_sequence=None, rle="greedy", eob=True,
                hlit_field=None, hdist_field=None, stop_after_bits=None):
        """A dynamic block.  lit_lens has HLIT entries (257..286), dist_lens HDIST (1..30).  cl_sequence: explicit
        [(code-length symbol, extra value)]; otherwise the lengths are run-length coded by `rle`.  cl_lens: the 19
        lengths of the code-length code; by default a complete code over the symbols the sequence uses.  hlit_field /
        hdist_field override the two 5-bit counts as written."""
        self._header(final, 2)
        w = self.w
        seq = list(cl_sequence) if cl_sequence is not None else rle_code_lengths(lit_lens, dist_lens, rle)
        if cl_lens is None:
            used = sorted(set(s for s, _ in seq), key=lambda s: -sum(1 for q, _ in seq if q == s))
            if len(used) == 1:
                used.append(0 if used[0] != 0 else 1)
            cl_lens = assign(19, used, complete_shape(len(used)))
        assert len(cl_lens) == 19
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        assert 4 <= hclen <= 19
        w.put(len(lit_lens) - 257 if hlit_field is None else hlit_field, 5)
        w.put(len(dist_lens) - 1 if hdist_field is None else hdist_field, 5)
        w.put(hclen - 4, 4)
        for k in range(hclen):
            w.put(cl_lens[CL_ORDER[k]], 3)
        cc = canonical_codes(cl_lens)
        for sym, extra in seq:
            assert cl_lens[sym], "no code for code-length symbol %d" % sym
            w.code(cc[sym], cl_lens[sym])
            if sym >= 16:
                w.put(extra, CL_EXTRA[sym])
        self.cl_sequence, self.hclen = seq, hclen
        self._emit(tokens, list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens)), eob)
        return self


def expected(raw, isize=None):
    """What zlib makes of a raw stream: ("ok", bytes, unused) when the final block's end was reached, ("error", message)
    on zlib.error, ("truncated", bytes) when the stream ends before that.  With `isize` (a BGZF member's trailer) a stream
    that zlib inflates to another number of bytes is an error too, as it is for htslib's reader."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error as e:
        return ("error", str(e))
    if not d.eof:
        return ("truncated", out)
    if isize is not None and len(out) != isize:
        return ("error", "inflates to %d bytes, ISIZE says %d" % (len(out), isize))
    return ("ok", out, d.unused_data)
