"""Payloads built to reach the limits of the device BGZF compressor (fade_amd/csrc/bgzf_deflate_g64.hpp, bgzf_deflate_g32.hpp),
and what proves that a limit was reached: a DEFLATE (RFC 1951) token parser of the tests' own.

build_edge_cases(geom) -> {name: payload}, deterministic from fixed seeds, at most two blocks and a ragged tail each.
deflate_tokens(raw)    -> the block type, the header's counts and code lengths, and the tokens of one raw stream.  It shares no
                          code with tests/deflate_builder.py's writer and none with the product.
optimal_depth(freqs)   -> the depth of an unrestricted Huffman code for a frequency table.
reach(geom, name, payload, streams) asserts the case's reach condition on the CPU model's streams
(tests/test_bgzf_edges_model.py); tests/test_gpu_bgzf_edges.py then holds the device to the model's bytes, which carries the
conditions over.

The header counts are reported as COUNTS: n_litlen = HLIT + 257, n_dist = HDIST + 1, n_cl = HCLEN + 4, next to the raw fields
(hlit, hdist, hclen).  A full literal/length alphabet is n_litlen == 286, a full distance alphabet n_dist == 30.

Not built: a header whose code-length alphabet needs the 7-bit limit.  Its 19 symbols would have to come with Fibonacci-like
frequencies out of the run-length coded code lengths of a real block (at least 34 + 21 + 13 + ... tokens in the right
proportions from at most 316 lengths); no payload tried here reached it through the model, so the limit_code_lengths(.., 7, ..)
call is covered only by the model's own unit check of that helper."""
import heapq
import os
import struct
import subprocess

import numpy as np

CUT = {64: 0xff00, 32: 0x7f00}      # FADEHIP_BGZF_GEOM -> bytes of a block
CAP = {64: 8192, 32: 320}           # match records: a block's (g64), a segment's (g32)
N_SEG = 8                           # segments of a g32 block
MIN_MATCH, MAX_MATCH = 4, 258


# ---------------------------------------------------------------- the reference: the CPU model
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fade_amd", "csrc")


def model_streams(geom, cases, tmp):
    """{name: [the raw DEFLATE stream of every block]} from host/selftest/gpu_deflate_model.cpp (an ASan + UBSan build: a report
    fails the run), one run for all the payloads.  The model also inflates every stream with zlib and fails if one differs."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/gpu_deflate_model"])
    names, files = list(cases), []
    for k, name in enumerate(names):
        files.append(os.path.join(str(tmp), "g%d_%03d.bin" % (geom, k)))
        with open(files[-1], "wb") as f:
            f.write(cases[name])
    dump = os.path.join(str(tmp), "g%d.model" % geom)
    if os.path.exists(dump):
        os.remove(dump)
    env = dict(os.environ, MODEL_DUMP=dump, MODEL_GEOM=str(geom), MODEL_FILES_ONLY="1",
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    subprocess.run([os.path.join(CSRC, "build", "gpu_deflate_model")] + files, check=True, stdout=subprocess.DEVNULL, env=env)
    with open(dump, "rb") as f:
        raw = f.read()
    out, at = {}, 0
    for name in names:
        out[name] = []
        for _ in range((len(cases[name]) + CUT[geom] - 1) // CUT[geom]):
            n = struct.unpack_from("<I", raw, at)[0]
            out[name].append(raw[at + 4:at + 4 + n])
            at += 4 + n
    assert at == len(raw)
    return out


# ---------------------------------------------------------------- the parser
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, raw):
        self.raw, self.at, self.acc, self.n = raw, 0, 0, 0

    def need(self, k):
        while self.n < k:
            self.acc |= (self.raw[self.at] if self.at < len(self.raw) else 0) << self.n
            self.at += 1
            self.n += 8

    def take(self, k):
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def bytes_used(self):
        return self.at - self.n // 8


def _decoder(lengths):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2), codes as read bit by bit, first bit most significant."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError("no such code")


def deflate_tokens(raw):
    """One raw DEFLATE stream of ONE block (BFINAL set), as the compressor writes them.  Returns a dict: btype (0 stored,
    1 fixed, 2 dynamic); for a dynamic block hlit / hdist / hclen (the raw fields), n_litlen / n_dist / n_cl (the counts),
    cl_lengths (19, by symbol), ll_lengths (n_litlen), d_lengths (n_dist); tokens: (position, literal) or
    (position, length, distance); out: the bytes the block stands for; used: bytes of raw consumed."""
    bits = _Bits(raw)
    assert bits.take(1) == 1, "one final block expected"
    btype = bits.take(2)
    r = {"btype": btype, "tokens": []}
    if btype == 0:
        bits.take(bits.n & 7)
        ln, nl = bits.take(16), bits.take(16)
        assert ln ^ nl == 0xffff
        at = bits.bytes_used()
        r["out"], r["used"] = bytes(raw[at:at + ln]), at + ln
        assert len(r["out"]) == ln
        return r
    assert btype == 2, "the compressor writes stored and dynamic blocks only"
    hlit, hdist, hclen = bits.take(5), bits.take(5), bits.take(4)
    cl = [0] * 19
    for k in range(hclen + 4):
        cl[_CL_ORDER[k]] = bits.take(3)
    cl_table, lens = _decoder(cl), []
    while len(lens) < hlit + 257 + hdist + 1:
        s = _symbol(bits, cl_table)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits.take(2))
        elif s == 17:
            lens += [0] * (3 + bits.take(3))
        else:
            lens += [0] * (11 + bits.take(7))
    assert len(lens) == hlit + 257 + hdist + 1
    ll, dl = lens[:hlit + 257], lens[hlit + 257:]
    r.update(hlit=hlit, hdist=hdist, hclen=hclen, n_litlen=hlit + 257, n_dist=hdist + 1, n_cl=hclen + 4, cl_lengths=cl,
             ll_lengths=ll, d_lengths=dl)
    lt, dt = _decoder(ll), _decoder(dl)
    out, toks = bytearray(), r["tokens"]
    while True:
        s = _symbol(bits, lt)
        if s < 256:
            toks.append((len(out), s))
            out.append(s)
        elif s == 256:
            break
        else:
            ln = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
            d = _symbol(bits, dt)
            dist = _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])
            assert dist <= len(out)
            toks.append((len(out), ln, dist))
            for _ in range(ln):
                out.append(out[-dist])
    r["out"], r["used"] = bytes(out), bits.bytes_used()
    return r


def optimal_depth(freqs):
    """Depth of an unrestricted Huffman code for the non-zero frequencies (of equal weights the shallower subtree merges first:
    the least depth an optimal code can have)."""
    h = [(f, 0) for f in freqs if f]
    heapq.heapify(h)
    while len(h) > 1:
        (fa, da), (fb, db) = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (fa + fb, max(da, db) + 1))
    return h[0][1]


def litlen_frequencies(tokens):
    """What the compressor counted for the literal/length alphabet: the tokens and the end-of-block symbol."""
    f = [0] * 286
    for t in tokens:
        if len(t) == 2:
            f[t[1]] += 1
        else:
            f[257 + max(k for k in range(29) if _LEN_BASE[k] <= t[1])] += 1
    f[256] = 1
    return f


def length_symbol(ln):
    return 257 + max(k for k in range(29) if _LEN_BASE[k] <= ln)


def dist_symbol(d):
    return max(k for k in range(30) if _DIST_BASE[k] <= d)


def matches(tokens):
    return [t for t in tokens if len(t) == 3]


# ---------------------------------------------------------------- the payloads
def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _fib(k):
    a, b = 1, 1
    for _ in range(k - 1):
        a, b = b, a + b
    return a


def de_bruijn(k, n):
    """B(k, n) over 0 .. k-1: every n-gram once (cyclically), so every n-gram of a prefix is unique."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def flood(geom):
    """a. The model's "match flood" law: 4-byte words drawn from 512 values, each written twice; a block and a ragged tail.  That
    is a match every eight bytes: 512 a segment of the 0x7f00 geometry, against 320, but 8,160 a block of the 0xff00 geometry,
    against 8,192.  There the list is filled in two stretches: 38,000 bytes of a de Bruijn sequence B(9, 5) (every 4-gram repeats,
    no 5-gram does: a match of 4 at every step, about 8,100 of them), then 41-byte units — one of 24 words of 40 bytes and a byte
    of noise — in which a match of 40 straddles nearly every piece boundary, so that the piece at which the list is full begins
    with positions that an earlier match covers (and that have lengths of their own, if their extender ran ahead)."""
    rng = np.random.default_rng(4000 + geom)
    n = CUT[geom] + 1000
    if geom == 32:
        w = rng.integers(0, 512, n // 8 + 1, dtype=np.uint32)
        return np.repeat(w, 2).astype("<u4").tobytes()[:n]
    out = (np.array(de_bruijn(9, 5)[:38000], np.uint8) + 0xA0).astype(np.uint8).tobytes()
    words = [rng.integers(0, 128, 40, dtype=np.uint8).tobytes() for _ in range(24)]
    while len(out) < 52000:
        out += words[int(rng.integers(0, 24))] + bytes([int(rng.integers(0, 128))])
    return out + rng.integers(0, 256, n - len(out), dtype=np.uint8).tobytes()


def acgt(geom):
    """a. Random ACGT, a block and a byte: about eight bytes a match, which comes within 64 records of the 0xff00 geometry's list."""
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(4050 + geom).integers(0, 4, CUT[geom] + 1)].tobytes()


def gate(extra_zero):
    """b. 300 bytes of noise at 0 and again at 32,768 (+ 1 for the twin), zeros between and behind, to the block size."""
    a = bytes([7]) + _noise(4100, 299)
    second = 32768 + extra_zero
    return a + bytes(second - 300) + a + bytes(0xff00 - second - 300)


C_PREFIX = {64: 0, 32: 7200}


def run_case(geom, k, r):
    """c. A run of one byte of 1 + 258 k + r bytes, at the block's end.  In the 0x7f00 geometry a match ends with its segment and
    a short block's segments are shorter than a match, so there 7200 bytes of noise stand in front: the last segment then begins
    inside the noise (at 6720 or 7168) and holds the whole run."""
    return _noise(4200 + geom, C_PREFIX[geom]) + bytes([0x55]) * (1 + 258 * k + r)


# d. period-11 data whose length leaves 0, 1, 3, 4, 5, 63 positions in the last piece, near 1 KB and near the block size.  The
# lengths are the nearest below 1088 / the block size at which the last match is at least MIN_MATCH long (a shorter rest stays
# literals in either geometry and could not end at n): see reach().
D_LENGTHS = {
    64: [1024, 1025, 1027, 1028, 1029, 1087, 0xff00, 0xff00 - 63, 0xff00 - 61, 0xff00 - 60, 0xff00 - 59, 0xff00 - 1],
    32: [1024, 1025, 1027, 1028, 1029, 1087, 0x7f00, 0x7f00 - 63, 0x7f00 - 61, 0x7f00 - 60, 0x7f00 - 59, 0x7f00 - 1],
}


def period11(n):
    return bytes((37 * (i % 11) + 11) & 255 for i in range(n))


def leonardo(i):
    """1, 1, 3, 5, 9, 15, 25, ...: L(i) = L(i-1) + L(i-2) + 1 = 2 Fib(i+1) - 1."""
    return 2 * _fib(i + 1) - 1


E_TOP = {64: 18, 32: 16}          # the chain's symbols: byte value 2 i + 1 occurs leonardo(i) times, i = 0 .. E_TOP
E_FLOOD = {64: 42000, 32: 2600}   # bytes of a flood: a block's (0xff00), a segment's (0x7f00, eight of them)


def fibonacci(geom):
    """e. Symbols whose counts grow like Fibonacci's numbers need codes of more than 15 bits — if those counts are the counts
    of TOKENS.  As bytes of a payload they are not: symbols that skewed repeat their 4-grams (the five most frequent fill nine
    positions of ten, and have 625 4-grams between them), so most of the frequent ones leave in matches, and a shuffled payload
    with the counts Fib(1) .. Fib(22) reaches a depth of 14 through the model.  And Fibonacci's own numbers tie at every merge
    once the end-of-block symbol adds its 1, so that a shallow optimal code exists (depth 9 for 17 symbols).  So: the counts are
    Leonardo's numbers (Fibonacci's growth, every merge decided), and the symbols stand where the compressor takes no match —
    behind a flood that has filled the match list (a de Bruijn sequence B(k, 5): every 4-gram repeats, no 5-gram does, a match
    of 4 at every step).  The 0xff00 geometry has one list a block, the 0x7f00 geometry one a segment of 4096 bytes: there every
    segment begins with its flood."""
    m = E_TOP[geom]
    chain = np.concatenate([np.full(leonardo(i), 2 * i + 1, np.uint8) for i in range(m + 1)])
    np.random.default_rng(4400 + geom).shuffle(chain)
    chain = chain.tobytes()
    k = 9 if geom == 64 else 5
    flood = (np.array(de_bruijn(k, 5)[:E_FLOOD[geom]], np.uint8) + 0xA0).astype(np.uint8).tobytes()
    if geom == 64:
        return flood + chain
    out, at, zone = b"", 0, 4096 - len(flood)
    for _ in range(N_SEG):
        z = chain[at:at + zone]
        at += zone
        out += flood + z + bytes([2 * m + 1]) * (zone - len(z))  # (the most frequent symbol fills what is left)
    assert at >= len(chain)
    return out[:CUT[32]]


def no_match(n):
    """f. A prefix of a de Bruijn sequence B(16, 4) on 16 byte values: compressible (4 bits a byte) and every 4-gram unique."""
    seq = np.array(de_bruijn(16, 4)[:n], np.uint8)
    return (seq * 13 + 3).astype(np.uint8).tobytes()


G_FAR = 1025  # distances from here on are nested: the sources side by side, the copies behind


def alphabets(geom):
    """g. All 256 literals (a permutation), then a run for every length symbol a match can have (258 .. 285: a run of L + 1
    equal bytes is a literal and a match of L at distance 1), then a pair for every distance symbol in reach: six bytes at
    64 m - d and again at 64 m (a periodic stretch where d < 6).  The copy begins a piece because a piece's lookups see none of its
    own positions (and the 0x7f00 geometry tries only the distances 1 and 2 directly).  Zeros between — they churn one bucket
    only, so the far sources stay in the table —, unique non-zero bytes around runs and chunks so that a match is what was built
    and nothing else.  The 0x7f00 geometry reaches back through its segment (4096 bytes of a full block) and 1 KB in front of it:
    its far pairs lie in one segment, up to distance symbol 23."""
    rng = np.random.default_rng(4600 + geom)
    out = bytearray(rng.permutation(256).astype(np.uint8).tobytes())
    fresh = iter(rng.permutation(np.arange(1, 256)).tolist() * 4)
    for k in range(1, 29):
        out += bytes([next(fresh)]) + bytes([k]) * (_LEN_BASE[k] + 1)
    out += bytes([next(fresh)])
    top = 30 if geom == 64 else 24
    dist = [_DIST_BASE[k] + (_DIST_BASE[k] >= 5) for k in range(top)]  # (the second distance of a class where it has two)

    def pair_bytes(d):
        if d < 6:
            per = bytes(rng.choice(np.arange(1, 256), d, replace=False).astype(np.uint8))
            return (per * 8)[:d + 6]
        return None
    for k in range(top):
        d = dist[k]
        if d >= G_FAR:
            break
        at = (len(out) + 1 + d + 63) // 64 * 64  # where the copy begins
        out += bytes(at - d - 1 - len(out)) + bytes([next(fresh)])
        if d < 6:
            out += pair_bytes(d) + bytes([next(fresh)])
        else:
            c = bytes(rng.choice(np.arange(1, 256), 6, replace=False).astype(np.uint8))
            out += c + (bytes([next(fresh)]) + bytes(d - 7) if d > 6 else b"") + c + bytes([next(fresh)])
        assert len(out) == at + 7, (k, d, len(out), at)
    far = [k for k in range(top) if dist[k] >= G_FAR]
    if geom == 32:
        out += bytes((len(out) + 4095) // 4096 * 4096 - len(out))  # the far pairs within one segment
    src = []
    for k in far:
        c = bytes(rng.choice(np.arange(1, 256), 6, replace=False).astype(np.uint8))
        src.append((len(out) + 1, c))
        out += bytes([next(fresh)]) + c + bytes([next(fresh)]) + bytes(8)
    for k, (s0, c) in zip(far, src):
        hi = _DIST_BASE[k + 1] - 1 if k < 29 else 32768
        at = (s0 + _DIST_BASE[k] + 63) // 64 * 64
        assert len(out) < at and _DIST_BASE[k] <= at - s0 <= hi, (k, len(out), at, s0)
        out += bytes(at - len(out)) + c + bytes([next(fresh)])
    n = CUT[geom]
    assert len(out) <= n, len(out)
    return bytes(out) + bytes(n - len(out))


# h. Noise and a tail of zeros: the tail lengths at which the CPU model's stream is stored (bytes > n + 5) and, one zero more,
# dynamic.  Found by bisect_stored_tail() on the model, which is the reference; reach() checks them.
H_TAILS = {64: {0xff00: 55, 1000: 55}, 32: {0x7f00: 41, 1000: 56}}


def stored_case(geom, n, tail):
    return _noise(4700 + geom + n, n)[:n - tail] + bytes(tail)


def bisect_stored_tail(geom, n, model):
    """The tail t such that model(stored_case(geom, n, t)) is a stored block and ... (.., t + 1) a dynamic one.
    model(payload) -> the raw stream of a one-block payload."""
    lo, hi = 0, n - 1  # stored at lo (noise alone), dynamic at hi
    assert model(stored_case(geom, n, lo))[0] & 6 == 0 and model(stored_case(geom, n, hi))[0] & 6 == 4
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if model(stored_case(geom, n, mid))[0] & 6 == 0:
            lo = mid
        else:
            hi = mid
    return lo


SEAM_BOUNDARIES = [1, 4, 7]  # the first, a middle and the last boundary of a full block's eight segments (4096 bytes each)


def seams():
    """i. (0x7f00) At each of three segment boundaries b: 200 bytes of noise at b - 3000 and again at b - 100, zeros elsewhere.  The
    copy's match is cut at b; the next segment's table holds the 1 KB in front of b, not the source, so its first 100 positions
    are literals of its own parse and the seam gives them back to the match."""
    out = bytearray(0x7f00)
    for k, s in enumerate(SEAM_BOUNDARIES):
        b = s * 4096
        c = bytes([9]) + np.random.default_rng(4800 + k).integers(1, 256, 199, dtype=np.uint8).tobytes()
        out[b - 3000:b - 2800] = c
        out[b - 100:b + 100] = c
    return bytes(out)


J_GRAM = bytes([0xC1, 0xC2, 0xC3, 0xC4])
# (position of the 4-gram, the bytes behind it): eight occurrences in eight pieces, more than 8 apart.  What follows an
# occurrence says which earlier one would give the longer match if the 4-way bucket still held it.
J_SPREAD = [(100, b"ab"), (230, b"c"), (370, b"d"), (480, b"e!"), (650, b"f"), (790, b"ab"), (860, b"c#"), (940, b"e!")]
# four occurrences in ONE piece (positions 128 .. 191), 16 apart, and one later
J_PIECE = [(130, b"m"), (146, b"n"), (162, b"pq"), (178, b"r"), (300, b"pq")]


def bucket_case(places):
    out = bytearray(1000)
    for k, (at, tag) in enumerate(places):
        out[at - 1:at + 4 + len(tag) + 1] = bytes([0xE0 + k]) + J_GRAM + tag + bytes([0xF0 + k])
    return bytes(out)


def build_edge_cases(geom):
    cut = CUT[geom]
    cases = {"a flood": flood(geom)}
    if geom == 64:
        cases["a acgt"] = acgt(geom)
        cases["b gate 32768"] = gate(0)
        cases["b gate 32769"] = gate(1)
    for k in (1, 3):
        for r in range(5):
            cases["c run k=%d r=%d" % (k, r)] = run_case(geom, k, r)
    for n in D_LENGTHS[geom]:
        cases["d period 11 n=%d" % n] = period11(n)
    cases["e fibonacci"] = fibonacci(geom)
    cases["f no match %d" % cut] = no_match(cut)
    cases["f no match 4096"] = no_match(4096)
    cases["g alphabets"] = alphabets(geom)
    for n, t in H_TAILS[geom].items():
        cases["h stored n=%d" % n] = stored_case(geom, n, t)
        cases["h dynamic n=%d" % n] = stored_case(geom, n, t + 1)
    if geom == 32:
        cases["i seams"] = seams()
    cases["j bucket spread"] = bucket_case(J_SPREAD)
    cases["j bucket one piece"] = bucket_case(J_PIECE)
    return cases


CAP_CASES = {64: ["a flood", "a acgt"], 32: ["a flood"]}  # the cases that fill a match list (tests/test_gpu_bgzf_edges.py compresses them three times)


# ---------------------------------------------------------------- the reach conditions
def reach(geom, name, payload, streams):
    """Asserts that the case reached its edge, on the parsed streams (one per block of the payload) of the CPU model."""
    cut = CUT[geom]
    blocks = [payload[o:o + cut] for o in range(0, len(payload), cut)]
    parsed = [deflate_tokens(s) for s in streams]
    assert len(parsed) == len(blocks)
    for p, s, b in zip(parsed, streams, blocks):
        assert p["out"] == b and p["used"] == len(s), name
    p0, n0 = parsed[0], len(blocks[0])
    toks = p0["tokens"]
    ms = matches(toks)
    kind = name.split()[0]
    if kind == "a":
        assert p0["btype"] == 2
        if geom == 64:
            assert CAP[64] - 64 < len(ms) <= CAP[64], len(ms)
            last = ms[-1]
            assert n0 - (last[0] + last[1]) >= 259 and all(len(t) == 2 for t in toks if t[0] >= last[0] + last[1])
        else:
            n_pieces = (n0 + 63) // 64
            seg_bytes = 64 * ((n_pieces + N_SEG - 1) // N_SEG)
            full = 0
            for s in range(N_SEG):
                mine = [m for m in ms if m[0] // seg_bytes == s]
                seg_end = min(n0, (s + 1) * seg_bytes)
                if CAP[32] - 64 < len(mine) <= CAP[32] and seg_end - (mine[-1][0] + mine[-1][1]) >= 259:
                    full += 1
                assert len(mine) <= CAP[32], (s, len(mine))
            assert full >= 2, full
    elif kind == "b":
        if name.endswith("32768"):
            assert any(m[2] == 32768 and m[1] >= 200 for m in ms)
        else:
            assert all(m[2] <= 32768 for m in ms)
            lit = {t[0] for t in toks if len(t) == 2}
            assert all(q in lit for q in range(32769, 32769 + 300))
        assert p0["btype"] == 2
    elif kind == "c":
        k, r = int(name.split("k=")[1][0]), int(name.split("r=")[1])
        at = C_PREFIX[geom]
        tail = [t for t in toks if t[0] >= at]
        want = [(at, 0x55)] + [(at + 1 + 258 * j, 258, 1) for j in range(k)]
        want += [(at + 1 + 258 * k, 4, 1)] if r == 4 else [(at + 1 + 258 * k + j, 0x55) for j in range(r)]
        assert p0["btype"] == 2 and tail == want, (tail, want)
    elif kind == "d":
        assert p0["btype"] == 2 and ms and ms[-1][0] + ms[-1][1] == n0 and toks[-1] == ms[-1]
    elif kind == "e":
        f = litlen_frequencies(toks)
        assert p0["btype"] == 2
        assert optimal_depth(f) > 15, optimal_depth(f)
        assert max(p0["ll_lengths"]) == 15
        assert sum(2 ** (15 - l) for l in p0["ll_lengths"] if l) == 2 ** 15
        assert [s for s, l in enumerate(p0["ll_lengths"]) if l] == [s for s, c in enumerate(f) if c]
        for i in range(E_TOP[geom]):  # the chain's symbols stayed literals, every one of them
            assert f[2 * i + 1] == leonardo(i), (i, f[2 * i + 1])
    elif kind == "f":
        # no match token and no distance code in use; the header still carries TWO distance code lengths (HDIST field 1), as
        # zlib's own deflate sends for a block without matches, for inflaters that expect a complete code
        assert p0["btype"] == 2 and not ms and p0["hdist"] == 1 and p0["d_lengths"] == [1, 1]
    elif kind == "g":
        assert p0["btype"] == 2 and p0["n_litlen"] == 286
        assert {length_symbol(m[1]) for m in ms} == set(range(258, 286))  # (257 is a match of 3: below MIN_MATCH)
        assert len({t[1] for t in toks if len(t) == 2}) == 256
        # every distance symbol: all 30 in the 0xff00 geometry, the 24 a segment and its seed can hold in the 0x7f00 geometry
        assert p0["n_dist"] == (30 if geom == 64 else 24) and {dist_symbol(m[2]) for m in ms} == set(range(p0["n_dist"]))
    elif kind == "h":
        if name.split()[1] == "stored":
            assert p0["btype"] == 0 and len(streams[0]) == n0 + 5
        else:
            assert p0["btype"] == 2 and n0 + 5 - 16 <= len(streams[0]) <= n0 + 5, (len(streams[0]), n0 + 5)
    elif kind == "i":
        for s in SEAM_BOUNDARIES:
            b = s * 4096
            assert any(m[0] < b < m[0] + m[1] for m in ms), b
    elif kind == "j":
        places = J_SPREAD if name.endswith("spread") else J_PIECE
        at = {t[0]: t for t in toks}
        pos = [q for q, _ in places]
        g0 = J_GRAM[0]
        if name.endswith("spread"):
            # the bucket holds the four newest occurrences.  The second to the fifth find the one before them.
            for k in range(1, 5):
                assert at[pos[k]] == (pos[k], 4, pos[k] - pos[k - 1])
            # The sixth goes on like the first, which has left the bucket: four bytes at the newest — and it yields to the five
            # bytes that the gram one position on (a bucket of its own, without pressure) finds at the first.  Had the first
            # stayed: six bytes at once, (pos, 6, pos - first).
            assert at[pos[5]] == (pos[5], g0) and at[pos[5] + 1] == (pos[5] + 1, 5, pos[5] - pos[0])
            # the seventh goes on like the second (gone too) for one byte only: four bytes at the newest
            assert at[pos[6]] == (pos[6], 4, pos[6] - pos[5])
            # the eighth goes on like the fourth, the oldest the bucket still holds: six bytes there
            assert at[pos[7]] == (pos[7], 6, pos[7] - pos[3])
        else:
            # a piece's lookups see none of its own positions: its four occurrences are literals
            for q in pos[:4]:
                assert at[q] == (q, g0)
            # of the piece's four lanes on the bucket the last stays: the later occurrence goes on like the third but finds four
            # bytes at the fourth, and yields to the five bytes the next gram finds at the third.  Had the third stayed: (pos, 6, ..).
            assert at[pos[4]] == (pos[4], g0) and at[pos[4] + 1] == (pos[4] + 1, 5, pos[4] - pos[2])
    else:
        raise AssertionError("no reach condition for %r" % name)
