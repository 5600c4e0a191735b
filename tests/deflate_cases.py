"""The hand-built DEFLATE corpus (tests/deflate_builder.py does the writing): streams that are legal RFC 1951 and that
zlib's deflate never writes, and a fixed list of streams that zlib's inflate refuses.  Fixed seeds; every case is
(name, raw stream, verdict, payload).  For a valid case the payload is what zlib inflates the stream to (asserted here);
for an invalid case it is the payload the member's trailer claims (CRC32 and ISIZE are made from it, so that a lenient
decoder is caught by its verdict, not saved by the CRC), and zlib's verdict is "error" or "truncated" (asserted here).

Three things in the corpus follow from the formats and not from a choice:
  * HCLEN = 4 admits only the code-length symbols 16, 17, 18 and 0, so every length it can write is 0 and the block has
    no end-of-block code: that header is in the invalid list; the valid ones run from 5 to 19.
  * A stored block of 65535 or 65536 bytes does not fit a BGZF member (BSIZE < 65536 with 26 bytes of frame), so the
    "stored" payloads of these two sizes are 60000 bytes of stored blocks and a run of matches behind them.
  * The longest distance DEFLATE can write is 32768, so "one byte beyond what was written" is not expressible at
    position 40000; it is taken at positions 0, 20000 and 32767."""
import functools
import os
import struct
import subprocess
import zlib

import numpy as np

import deflate_builder as B

A, Z = ord("a"), ord("z")
FADE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fade_amd", "fade")
EOF_MARK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _lits(data):
    return list(bytes(data))


def _flat(n_symbols, used):
    return B.assign(n_symbols, list(used), B.complete_shape(len(used)))


def _shaped(n_symbols, used_short_first, longest):
    return B.assign(n_symbols, list(used_short_first), B.complete_shape(len(used_short_first), longest))


def _run_matches(n):
    """(length, 1) tokens adding up to n bytes (n = 0 or n >= 3)."""
    out = []
    while n:
        take = 258 if n >= 261 or n == 258 else (n if n <= 258 else n - 3)
        out.append((take, 1))
        n -= take
    return out


# ------------------------------------------------------------------ a composer that encodes a GIVEN payload
def _parse(payload, start, end, rng, p_match):
    tokens, i = [], start
    while i < end:
        if i >= 1 and end - i >= 3 and rng.random() < p_match:
            j = payload.rfind(payload[i:i + 3], max(0, i - 32768), i + 2)
            if j >= 0:
                cap = min(int(rng.integers(3, 259)), end - i)
                n = 3
                while n < cap and payload[j + n] == payload[i + n]:
                    n += 1
                tokens.append((n, i - j))
                i += n
                continue
        tokens.append(payload[i])
        i += 1
    return tokens


def _random_lens(n_alphabet, freq, rng, longest, n_spare, by_freq):
    """A complete set over the used symbols and a few unused ones; lengths shuffled unless by_freq."""
    syms = sorted(freq, key=lambda s: -freq[s])
    spare = [s for s in rng.permutation(n_alphabet).tolist() if s not in freq][:n_spare]
    syms += spare
    n = len(syms)
    lo, hi = (n - 1).bit_length(), min(15, n - 1)
    want = int(rng.integers(lo, hi + 1)) if longest == "random" else (lo if longest is None else min(max(longest, lo), hi))
    if not by_freq:
        syms = [syms[k] for k in rng.permutation(n).tolist()]
    return B.assign(n_alphabet, syms, B.complete_shape(n, want))


def encode(payload, rng, kinds=("stored", "fixed", "dynamic"), max_blocks=12, lit_longest="random", dist_longest="random",
           cl_longest="random", rle=None, p_match=0.3, by_freq=None, full_alphabets=False):
    """`payload` as one DEFLATE stream of 1..max_blocks blocks of random kind, with random complete code-length sets."""
    payload = bytes(payload)
    by_freq = len(payload) > 12000 if by_freq is None else by_freq
    n_blocks = int(rng.integers(1, max_blocks + 1))
    cuts = sorted(int(c) for c in rng.integers(0, len(payload) + 1, n_blocks - 1)) + [len(payload)]
    s, at = B.Stream(), 0
    for b, end in enumerate(cuts):
        final = b == len(cuts) - 1
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == "stored" and end - at <= 65535:
            s.stored(payload[at:end], final)
        else:
            tokens = _parse(payload, at, end, rng, p_match)
            if kind != "dynamic":
                s.payload = bytearray(payload[:at])
                s.fixed(tokens, final)
            else:
                lf, df = {256: 1}, {}
                for t in tokens:
                    if isinstance(t, int):
                        lf[t] = lf.get(t, 0) + 1
                    else:
                        ls, ds = B.length_symbol(t[0])[0], B.dist_symbol(t[1])[0]
                        lf[ls] = lf.get(ls, 0) + 1
                        df[ds] = df.get(ds, 0) + 1
                if len(lf) == 1:
                    lit_lens = B.lone_code(257, 256) if rng.random() < 0.5 else _flat(286, [256, 0])
                else:
                    lit_lens = _random_lens(286, lf, rng, lit_longest, int(rng.integers(0, 6)), by_freq)
                if not df:
                    pick = int(rng.integers(0, 3))
                    dist_lens = B.no_code(1) if pick == 0 else B.lone_code(30, int(rng.integers(0, 30))) if pick == 1 else _random_lens(30, {0: 1, 5: 1}, rng, dist_longest, 3, by_freq)
                elif len(df) == 1 and rng.random() < 0.5:
                    dist_lens = B.lone_code(30, next(iter(df)))
                else:
                    if len(df) == 1:
                        df[(next(iter(df)) + 7) % 30] = 0
                    dist_lens = _random_lens(30, df, rng, dist_longest, int(rng.integers(0, 4)), by_freq)
                if not full_alphabets:
                    hlit = int(rng.integers(max(257, max(k for k in range(len(lit_lens)) if lit_lens[k]) + 1), 287))
                    hdist = int(rng.integers(max(1, max([k for k in range(len(dist_lens)) if dist_lens[k]] + [0]) + 1), 31))
                    lit_lens, dist_lens = (list(lit_lens) + [0] * 30)[:hlit], (list(dist_lens) + [0] * 30)[:hdist]
                mode = rle or ("none", "greedy", "long")[int(rng.integers(0, 3))]
                seq = B.rle_code_lengths(lit_lens, dist_lens, mode)
                cf = {}
                for sym, _ in seq:
                    cf[sym] = cf.get(sym, 0) + 1
                if len(cf) == 1:
                    cf[(next(iter(cf)) + 1) % 19] = 0
                cl_lens = _random_lens(19, cf, rng, cl_longest if cl_longest is None or cl_longest == "random" else min(cl_longest, 7),
                                       int(rng.integers(0, 3)), len(seq) > 150)
                if max(cl_lens) > 7:  # (the code-length code has 3-bit lengths)
                    cl_lens = _random_lens(19, cf, rng, 7, 0, len(seq) > 150)
                lo = max([4] + [k + 1 for k in range(19) if cl_lens[B.CL_ORDER[k]]])
                s.payload = bytearray(payload[:at])
                s.dynamic(tokens, final, lit_lens, dist_lens, cl_lens=cl_lens, hclen=int(rng.integers(lo, 20)), cl_sequence=seq)
        assert bytes(s.payload) == payload[:end], "the composer's own parse went wrong"
        at = end
    return s


def encode_incomplete(payload, rng, which):
    """`payload` as one dynamic block whose code-length / literal-length / distance set (`which`) is INCOMPLETE: a complete
    set over the symbols the data uses and one more, whose code is then taken away.  The missing code never occurs in the
    data and the payload is right, so only an inflater that checks the set as zlib does refuses the stream."""
    payload = bytes(payload)
    tokens = _parse(payload, 0, len(payload), rng, 0.5)
    lf, df = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
        else:
            ls, ds = B.length_symbol(t[0])[0], B.dist_symbol(t[1])[0]
            lf[ls] = lf.get(ls, 0) + 1
            df[ds] = df.get(ds, 0) + 1
    assert len(df) >= 2, "the payload has no repeats to speak of"

    def with_spare(n_alphabet, freq, drop):
        spare = next(s for s in range(n_alphabet) if s not in freq)
        lens = _random_lens(n_alphabet, {**freq, spare: 0}, rng, None, 0, True)
        if drop:
            lens[spare] = 0
        return lens

    lit_lens, dist_lens = with_spare(286, lf, which == "literal_length"), with_spare(30, df, which == "distance")
    seq = B.rle_code_lengths(lit_lens, dist_lens, "greedy")
    cf = {}
    for sym, _ in seq:
        cf[sym] = cf.get(sym, 0) + 1
    s = B.Stream().dynamic(tokens, True, lit_lens, dist_lens, cl_lens=with_spare(19, cf, which == "code_length"), cl_sequence=seq)
    v = B.expected(s.raw())
    message = {"code_length": "invalid code lengths set", "literal_length": "invalid literal/lengths set", "distance": "invalid distances set"}[which]
    assert bytes(s.payload) == payload and v[0] == "error" and message in v[1], (which, v)
    return s


def random_payload(rng, n):
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == 1:
        return rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
    if kind == 2:
        p = 0.6 ** np.arange(1, 61)
        return rng.choice(np.arange(60, dtype=np.uint8), n, p=p / p.sum()).tobytes()
    if kind == 3:
        unit = rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes()
        return (unit * (n // len(unit) + 1))[:n]
    if kind == 4:
        return bytes(n)
    parts, left = [], n
    while left:
        k = min(left, int(rng.integers(1, 600)))
        parts.append(random_payload(rng, k))
        left -= k
    return b"".join(parts)


N_RANDOM_MEMBERS = 300


def random_members(seed=20260, count=N_RANDOM_MEMBERS):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        u = rng.random()
        n = int(rng.integers(0, 300)) if u < 0.3 else int(rng.integers(300, 9000)) if u < 0.9 else int(rng.integers(9000, 65537))
        payload = random_payload(rng, n)
        s = encode(payload, rng)
        if len(s.raw()) > 65000:  # (would not fit a member: the same payload with the short codes on the frequent symbols)
            s = encode(payload, rng, by_freq=True, lit_longest=None, dist_longest=None)
        out.append(("random_%03d" % k, s.raw(), payload))
    return out


# header shapes of section 1 that can carry any payload (the file-path tests re-encode BAM records with them)
SHAPES = {
    "no_repeats_hclen_19": dict(kinds=("dynamic",), rle="none", full_alphabets=True, cl_longest=None),
    "repeats_across_the_seam": dict(kinds=("dynamic",), rle="long", full_alphabets=True),
    "cl_code_7_bits": dict(kinds=("dynamic",), rle="greedy", cl_longest=7, lit_longest=15),
    "lit_15_dist_15": dict(kinds=("dynamic",), lit_longest=15, dist_longest=15, p_match=0.6),
    "lit_9_dist_9": dict(kinds=("dynamic",), lit_longest=9, dist_longest=9, p_match=0.6),
    "literals_only": dict(kinds=("dynamic",), p_match=0.0, max_blocks=3),
    "fixed_blocks": dict(kinds=("fixed",), p_match=0.5),
    "stored_and_fixed": dict(kinds=("stored", "fixed"), max_blocks=12),
    "one_block_each_kind": dict(kinds=("stored", "fixed", "dynamic"), max_blocks=3, p_match=0.8),
}


# ------------------------------------------------------------------ the named valid cases
def _named_valid():
    rng = np.random.default_rng(1951)
    cases = []

    def add(name, s, tail=b""):
        cases.append((name, s.raw() + tail, bytes(s.payload)))

    noise = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()

    # -- 1. header shapes
    # 256 codes of 8 bits (0..254 and 256): the lengths are 8 and 0 only, so the header's code-length code needs the
    # symbols 8, 16 and 0; one more symbol with a code (never used) sets HCLEN to any value from 5 to 19.
    lit8 = [8] * 255 + [0, 8]
    for hclen in range(5, 20):
        seq = B.rle_code_lengths(lit8, [0], "greedy")
        used = sorted(set(q for q, _ in seq))
        last = B.CL_ORDER[hclen - 1]
        syms = used + ([last] if last not in used else [])
        s = B.Stream().dynamic(_lits(b"HCLEN %d" % hclen), True, lit8, [0], cl_lens=_flat(19, syms), cl_sequence=seq)
        assert s.hclen == hclen
        add("hclen_%d" % hclen, s)
    # code-length codes of 7 bits: a literal/length set with the lengths 1..12 in it, so that 13 and more code-length
    # symbols are used
    lit12 = _shaped(286, list(range(A, A + 26)) + list(range(48, 58)) + [256, 257, 270, 285], 12)
    dist7 = _shaped(30, list(range(0, 12)), 7)
    seq = B.rle_code_lengths(lit12, dist7, "greedy")
    used = sorted(set(q for q, _ in seq), key=lambda q: -sum(1 for r, _ in seq if r == q))
    assert len(used) >= 8
    cl7 = _shaped(19, used, 7)
    s = B.Stream().dynamic(_lits(b"abcdefghijklmnopqrstuvwxyz0123456789") + [(3, 5), (24, 17), (258, 40)] + _lits(b"zz99"), True, lit12, dist7,
                           cl_lens=cl7, cl_sequence=seq)
    assert max(cl7) == 7 and any(cl7[q] == 7 for q, _ in seq)
    add("cl_code_7_bits", s)

    # repeats that run across the HLIT / HDIST seam
    def crosses(s, hlit, sym):
        return any(q == sym and a < hlit < a + n for (q, _), (a, n) in zip(s.cl_sequence, B.cl_spans(s.cl_sequence)))

    lits = list(range(A, A + 8))
    lit = _flat(260, lits + [256, 257, 258, 259])  # 257..259 get 4 bits, and so do 16 distance codes
    s = B.Stream().dynamic(_lits(b"abcdefgh") + [(3, 8), (4, 2), (5, 11)] + _lits(b"hg"), True, lit, [4] * 16, rle="long")
    assert crosses(s, 260, 16)
    add("seam_repeat_16", s)
    lit = _flat(265, lits + [256, 257])  # 258..264 are 0, and so are the first three distance codes
    s = B.Stream().dynamic(_lits(b"abcdefgh") + [(3, 4), (3, 5), (3, 6)] + _lits(b"a"), True, lit, [0, 0, 0, 2, 2, 2, 2], rle="long")
    assert crosses(s, 265, 17)
    add("seam_repeat_17", s)
    lit = _flat(286, lits + [256, 257])  # 258..285 are 0 and the first 20 distance codes
    s = B.Stream().stored(noise[:1600]).dynamic(_lits(b"abc") + [(3, 1025), (3, 1536 + 7)] + _lits(b"h"), True, lit, [0] * 20 + [1, 1], rle="long")
    assert crosses(s, 286, 18)
    add("seam_repeat_18", s)
    # the longest repeat (138) and one between 65 and 128, in a block behind a fixed block (whose 288 + 32 lengths are all
    # non-zero: whatever the inflater keeps of them must be overwritten by the zeros)
    lit = _flat(286, [0, 1, 2, 3, 256, 285])
    s = B.Stream().fixed(_lits(b"\x00\x01"), False).dynamic([0, 1, 2, 3, (258, 2), 3, 2], True, lit, [1, 1], rle="greedy")
    assert (18, 127) in s.cl_sequence and any(q == 18 and 64 < 11 + x <= 128 for q, x in s.cl_sequence)
    add("repeat_138_behind_fixed_block", s)
    lit = _flat(286, [0, 1, 2, 3, 200, 256, 260])  # zeros 4..199: 138 + 58; 201..255: 55
    s = B.Stream().fixed(_lits(b"\x00\x01"), False).dynamic([0, 200, 1, 2, 3, (6, 2), 200], True, lit, [0, 1], rle="greedy")
    add("repeat_138_then_58", s)
    lit = [9] * 200 + [0] * 56 + [9] + [9] * 29  # long runs of one non-zero length: code 16 many times over
    lit = lit[:286]
    assert B.kraft_left(lit) > 0
    # top up to a complete code: 230 codes of 9 bits leave room that 8-bit codes on the first symbols fill
    k = 0
    while B.kraft_left(lit) > 0:
        lit[k] = 8
        k += 1
    assert B.kraft_left(lit) == 0
    s = B.Stream().dynamic(_lits(bytes(range(0, 200, 7))) + [(258, 3)], True, lit, [3] * 8, rle="greedy")
    assert sum(1 for q, _ in s.cl_sequence if q == 16) > 30
    add("repeat_16_runs", s)
    # HLIT = 257 and 286, HDIST = 1 (a lone 1-bit code; no code at all) and 30, a literal/length set that is the lone code 256
    add("hlit_257_hdist_1_lone", B.Stream().dynamic(_lits(b"abba"), True, _flat(257, [A, A + 1, 256, 0]), [1]))
    s = B.Stream().dynamic(_lits(b"ab") + [(257, 0, 0, 0), (285, 0, 0, 0), (284, 31, 0, 0)], True, _flat(286, [A, A + 1, 256, 257, 284, 285]), [1])
    add("hlit_286_hdist_1_lone", s)
    add("hdist_1_no_distance_code", B.Stream().dynamic(_lits(b"literals only " * 9), True, _flat(257, sorted(set(b"literals only ")) + [256]), [0]))
    s = B.Stream().stored(noise[:32768]).dynamic(_lits(b"ab") + [(3, 24577), (258, 32768), (9, 1), (3, 32768)], True,
                                                 _flat(286, [A, A + 1, 256, 257, 263, 285]), _shaped(30, [0, 29, 28, 1, 2], 4))
    add("hdist_30_distance_32768", s)
    add("lone_code_256_empty_block", B.Stream().dynamic([], False, B.lone_code(257, 256), [0]).fixed(_lits(b"after the empty block"), True))

    # -- symbols
    f = B.Stream().fixed(_lits(b"x") + [(285, 0, 0, 0)], True)
    add("length_258_as_code_285", f)
    add("length_258_as_code_284_extra_31", B.Stream().fixed(_lits(b"xy") + [(284, 31, 1, 0)], True))
    add("length_3", B.Stream().fixed(_lits(b"abc") + [(3, 3), (3, 1), (3, 2)], True))
    add("distance_1_length_258", B.Stream().fixed(_lits(b"q") + [(258, 1)] * 3, True))
    add("distance_32768_fixed", B.Stream().stored(noise[:32768]).fixed([(258, 32768), (3, 32768), (100, 32767)], True))
    add("match_into_earlier_huffman_block", B.Stream().fixed(_lits(b"first block, "), False).fixed([(13, 13), (5, 20)] + _lits(b"!"), True))
    add("match_into_stored_block", B.Stream().stored(b"stored bytes ").fixed([(13, 13), (6, 26)], True))
    for n in (1, 8, 14, 15, 16, 272, 273, 274, 300):
        add("match_ends_at_isize_after_%d" % n, B.Stream().fixed(_lits(noise[:n]) + [(258, max(1, n // 2))], True))
    add("bytes_behind_the_final_block", B.Stream().fixed(_lits(b"the member goes on"), True), tail=b"\xa5\x5a\xff")

    # -- 2. codes of 9, 10, 11, 12 and 15 bits on literals, on length symbols with extra bits, on distance symbols with 13
    # extra bits; behind a stored block of 33000 bytes, so that every distance is legal
    for longest in (9, 10, 11, 12, 15):
        # short first; the last two get `longest` bits: a literal and length symbol 284 (5 extra bits)
        order = [A, A + 1, A + 2, 256, A + 3, A + 4, A + 5, A + 6, A + 7, A + 8, A + 9, 257, 265, 285, 269, A + 10, A + 11, 273, 277, 282,
                 283, 284, Z, 281]
        lit = _shaped(286, order, longest)
        dist = _shaped(30, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29], longest)
        assert lit[281] == longest and lit[Z] == longest and dist[28] == longest and dist[29] == longest
        s = B.Stream().stored(noise[:33000])
        tokens, phases, bits = [], set(), 0  # (bits: relative to the first match; the GPU test moves the whole stream byte by byte)
        for k in range(400):
            phases.add(bits % 32)
            tokens.append((281, int(rng.integers(0, 32)), 28 + (k & 1), int(rng.integers(0, 8192))))
            bits += 2 * longest + 5 + 13
            # short literals move the next match to a bit of the buffer that has not been met yet
            fill = [A + (j + k) % 12 for j in range(6)]
            reach = [sum(lit[q] for q in fill[:n]) for n in range(7)]
            n = next((n for n in range(7) if (bits + reach[n]) % 32 not in phases), k % 7)
            tokens += fill[:n]
            bits += reach[n]
            if k % 11 == 0:
                tokens += [Z, (283, 7, 13, 5), (3, 1), A + 11, (284, 30, 29, 8191)]
                bits += lit[Z] + lit[283] + 5 + dist[13] + 6 + lit[257] + dist[0] + lit[A + 11] + lit[284] + 5 + dist[29] + 13
            if len(phases) == 32 and k >= 100 and bits > 8 * 640:
                break
        assert len(phases) == 32, "the %d-bit sequence does not meet every position of a 32-bit refill" % longest
        s.dynamic(tokens, True, lit, dist)
        assert len(s.payload) <= 65536 and len(s.raw()) - 33005 > 600, (longest, k, len(s.payload), len(s.raw()))
        add("codes_of_%d_bits" % longest, s)

    # -- 3. block headers at every bit alignment; the final end-of-block code ending on every bit of the last byte
    simple_lit = _flat(286, [A, A + 1, A + 2, 256, 257, 258])
    for kind in ("stored", "fixed", "dynamic"):
        seen = set()
        for m in range(8):
            s = B.Stream().fixed(_lits(b"head") + [200] * m, False)  # (literal 200 takes 9 bits: m of them move the next header bit by bit)
            seen.add(s.bits % 8)
            name = "%s_header_at_bit_%d" % (kind, s.bits % 8)
            if kind == "stored":
                s.stored(b"stored, byte aligned", True)
            elif kind == "fixed":
                s.fixed([(4, 4 + m)] + _lits(b" fixed"), True)
            else:
                s.dynamic([A, A + 1, A + 2, (3, 3), (4, 2 + m)], True, simple_lit, [3] * 8)
            add(name, s)
        assert seen == set(range(8))
    seen = set()
    for m in range(8):
        s = B.Stream().fixed(_lits(b"tail") + [201] * m, True)
        seen.add(s.bits % 8)
        add("final_end_of_block_ends_at_bit_%d" % (s.bits % 8), s)
    assert seen == set(range(8))

    # -- 4. literals pending in front of a stored block, a match, the end of the member
    for n in (0, 1, 63, 64, 65):
        pend = _lits(noise[100:100 + n])
        add("pending_%d_then_stored" % n, B.Stream().stored(b"0123456789").fixed(pend, False).stored(b"<stored>").fixed(_lits(b"."), True))
        add("pending_%d_then_match" % n, B.Stream().stored(b"0123456789").fixed(pend + [(7, 3 + n)] + _lits(b"."), True))
        add("pending_%d_then_end" % n, B.Stream().stored(b"0123456789").fixed(pend, True))

    # -- 5. a stored block whose header, LEN / NLEN and bytes lie on either side of a 256-byte boundary of the stream (the
    # device reader's window turns over there); the four byte alignments are the GPU test's business
    for n in range(244, 263):
        s = B.Stream().fixed(_lits(bytes(k % 128 for k in range(n))), False).stored(noise[500:800])
        s.fixed(_lits(noise[900:1100]) + [(258, 300), (20, 1)] + _lits(b"end"), True)
        add("stored_block_after_%d_stream_bytes" % (n + 2), s)

    # -- 6. payload sizes
    for n in (0, 1, 63, 64, 65):
        add("size_%d" % n, B.Stream().fixed(_lits(noise[2000:2000 + n]), True))
    four = _flat(257, [65, 67, 71, 84, 256])
    for n in (65280, 65535, 65536):
        acgt = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
        add("size_%d_literals_only" % n, B.Stream().dynamic(_lits(acgt), True, four, [0]))
        add("size_%d_one_literal_and_matches" % n, B.Stream().fixed([7] + _run_matches(n - 1), True))
        s = B.Stream().stored(noise[:30000]).stored(noise[5000:35000])
        if n == 65280:
            s.stored(noise[:5280], True)
        else:  # (the member's frame leaves no room for the rest as stored bytes)
            s.fixed(_run_matches(n - 60000), True)
        add("size_%d_stored_blocks" % n, s)

    # -- 7. many blocks
    s = B.Stream()
    for _ in range(500):
        s.fixed([], False)
    add("500_empty_fixed_blocks_then_data", s.fixed(_lits(b"data at last"), True))
    s = B.Stream()
    for _ in range(200):
        s.stored(b"", False)
    add("200_stored_blocks_of_len_0", s.fixed(_lits(b"data at last") + [(3, 5)], True))
    add("one_stored_block_of_len_0", B.Stream().stored(b"", True))
    s = B.Stream().stored(b"seed bytes for the first match")
    for k in range(300):
        chunk = noise[3000 + 40 * k:3000 + 40 * k + 25]
        back = [(int(rng.integers(3, 30)), int(rng.integers(26, 60)))]  # reaches into the block before this one
        if k % 3 == 0:
            s.stored(chunk + b"/", k == 299)
        elif k % 3 == 1:
            s.fixed(back + _lits(chunk), k == 299)
        else:
            syms = sorted(set(chunk)) + [256, B.length_symbol(back[0][0])[0]]
            s.dynamic(back + _lits(chunk), k == 299, _flat(286, syms), _flat(30, [B.dist_symbol(back[0][1])[0], 3]),
                      rle=("none", "greedy", "long")[k % 9 // 3])
    add("300_blocks_alternating_kinds", s)
    return cases


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, raw, "ok", payload)]: the named cases, then the random composer's members."""
    out = []
    for name, raw, payload in _named_valid() + random_members():
        v = B.expected(raw)
        assert v[0] == "ok", (name, v[:2] if v[0] == "error" else v[0])
        assert v[1] == payload, "%s: zlib inflates this stream to other bytes than the builder meant" % name
        assert v[2] == (b"\xa5\x5a\xff" if name == "bytes_behind_the_final_block" else b""), name
        assert len(payload) <= 65536 and len(raw) <= 65536 - 26 - 7, (name, len(raw))  # (fits a member, with a subfield of 7 bytes)
        out.append((name, raw, "ok", payload))
    assert len(set(c[0] for c in out)) == len(out)
    return tuple(out)


# ------------------------------------------------------------------ the invalid cases
@functools.lru_cache(maxsize=None)
def invalid_cases():
    """[(name, raw, "error" | "truncated", claimed payload)].  The comment beside each case names the check of
    bgzf_inflate.hpp's inflate_member that ends it (INF_E_*), read off the kernel before any of them was sent to a device.
    Every loop of the kernel is bounded whatever the bits say: the block loop by `guard` (3 bits a block at least), the
    header's length loop by `k < total`, literals by `pos` against `isize`, matches by `pos + length > isize`, and the
    reader returns zeros beyond the member's last dword — so a case whose tail is decoded from the trailer's bits ends in
    one of the listed checks, whichever the bits select."""
    rng = np.random.default_rng(1952)
    noise = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    ab = _flat(257, [A, A + 1, 256, 0])
    abm = _flat(258, [A, A + 1, 256, 257])
    text = _lits(b"abbaabab")
    cases = []

    def add(name, raw, claimed, by_isize=False):
        raw = raw.raw() if isinstance(raw, B.Stream) else raw
        v = B.expected(raw, isize=len(claimed) if by_isize else None)  # (zlib's own verdict, but for the five cases about ISIZE)
        assert v[0] in ("error", "truncated"), "%s: zlib takes this stream (%d bytes)" % (name, len(v[1]))
        cases.append((name, raw, v[0], bytes(claimed)))

    # INF_E_BTYPE
    add("btype_3", B.Stream().fixed(_lits(b"abc"), False).reserved(), b"abc")
    # INF_E_STORED (len ^ nlen != 0xffff)
    add("stored_nlen_mismatch", B.Stream().stored(b"hello", True, nlen_field=0x1234), b"hello")
    # INF_E_OVERRUN_IN (at + len > in_limit: 1000 bytes claimed, 10 there, 8 bytes of slack)
    add("stored_len_beyond_the_member", B.Stream().stored(noise[:1000], True, body=noise[:10]), noise[:1000])
    # INF_E_HEADER (hlit > 286 || hdist > 30), straight behind the 14 header bits
    for field in (30, 31):
        add("hlit_field_%d" % field, B.Stream().dynamic(text, True, ab, [0], hlit_field=field), b"abbaabab")
        add("hdist_field_%d" % field, B.Stream().dynamic(text, True, ab, [0], hdist_field=field), b"abbaabab")
    # INF_E_HEADER (build_table: left < 0), for each of the three alphabets
    add("code_length_set_oversubscribed", B.Stream().dynamic(text, True, ab, [0], cl_lens=B.assign(19, [0, 2, 18, 17], [1, 1, 1, 2])), b"abbaabab")
    add("literal_length_set_oversubscribed", B.Stream().dynamic(text, True, B.assign(257, [A, A + 1, 256], [1, 1, 1]), [0]), b"abbaabab")
    add("distance_set_oversubscribed", B.Stream().dynamic(text + [(3, 1)], True, abm, [1, 1, 1]), b"abbaabab" + b"bbb")
    # INF_E_HEADER (build_table: left > 0 and not the lone 1-bit code; this is what the kernel used to take).  In all of
    # them the unused part of the code space never occurs in the data and the trailer is right.
    add("code_length_set_incomplete", B.Stream().dynamic(text, True, ab, [0], cl_lens=B.assign(19, [0, 2, 18], [2, 2, 2])), b"abbaabab")
    add("code_length_set_lone_1_bit_code", B.Stream().dynamic([], True, [0] * 257, [0], cl_lens=B.lone_code(19, 18), eob=False,
                                                              cl_sequence=[(18, 127), (18, 109)]), b"")  # (and no code for 256 either way)
    add("literal_length_set_incomplete_unused_code", B.Stream().dynamic(_lits(b"aaaa"), True, B.assign(286, [A, 256, 285], [1, 2, 3]), [0]), b"aaaa")
    add("literal_length_set_incomplete_two_2_bit_codes", B.Stream().dynamic(_lits(b"aaaa"), True, B.assign(257, [A, 256], [2, 2]), [0]), b"aaaa")
    add("literal_length_set_lone_2_bit_code_256", B.Stream().dynamic([], True, B.assign(257, [256], [2]), [0]), b"")
    add("distance_set_incomplete", B.Stream().dynamic(text + [(3, 1)], True, abm, [2, 2, 2]), b"abbaabab" + b"bbb")
    add("distance_set_lone_2_bit_code", B.Stream().dynamic(text + [(3, 1)], True, abm, [2]), b"abbaabab" + b"bbb")
    # INF_E_HEADER (lens[256] == 0)
    add("no_code_for_256", B.Stream().dynamic(text, True, B.assign(257, [A, A + 1], [1, 1]), [0], eob=False), b"abbaabab")
    add("hclen_4_every_length_0", B.Stream().dynamic([], True, [0] * 257, [0], cl_lens=B.assign(19, [18, 0], [1, 1]), eob=False,
                                                    cl_sequence=[(18, 127), (18, 109)]), b"")
    # INF_E_HEADER (sym == 16 with k == 0)
    seq = [(16, 0)] + B.rle_code_lengths(ab, [0], "none")[3:]
    add("code_16_first", B.Stream().dynamic(text, True, ab, [0], cl_sequence=seq), b"abbaabab")
    # INF_E_HEADER (k + rep > total)
    seq = B.rle_code_lengths(ab, [0], "greedy")
    assert seq[-1] == (0, 0) and seq[-2] == (2, 0)  # ... 256: 2 bits, then the distance length 0
    add("repeat_overruns_hlit_plus_hdist", B.Stream().dynamic(text, True, ab, [0], cl_sequence=seq[:-1] + [(17, 0)]), b"abbaabab")
    add("repeat_138_overruns_hlit_plus_hdist", B.Stream().dynamic(text, True, ab, [0], cl_sequence=seq[:-1] + [(18, 127)]), b"abbaabab")
    # INF_E_CODE (sym - 257 >= 29)
    for sym in (286, 287):
        add("fixed_block_symbol_%d" % sym, B.Stream().fixed(_lits(b"abc") + [("sym", sym)], True), b"abc")
    # INF_E_CODE (dsym >= 30)
    for sym in (30, 31):
        add("fixed_block_distance_symbol_%d" % sym, B.Stream().fixed(_lits(b"abc") + [(257, 0, sym, 0)], True), b"abcabc")
    # INF_E_DIST (dist > pos)
    add("distance_1_at_position_0", B.Stream().fixed([(3, 1)] + _lits(b"abc"), True), b"\0\0\0abc")
    add("distance_20001_at_position_20000", B.Stream().stored(noise[:20000]).fixed([(3, 20001)], True), noise[:20000] + b"\0\0\0")
    add("distance_32768_at_position_32767", B.Stream().stored(noise[:32767]).fixed([(3, 32768)], True), noise[:32767] + b"\0\0\0")
    # INF_E_CODE (the distance table is all zeros and canon_decode finds no code)
    add("match_in_a_block_without_distance_code", B.Stream().dynamic(text + [("sym", 257), ("bits", 0, 5)], True, abm, [0]), b"abbaabab" + b"bbb")
    # INF_E_OVERRUN_OUT (a literal with pos >= isize: the literal line's fast path is closed in the last 63 bytes)
    add("one_literal_more_than_isize", B.Stream().fixed(_lits(b"abcdef"), True), b"abcde", by_isize=True)
    add("one_literal_more_than_isize_100", B.Stream().fixed(_lits(noise[:101]), True), noise[:100], by_isize=True)
    # INF_E_OVERRUN_OUT (pos + length > isize)
    add("match_one_byte_beyond_isize", B.Stream().fixed(_lits(b"x") + [(258, 1)], True), b"x" * 258, by_isize=True)
    # INF_E_SIZE (pos != isize after the final block)
    add("one_byte_less_than_isize", B.Stream().fixed(_lits(b"abcdef"), True), b"abcdefg", by_isize=True)
    add("one_byte_less_than_isize_100", B.Stream().fixed(_lits(noise[:99]) + [(3, 7)], True), noise[:99] + noise[92:95] + b"!", by_isize=True)
    # INF_E_STORED: no final block.  The next header is read from the zero bits that pad the last byte (000: a stored
    # block, not final), LEN and NLEN from the four bytes behind the stream, the trailer's CRC32, which do not match (the
    # payload's last byte is chosen so, and so that at least three pad bits are there; asserted below).
    for tail in range(256):
        claimed = b"no final block " + bytes([tail])
        s = B.Stream().fixed(_lits(claimed), False)
        crc = zlib.crc32(claimed) & 0xffffffff
        if (-s.bits) % 8 >= 3 and ((crc & 0xffff) ^ (crc >> 16)) != 0xffff:
            break
    else:
        raise AssertionError("no payload found for the no-final-block case")
    add("no_final_block", s, claimed)
    # A stream cut short.  The kernel reads on through the trailer (4 to 7 bytes are inside last_dw) and then zeros; in a
    # FIXED block seven zero bits are the end-of-block code.  The streams and their trailers are fixed, so the walk can be
    # followed bit by bit at each of the four byte alignments (done with a restatement of inflate_member's rules):
    #   cut_in_the_middle_of_a_code: the trailer's bits decode as three more literals (23 of 40 bytes), the zeros end the
    #     block, which is final: INF_E_SIZE (pos != isize).
    #   cut_in_the_middle_of_extra_bits: the match completes with the trailer's bits (inside isize), the zeros end the
    #     block, which is not final; the next header is 000 from the zeros, a stored block with LEN = NLEN = 0:
    #     INF_E_STORED.
    s = B.Stream().fixed(_lits(noise[:40]), True)
    add("cut_in_the_middle_of_a_code", s.raw()[:20], noise[:40])
    s = B.Stream().fixed(_lits(noise[:3100]), False)
    b0 = s.bits
    s.fixed([(200, 3000)], False)
    b1 = s.bits - 7  # (behind the distance's 10 extra bits, in front of the end-of-block code)
    cut = (b1 - 5) // 8
    assert b1 - 10 < 8 * cut < b1 and b0 < b1 - 10
    s.fixed(_lits(b"and more"), True)
    add("cut_in_the_middle_of_extra_bits", s.raw()[:cut], bytes(s.payload))
    #   cut_in_the_middle_of_a_dynamic_header: the lengths that are missing come from the trailer's bits and then from
    #     zeros (the all-zeros code of the code-length code) until `k < total` ends the loop; 256 has a code by then, and
    #     the literal/length and distance lengths so spelled over-subscribe their code space: INF_E_HEADER (build_table,
    #     left < 0).
    s = B.Stream().dynamic(_lits(b"abcdefghijklmnopqrstuvwxyz0123456789"), True, _shaped(286, list(range(A, A + 26)) + list(range(48, 58)) + [256, 257, 270, 285], 12),
                           _shaped(30, list(range(0, 12)), 7))
    add("cut_in_the_middle_of_a_dynamic_header", s.raw()[:12], bytes(s.payload))
    assert len(set(c[0] for c in cases)) == len(cases)
    return tuple(cases)


def member_trailer(payload):
    return struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


# ------------------------------------------------------------------ BAM files whose record members come from the builder
def _sam(path, n, seed):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:20000\n")
        for i in range(n):
            lq = int(rng.integers(30, 150))
            seq = "".join("ACGT"[k] for k in rng.integers(0, 4, lq))
            qual = "".join(chr(33 + int(k)) for k in rng.choice([2, 11, 25, 37], lq, p=[0.05, 0.1, 0.15, 0.7]))
            f.write("read%d\t0\tchr1\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\tNM:i:%d\n" % (i, int(rng.integers(1, 19000)), lq, seq, qual, int(rng.integers(0, 4))))


def bgzf_member(payload, raw=None, extra=b""):
    if raw is None:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(payload) + c.flush()
    xlen = 6 + len(extra)
    bsize = 12 + xlen + len(raw) + 8 - 1
    assert bsize < 65536
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra + b"BC" + struct.pack("<HH", 2, bsize)
    return head + raw + member_trailer(payload)


def _members(buf):
    at = 0
    while at < len(buf):
        bsize = struct.unpack_from("<H", buf, at + 16)[0] + 1
        yield buf[at:at + bsize]
        at += bsize


def handbuilt_bams(tmp_path, n_reads=300, per_member=10):
    """(sam path, {name: bam path} of valid files, {name: bam path} of invalid files, members in the valid files, the same
    records as a BAM whose members zlib wrote, (length of the header member, 17 MiB of good members to insert behind it)).  The
    records are the ones `fade out -u` makes of a small SAM; the header member and the end-of-file member are ordinary;
    every record member's DEFLATE stream is the builder's: one valid file per encoder (the random composer, each header
    shape of deflate_cases.SHAPES), one invalid file per invalid case (a record member replaced by the case's stream, with
    the trailer its payload would have had)."""
    sam = tmp_path / "reads.sam"
    _sam(sam, n_reads, 17)
    p = subprocess.run([FADE, "out", "-u", "-t", "1", str(sam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    payload = b"".join(zlib.decompress(m[18:-8], -15) for m in _members(p.stdout))
    o = 4
    o += 4 + struct.unpack_from("<i", payload, o)[0]
    n_ref = struct.unpack_from("<i", payload, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", payload, o)[0] + 4
    header, recs = payload[:o], []
    while o < len(payload):
        bs = struct.unpack_from("<i", payload, o)[0]
        recs.append(payload[o:o + 4 + bs])
        o += 4 + bs
    assert len(recs) == n_reads
    pieces = [b"".join(recs[k:k + per_member]) for k in range(0, len(recs), per_member)]
    rng = np.random.default_rng(23)
    valid, invalid, n_members = {}, {}, 0
    encoders = [("random_composer", {})] + sorted(SHAPES.items())
    for name, opts in encoders:
        ms = []
        for piece in pieces:
            s = encode(piece, rng, **opts)
            assert B.expected(s.raw()) == ("ok", piece, b""), name
            ms.append(bgzf_member(piece, raw=s.raw()))
        path = tmp_path / ("valid_%s.bam" % name)
        path.write_bytes(bgzf_member(header) + b"".join(ms) + EOF_MARK)
        valid[name] = path
        n_members += len(ms)
    good = [bgzf_member(piece, raw=encode(piece, rng).raw()) for piece in pieces]
    for k, (name, raw, verdict, claimed) in enumerate(invalid_cases()):
        ms = list(good)
        ms[3 + k % (len(ms) - 3)] = bgzf_member(claimed, raw=raw)
        path = tmp_path / ("invalid_%s.bam" % name)
        path.write_bytes(bgzf_member(header) + b"".join(ms) + EOF_MARK)
        invalid[name] = path
    # The same faults around REAL records, where the fault allows it: the stream decodes to the member's records if the
    # inflater is lenient, so nothing but the inflater's verdict can turn the exit status of the run.
    for k, which in enumerate(("code_length", "literal_length", "distance")):
        ms, at = list(good), 5 + 7 * k
        s = encode_incomplete(pieces[at], rng, which)
        ms[at] = bgzf_member(pieces[at], raw=s.raw())
        path = tmp_path / ("invalid_records_in_incomplete_%s_set.bam" % which)
        path.write_bytes(bgzf_member(header) + b"".join(ms) + EOF_MARK)
        invalid["records_in_incomplete_%s_set" % which] = path
    for name, at, raw, claimed in (("records_one_byte_more_than_isize", 4, encode(pieces[4], rng).raw(), pieces[4][:-1]),
                                   ("records_one_byte_less_than_isize", 9, encode(pieces[9], rng).raw(), pieces[9] + b"\0"),
                                   ("records_without_final_block", 14, B.Stream().fixed(list(pieces[14]), False).raw(), pieces[14])):
        assert B.expected(raw, isize=len(claimed))[0] in ("error", "truncated"), name
        ms = list(good)
        ms[at] = bgzf_member(claimed, raw=raw)
        path = tmp_path / ("invalid_%s.bam" % name)
        path.write_bytes(bgzf_member(header) + b"".join(ms) + EOF_MARK)
        invalid[name] = path
    # the same records written by zlib: the reference that owes nothing to the inflaters under test
    ref = tmp_path / "zlib_written.bam"
    ref.write_bytes(bgzf_member(header) + b"".join(bgzf_member(piece) for piece in pieces) + EOF_MARK)
    # Good members to put between the header and a file's own members: the reader that fetches the header inflates the
    # file's first 16 MiB on the host, so a member is the device inflater's to judge only when it lies beyond them.
    unit = b"".join(good)
    padding = unit * ((17 << 20) // len(unit) + 1)
    return sam, valid, invalid, n_members, ref, (len(bgzf_member(header)), padding)
