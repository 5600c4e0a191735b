"""fadehip_extract_batch / Context.extract_batch: remap.d:11-87 (`fade extract`) on the device, over constructed records.

Every case is held to oracle/pyremap.extract_records field by field, and as bytes to a builder written here from the
layout: block_size, refID, pos, l_read_name, mapq 0, bin = reg2bin over the new CIGAR's span, n_cigar_op, flag (0x10 exactly
when the read has it clear), l_seq, mate refID 0, mate pos 0, tlen 0, name, ops, the bases reverse-complemented (pad nibble
zero), the qualities reversed, no aux."""
import struct

import numpy as np
import pytest

import fade_amd
import clip_cases as cc
from oracle import pyremap

pytestmark = pytest.mark.gpu

CONTIGS = ["ctgA", "ctgB", "ctgC"]
L_SEQ = [0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 150, 151, 513]
L_NAME = [2, 3, 4, 5, 254]           # l_read_name, NUL included: CIGAR, bases and qualities start at every byte alignment
N_OPS = [1, 2, 10, 16]
POS = [0, (1 << 14) - 1, (1 << 26) - 3, 12345]  # the second and third with a span that crosses into the next bin
FLAGS = [0x10 | 0x1 | 0x80, 0x1 | 0x40 | 0x400, 0x10, 0]
AUX = b"NMC\x05XZZhello\0"


def _ops(rng, n):
    return [(int(rng.integers(1, 40)), "=XIDS"[(k + int(rng.integers(0, 5))) % 5]) for k in range(n)]


def _cigar(ops):
    return "".join("%d%s" % o for o in ops)


def _case(rng, k, lseq, lname, rs, n_ops_l, n_ops_r, pos_l, pos_r, flag):
    seq = "".join(cc.NT16[(k + j) % 16] for j in range(lseq)) if k % 3 else "".join(cc.NT16[int(x)] for x in rng.integers(0, 16, size=lseq))
    qual = "".join(chr(33 + (0xff if (j + k) % 5 == 0 else int(q))) for j, q in enumerate(rng.integers(0, 94, size=lseq)))
    qname = "".join(chr(int(c)) for c in rng.integers(65, 91, size=lname - 1))
    rec = cc.build_rec(qname, k % 3, 100 + k, 37, flag, 1, 77, -5, "%dS%dM" % (1, max(lseq - 1, 1)) if lseq > 1 else "*", seq or "*", qual, AUX if k % 2 else b"")
    sides = ((k % 3, pos_l, _ops(rng, n_ops_l)), ((k + 1) % 3, pos_r, _ops(rng, n_ops_r)))
    return dict(qname=qname, flag=flag, seq=seq, qual=qual, rec=rec, rs=rs, sides=sides)


def _cases():
    rng = np.random.default_rng(20261017)
    out, k = [], 0
    for lseq in L_SEQ:                      # every l_seq at every name alignment
        for lname in L_NAME:
            out.append(_case(rng, k, lseq, lname, (2, 4, 6)[k % 3], N_OPS[k % 4], N_OPS[(k + 1) % 4], POS[k % 4], POS[(k + 2) % 4], FLAGS[k % 4]))
            k += 1
    for n_ops in N_OPS:                     # every CIGAR size on both sides, every pos
        for pos in POS:
            out.append(_case(rng, k, 33, 5, 6, n_ops, N_OPS[(k + 1) % 4], pos, POS[(k + 1) % 4], FLAGS[k % 4]))
            k += 1
    for rs in (0, 1, 2, 4, 6, 3, 5, 7):     # nothing out for 0 and 1; bit 0 changes nothing
        out.append(_case(rng, k, 17, 4, rs, 2, 10, 0, (1 << 14) - 1, FLAGS[k % 4]))
        k += 1
    return out


CASES = _cases()


def _sides_arg(c):
    ops = lambda s: [(n << 4) | cc.OPS.index(o) for n, o in s[2]]
    return tuple((s[0], s[1], ops(s)) for s in c["sides"])


def _built(c):
    """The expected records of a case as bytes, from the layout."""
    comp = {a: b for a, b in zip(cc.NT16, (cc.NT16[int("{:04b}".format(i)[::-1], 2)] for i in range(16)))}
    out = []
    for side, bit in ((0, 2), (1, 4)):
        if not c["rs"] & bit:
            continue
        tid, pos, ops = c["sides"][side]
        lq = len(c["seq"])
        rc = "".join(comp[ch] for ch in reversed(c["seq"]))
        packed = bytearray((lq + 1) // 2)
        for j, ch in enumerate(rc):
            packed[j >> 1] |= cc.NT16.index(ch) << (4 if j % 2 == 0 else 0)
        reflen = sum(n for n, o in ops if o in "=XD")
        name = c["qname"].encode() + b"\0"
        body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), 0, cc.reg2bin(pos, pos + max(reflen, 1)), len(ops), 0 if c["flag"] & 0x10 else 0x10, lq, 0, 0, 0)
        body += name + b"".join(struct.pack("<I", (n << 4) | cc.OPS.index(o)) for n, o in ops) + bytes(packed)
        body += bytes((ord(q) - 33) & 0xff for q in reversed(c["qual"]))
        out.append(struct.pack("<I", len(body)) + body)
        assert len(out[-1]) == 36 + len(name) + 4 * len(ops) + (lq + 1) // 2 + lq
    return out


def _oracle_lines(c):
    am = ";".join("%s,%d,%s" % (CONTIGS[s[0]], s[1], _cigar(s[2])) if c["rs"] & bit else "" for s, bit in zip(c["sides"], (2, 4)))
    r = dict(qname=c["qname"], flag=c["flag"], seq=c["seq"], qual=c["qual"], tags={"rs": ("i", str(c["rs"])), "am": ("Z", am)})
    return pyremap.extract_records([r], CONTIGS)


def _line(b):
    d = cc.decode_rec(b)
    assert d["pad"] == 0 and d["aux"] == b""
    return "\t".join([d["qname"], str(d["flag"]), CONTIGS[d["tid"]], str(d["pos"] + 1), str(d["mapq"]), d["cigar"],
                      "=" if d["mtid"] == d["tid"] else CONTIGS[d["mtid"]], str(d["mpos"] + 1), str(d["tlen"]), d["seq"], d["qual"]])


@pytest.fixture(scope="module")
def got(ctx):
    """Every case in one call, and every case on its own."""
    whole = ctx.extract_batch([c["rec"] for c in CASES], [c["rs"] for c in CASES], [_sides_arg(c) for c in CASES])
    return whole, [ctx.extract_batch([c["rec"]], [c["rs"]], [_sides_arg(c)]) for c in CASES]


def test_the_builder_of_this_file_agrees_with_the_oracle():
    for c in CASES:
        assert [_line(b) for b in _built(c)] == _oracle_lines(c)
    assert sum(len(_built(c)) for c in CASES) > len(CASES)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_extract_batch_case_against_the_oracle_and_as_bytes(got, k):
    c, recs = CASES[k], got[1][k]
    assert len(recs) == bin(c["rs"] & 6).count("1")
    assert [_line(b) for b in recs] == _oracle_lines(c)
    for b, e in zip(recs, _built(c)):
        d, x = cc.decode_rec(b), cc.decode_rec(e)
        assert d == x                      # bin, mate fields, flag: other flag bits of the read do not leak
        assert d["flag"] in (0, 0x10) and (d["mapq"], d["mtid"], d["mpos"], d["tlen"]) == (0, 0, 0, 0)
    assert recs == _built(c)
    if (c["rs"] & 6) == 6:                 # left first, each side with its own contig, position and CIGAR
        l, r = cc.decode_rec(recs[0]), cc.decode_rec(recs[1])
        assert (l["tid"], l["pos"], l["cigar"]) == (c["sides"][0][0], c["sides"][0][1], _cigar(c["sides"][0][2]))
        assert (r["tid"], r["pos"], r["cigar"]) == (c["sides"][1][0], c["sides"][1][1], _cigar(c["sides"][1][2]))
        assert l["tid"] != r["tid"]


def test_extract_batch_all_cases_in_one_call(got):
    assert got[0] == [b for c in CASES for b in _built(c)]


def test_bins_at_the_boundaries(ctx):
    rec = CASES[0]["rec"]
    for pos, ops, want in ((0, [(5 << 4) | 7], 4681), ((1 << 14) - 1, [(2 << 4) | 7], 585), ((1 << 26) - 3, [(10 << 4) | 7], 0),
                           ((1 << 26) - 3, [(3 << 4) | 7], 4681 + 4095), (7, [(9 << 4) | 4], 4681)):
        out = ctx.extract_batch([rec], [2], [((0, pos, ops), None)])
        assert cc.decode_rec(out[0])["bin"] == want == cc.reg2bin(pos, pos + max(sum(o >> 4 for o in ops if (o & 15) in (0, 2, 3, 7, 8)), 1))


def test_extract_batch_1500_records_in_random_order(ctx):
    """More than one block of either kernel, and every output alignment in play."""
    rng = np.random.default_rng(7)
    order = [int(x) for x in rng.integers(0, len(CASES), size=1500)]
    out = ctx.extract_batch([CASES[k]["rec"] for k in order], [CASES[k]["rs"] for k in order], [_sides_arg(CASES[k]) for k in order])
    exp = [b for k in order for b in _built(CASES[k])]
    assert len(exp) > 1500 and len({sum(map(len, exp[:j])) % 4 for j in range(40)}) == 4
    assert out == exp


def test_extract_batch_refuses_malformed_records(ctx):
    c = CASES[20]
    good, side = c["rec"], [_sides_arg(c)]
    assert ctx.extract_batch([], [], []) == []
    cut = good[:40]                                                   # block_size says more than there is
    lname0 = good[:12] + b"\0" + good[13:]                            # l_read_name 0
    big_lseq = good[:20] + (10 ** 6).to_bytes(4, "little") + good[24:]  # l_seq beyond the record
    neg_lseq = good[:20] + (-3).to_bytes(4, "little", signed=True) + good[24:]
    for k, bad in enumerate([cut, lname0, big_lseq, neg_lseq]):
        batch = [good] * k + [bad, good]
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.extract_batch(batch, [6] * len(batch), side * len(batch))
        assert e.value.code == -1 and ("record %d" % k) in str(e.value), str(e.value)
    # a CIGAR offset that steps backwards
    off = np.array([0, len(good)], dtype=np.int64)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.extract_batch_packed(np.frombuffer(good, np.uint8), off, [2], [0, 0], [0, 0], [3, 1, 1], np.zeros(4, np.uint32))
    assert e.value.code == -1 and "record 0" in str(e.value)
    # the context still works
    assert ctx.extract_batch([good], [c["rs"]], side) == _built(c)


def test_extract_batch_out_cap_one_byte_short_writes_nothing(ctx):
    cs = CASES[:12]
    exp = b"".join(b for c in cs for b in _built(c))
    recs = [c["rec"] for c in cs]
    off = np.zeros(len(cs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    tid, pos, coff, cig = [], [], [0], []
    for c in cs:
        for s in _sides_arg(c):
            tid.append(s[0]); pos.append(s[1]); cig += s[2]; coff.append(len(cig))
    L = ctx._L
    cat = np.frombuffer(b"".join(recs), np.uint8)
    args = lambda buf, cap, oo: (ctx._h, len(cs), cat.ctypes.data, off.ctypes.data, rs.ctypes.data, tid_a.ctypes.data,
                                 pos_a.ctypes.data, coff_a.ctypes.data, cig_a.ctypes.data, buf.ctypes.data, cap, oo.ctypes.data)
    rs, tid_a, pos_a = np.array([c["rs"] for c in cs], np.uint8), np.array(tid, np.int32), np.array(pos, np.int64)
    coff_a, cig_a = np.array(coff, np.int64), np.array(cig, np.uint32)
    buf = np.full(len(exp) + 64, 0xA5, dtype=np.uint8)
    oo = np.zeros(2 * len(cs) + 1, dtype=np.int64)
    assert L.fadehip_extract_batch(*args(buf, len(exp) - 1, oo)) == -1
    assert (buf == 0xA5).all()             # nothing at all, and nothing behind out_cap
    assert L.fadehip_extract_batch(*args(buf, len(exp), oo)) == 0
    assert buf[:len(exp)].tobytes() == exp and (buf[len(exp):] == 0xA5).all() and oo[-1] == len(exp)
    for k, c in enumerate(cs):
        for side in range(2):
            if not c["rs"] & (2 << side):
                assert oo[2 * k + side + 1] == oo[2 * k + side]
