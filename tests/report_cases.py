"""Hand-built annotated BAM records for the report tests (test_report_file_model.py, test_gpu_report_batch.py): the smallest
shapes at which the rules of `fade stats` / `fade stats-clip` over tags read back, and the kernels that state them, can go
wrong.  The tags need not come from an aligner.  good_records() is 600 records that take part, are skipped, or pass; FAILURES
holds one record per failure of the rules."""
import random
import struct

import clip_cases as cc

NAMES = ["chr10", "chr1", "c", "n" * 40]
# stem loops: 0.75 n rounds to 1, 2, 2; the edges of a lane group; every row class of the alignment (0.75 n <= 64, 128, 256,
# 512, beyond) with the last one-strip query (683 -> 512 rows) and the first two-strip one (684 -> 513)
STEMS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 128, 129, 300, 512, 513, 683, 684, 700)
_rng = random.Random(20261020)


def _bases(n):
    return "".join(_rng.choice("ACGT") for _ in range(n)).encode()


def _like(s):
    """s with a few substitutions and a gap: something for the alignment to find"""
    b = bytearray(s)
    for k in range(3, len(b), 11):
        b[k] = ord("ACGT"[(b"ACGT".index(bytes([b[k]])) + 1) % 4])
    return bytes(b[:len(b) // 2] + b[len(b) // 2 + (len(b) > 20):])


def _z(tag, text):
    return tag + b"Z" + text + b"\0"


def aux(rs=b"rsC\x03", am=None, as_=None, ar=None, ab=None):
    return (rs or b"") + b"".join(_z(t, v) for t, v in ((b"am", am), (b"as", as_), (b"ar", ar), (b"ab", ab)) if v is not None)


def rec(name, cigar, aux_bytes, tid=1, pos=100, flag=0, qual=None):
    lq = sum(n for n, c in cc.cigar_ops(cigar) if c in "MIS=X")
    seq = ("ACGT" * (lq // 4 + 1))[:lq]
    return cc.build_rec(name, tid, pos, 30, flag, -1, -1, 0, cigar, seq or "*", qual if qual is not None else "I" * lq, aux_bytes)


def left(name, n=12, cigar="8S50M", **kw):
    """an artifact on the left side with a stem loop of n bases"""
    sl = _bases(n)
    return rec(name, cigar, aux(b"rsC\x03", b"chr1,40,%dM;" % n, sl + b";", _like(sl) + b";", bytes(33 + (7 * k) % 60 for k in range(n))), **kw)


def _named():
    sl, sr = _bases(20), _bases(33)
    c = [("left_only", rec("left_only", "8S50M", aux(b"rsC\x03", b"chr1,40,12M", sl, _like(sl), b"J" * 20))),
         ("right_only", rec("right_only", "4S50M8S", aux(b"rsC\x05", b";chr10,77,4=1X3D9M", b";" + sr, b";" + _like(sr), b"5" * 33), flag=16)),
         ("both_sides", rec("both_sides", "6S40M9S", aux(b"rsC\x07", b"chr1,40,12M;chr10,+77,9M2I", sl + b";" + sr, _like(sl) + b";" + _like(sr),
                                                          bytes(range(40, 90)))))]
    c += [("stem_%d" % n, left("stem_%d" % n, n)) for n in STEMS]
    c += [("as_three_pieces", rec("three", "50M8S", aux(b"rsC\x05", b";chr1,5,8M", b"AAAA;GGGGCCCC;TTTT", b"TT;GGGGCACC;AA", b"0123456789"))),
          ("ab_longer", rec("ab_longer", "50M8S", aux(b"rsC\x05", b";chr1,5,8M", b";ACGTACGT", b";ACGAACGT", b"ABCDEFGHIJKLMNOPQR"))),
          ("cigar_5S10S100M", left("c1", cigar="5S10S100M")),
          ("cigar_3H5S90M7S2H", rec("c2", "3H5S90M7S2H", aux(b"rsC\x05", b";chr1,5,8M", b";ACGTACGT", b";ACGAACGT", b"ABCDEFGH"))),
          ("cigar_inner_S", rec("c3", "4S20M3S30M6S", aux(b"rsC\x07", b"c,1,2M;c,-3,4M", sl + b";" + sr, sr + b";" + sl, b"K" * 33))),
          ("pos_0_left_clip", left("p0", pos=0)),
          ("name_1", left("n1", tid=2)), ("name_40", left("n40", tid=3)),
          ("qual_ff", left("qff", qual=chr(288) * 58)),
          ("long_read", left("long", cigar="8S19992M", qual="!" * 12345 + '"' + "!" * 7654)),
          ("reversed", left("rev", flag=16)), ("ar_empty", rec("ar_empty", "8S50M", aux(b"rsC\x03", b"chr1,40,12M;", b"ACGTACGT;", b";", b"IIIIIIII")))]
    for t, f, v in (("c", "b", 3), ("C", "B", 3), ("s", "h", 0x0103), ("S", "H", 0x0103), ("i", "i", 0x01000003), ("I", "I", 0x80000003)):
        sl = _bases(9)
        c.append(("rs_" + t, rec("rs_" + t, "8S50M", aux(b"rs" + t.encode() + struct.pack("<" + f, v), b"chr1,40,9M;", sl + b";", _like(sl) + b";", b"F" * 9))))
    tags = (b"chr1,40,9M;", b"ACGTACGTA;", b"ACGTACGTA;", b"F" * 9)
    c += [("rs_absent", rec("rs_absent", "8S50M", aux(None, *tags))), ("rs_Z", rec("rs_Z", "8S50M", aux(_z(b"rs", b"3"), *tags))),
          ("am_absent", rec("am_absent", "8S50M", aux(b"rsC\x03", None, *tags[1:]))),
          ("am_i", rec("am_i", "8S50M", aux(b"rsC\x03" + b"ami" + struct.pack("<i", 5), None, *tags[1:]))),
          ("rs_clean_clipped", rec("clean", "5S45M7S", aux(b"rsC\x01"))), ("clip_0S", rec("zero", "0S50M", aux(b"rsC\x01"))),
          ("clip_only_S", rec("onlyS", "6S4S", aux(b"rsC\x01"))), ("clip_H_S_M_S_H", rec("hs", "2H3S40M4S1H", aux(b"rsC\x21")))]
    return c


def good_records():
    """600 records; LABELS[k] names record k.  Artifact rows at 255, 256, 257 and 511, 512: the edges of a block of records."""
    return list(_GOOD)


def _build():
    named = _named()
    recs, labels = [], []
    edge = {255, 256, 257, 511, 512}
    k = 0
    while len(recs) < 600:
        i = len(recs)
        if i in edge:
            recs.append(left("edge%d" % i, 10 + i % 7))
            labels.append("edge_%d" % i)
        elif k < len(named) and i % 3 == 1:
            labels.append(named[k][0])
            recs.append(named[k][1])
            k += 1
        else:
            recs.append(rec("f%d" % i, "5S45M" if i % 2 else "50M", aux(b"rsC\x01" if i % 2 else b"rsC\x00")))
            labels.append("filler")
    assert k == len(named)
    return recs, labels


_GOOD, LABELS = _build()

_T = dict(am=b"chr1,40,9M;chr1,50,9M", as_=b"ACGTACGTA;ACGTACGTT", ar=b"ACGTACGTA;ACGTACGTT", ab=b"F" * 12)


def _bad(rs=b"rsC\x07", cigar="8S50M6S", tid=1, **kw):
    t = dict(_T)
    t.update(kw)
    return rec("bad", cigar, aux(rs, t["am"], t["as_"], t["ar"], t["ab"]), tid=tid)


# label -> (report, FADEHIP_E_UNSUPPORTED instead of _INVALID, the record)
FAILURES = {
    "side_malformed": ("stats", False, _bad(am=b"chr1,40,9m;chr1,50,9M")),
    "side_missing": ("stats", False, _bad(am=b"chr1,40,9M")),
    "side_pos_outside_int32": ("stats", False, _bad(am=b"chr1,40,9M;chr1,2147483648,9M")),
    "as_absent": ("stats", False, _bad(as_=None)),
    "ar_not_Z": ("stats", False, rec("bad", "8S50M6S", aux(b"rsC\x07", _T["am"], _T["as_"], None, _T["ab"]) + b"arA5")),
    "ab_absent": ("stats", False, _bad(ab=None)),
    "as_no_piece_1": ("stats", False, _bad(as_=b"ACGTACGTA")),
    "ar_no_piece_1": ("stats", False, _bad(ar=b"ACGTACGTA")),
    "as_piece_empty": ("stats", False, _bad(as_=b";ACGTACGTT")),
    "ab_short": ("stats", False, _bad(ab=b"F" * 8)),
    "no_S_op": ("stats", False, _bad(cigar="50M")),
    "refid_beyond_header": ("stats", False, _bad(tid=len(NAMES))),
    "refid_unmapped": ("stats", False, _bad(tid=-1)),
    "piece_too_long": ("stats", True, _bad(rs=b"rsC\x03", as_=b"A" * 32769 + b";", ab=b"F" * 32769)),
    "aux_damaged": ("stats", False, rec("bad", "8S50M6S", aux(b"rsC\x07", _T["am"]) + b"asZACGT")),
    "clip_on_l_seq_0": ("clip", False, cc.build_rec("bad", 1, 100, 30, 0, -1, -1, 0, "5S", "*", "", aux(b"rsC\x01"))),
    "clip_longer_than_l_seq": ("clip", False, cc.build_rec("bad", 1, 100, 30, 0, -1, -1, 0, "12S10M", "ACGTACGTAC", "I" * 10, aux(b"rsC\x01"))),
}
