"""fadehip_tags_batch / Context.tags_batch: rs and am read back out of records on the device, against tests/tags_model.py
array for array — constructed records (clip_cases.build_rec with hand-built aux bytes) for every branch of the grammar,
then the annotated golden sets with the three consumers behind it, all on the device, against oracle/pyfilter and
oracle/pyremap."""
import ctypes
import struct

import numpy as np
import pytest

import fade_amd
import clip_cases as cc
import tags_model as tm
from oracle import pyfilter, pyremap

pytestmark = pytest.mark.gpu

NAMES = ["chr10", "chr1", "chr2", "dup", "dup", "c"]  # chr10 in front of chr1: a comparison that stops at the shorter length hits it
KEYS = ["rs", "have", "trim_left", "trim_right", "art_tid", "art_pos", "cig_off", "cig"]
GOOD = b"chr1,5,3M"


def _z(tag, text):
    return tag + b"Z" + text + b"\0"


def _barr(ty, n):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[ty]
    return b"XBB" + ty.encode() + struct.pack("<I", n) + struct.pack("<%d%s" % (n, fmt), *range(1, n + 1))


def _cases():
    """(label, own tid, aux bytes)"""
    c = []
    rs6 = b"rsC\x06"
    # rs: every integer type, the low byte of wide ones, a negative c, types that are no rs, none, two, behind other fields, last
    c += [("rs_" + t, 1, b"rs" + t.encode() + struct.pack("<" + f, v) + _z(b"am", GOOD + b";" + GOOD))
          for t, f, v in (("c", "b", 6), ("C", "B", 6), ("s", "h", 6), ("S", "H", 6), ("i", "i", 6), ("I", "I", 6))]
    c += [("rs_S_wide", 1, b"rsS" + struct.pack("<H", 0x0106)), ("rs_I_wide", 1, b"rsI" + struct.pack("<I", 0x01000204)),
          ("rs_s_wide_negative", 1, b"rss" + struct.pack("<h", -250)), ("rs_i_wide", 1, b"rsi" + struct.pack("<i", 0x7fffff02)),
          ("rs_c_negative", 1, b"rsc" + struct.pack("<b", -2)), ("rs_Z", 1, _z(b"rs", b"6")), ("rs_A", 1, b"rsA6"),
          ("rs_f", 1, b"rsf" + struct.pack("<f", 6.0)), ("rs_none", 1, b"NMC\x01"), ("no_aux", 1, b""),
          ("rs_twice", 1, b"rsC\x02" + rs6), ("rs_Z_then_C", 1, _z(b"rs", b"x") + rs6), ("rs_last", 1, b"NMC\x01" + _z(b"XZ", b"hello") + rs6)]
    c += [("rs_behind_B" + t, 1, _barr(t, 5) + rs6) for t in "cCsSiIf"]
    c += [("rs_behind_empty_B", 1, _barr("S", 0) + rs6), ("rs_behind_H", 1, b"XHH1AE3\0" + rs6), ("rs_behind_Z", 1, _z(b"XZ", b"rsC;am,") + rs6),
          ("rs_behind_empty_Z", 1, _z(b"XZ", b"") + rs6), ("rs_behind_A_f", 1, b"XAAr" + b"Xff" + struct.pack("<f", 1.5) + rs6)]
    # am: presence and sides
    c += [("am_absent", 1, rs6), ("am_i", 1, rs6 + b"ami" + struct.pack("<i", 5)), ("am_empty", 1, rs6 + _z(b"am", b"")),
          ("am_no_semicolon", 1, rs6 + _z(b"am", GOOD)), ("am_left_only", 1, rs6 + _z(b"am", GOOD + b";")),
          ("am_right_only", 1, rs6 + _z(b"am", b";" + GOOD)), ("am_both", 1, rs6 + _z(b"am", GOOD + b";chr2,77,4=1X")),
          ("am_only_semicolon", 1, rs6 + _z(b"am", b";")), ("am_second_semicolon", 1, rs6 + _z(b"am", GOOD + b";" + GOOD + b";")),
          ("am_twice", 1, rs6 + _z(b"am", b"chr2,1,1M;") + _z(b"am", GOOD + b";" + GOOD)), ("am_i_then_Z", 1, b"amC\x01" + _z(b"am", GOOD)),
          ("am_in_front_of_rs", 1, _z(b"am", GOOD + b";") + rs6), ("am_without_rs", 1, _z(b"am", b";" + GOOD))]
    # name
    c += [("name_own", 2, _z(b"am", b"chr2,5,3M")), ("name_other", 2, _z(b"am", b"chr1,5,3M;chr10,5,3M")), ("name_unknown", 1, _z(b"am", b"chrX,5,3M")),
          ("name_chr1_own_chr10", 0, _z(b"am", b"chr1,5,3M")), ("name_chr10_own_chr1", 1, _z(b"am", b"chr10,5,3M")),
          ("name_prefix_of_all", 1, _z(b"am", b"chr,5,3M;chr100,5,3M")), ("name_empty", 1, _z(b"am", b",5,3M")),
          ("name_dup_own_second", 4, _z(b"am", b"dup,5,3M")), ("name_dup_own_first", 3, _z(b"am", b"dup,5,3M")), ("name_dup_other", 1, _z(b"am", b"dup,5,3M")),
          ("name_unmapped_read", -1, _z(b"am", b"chr2,5,3M")), ("name_one_byte", 1, _z(b"am", b"c,5,3M")), ("name_case", 1, _z(b"am", b"CHR1,5,3M"))]
    # pos
    c += [("pos_" + lab, 1, _z(b"am", b"chr1," + p + b",3M;chr1," + p + b","))
          for lab, p in (("0", b"0"), ("above_2_32", b"%d" % ((1 << 32) + 5)), ("minus", b"-5"), ("plus", b"+5"), ("empty", b""), ("12a", b"12a"),
                         ("blank", b" 5"), ("20_digits", b"12345678901234567890"), ("int64_max", b"%d" % ((1 << 63) - 1)), ("int64_max_1", b"%d" % (1 << 63)),
                         ("int64_min", b"-%d" % (1 << 63)), ("int64_min_1", b"-%d" % ((1 << 63) + 1)), ("sign_only", b"-"), ("two_signs", b"+-5"),
                         ("zeros", b"0" * 25 + b"7"))]
    # CIGAR
    many = lambda n: b"".join(b"%d%s" % (1 + k % 9, b"MIDNSHP=XB"[k % 10:k % 10 + 1]) for k in range(n))
    c += [("cig_" + lab, 1, _z(b"am", b"chr1,5," + t + b";chr2,6," + t))
          for lab, t in (("empty", b""), ("1", many(1)), ("10", many(10)), ("17", many(17)), ("300", many(300)), ("count_0", b"0M3D"),
                         ("max_count", b"%dM" % ((1 << 28) - 1)), ("count_2_28", b"%dM" % (1 << 28)), ("count_huge", b"99999999999999999999M"),
                         ("zeros", b"0" * 12 + b"5M"), ("trailing_count", b"3M2"), ("leading_op", b"M3M"), ("two_ops", b"3MM"), ("lower", b"3m"),
                         ("third_comma", b"3M,2D"), ("blank", b"3M 2D"), ("star", b"*"),
                         ("trim_saturates", b"%dM" % ((1 << 28) - 1) * 9), ("no_ref_ops", b"5S4I3H2P1B"))]
    c += [("cig_left_bad_right_good", 1, _z(b"am", b"chr1,5,3m;chr2,6,4M2D")), ("cig_left_good_right_bad", 1, _z(b"am", b"chr1,5,4M2D;chr2,6,4"))]
    return c


CASES = _cases()
SEQ = "ACGTTGCAAC"


def _rec(k, tid, aux):
    lq = k % len(SEQ) + 1  # (every alignment of the aux area)
    return cc.build_rec("q%d" % k, tid, 100 + k, 30, 0, -1, -1, 0, "%dM" % lq, SEQ[:lq], "I" * lq, aux)


def _same(got, want, what=""):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key, got[key][:20], want[key][:20])


def test_the_cases_are_what_they_say():
    t = tm.tags_batch([_rec(k, tid, aux) for k, (_, tid, aux) in enumerate(CASES)], NAMES)
    by = {lab: k for k, (lab, _, _) in enumerate(CASES)}
    assert len(by) == len(CASES)
    f = lambda lab, key, side=None: int(t[key][by[lab]] if side is None else t[key][2 * by[lab] + side])
    assert [f("rs_" + x, "rs") for x in "cCsSiI"] == [6] * 6 and f("rs_S_wide", "rs") == 6 and f("rs_I_wide", "rs") == 4 and f("rs_c_negative", "rs") == 0xfe
    assert all(f(x, "have") & 1 == 0 and f(x, "rs") == 0 for x in ("rs_Z", "rs_A", "rs_f", "rs_none", "rs_Z_then_C")) and f("rs_twice", "rs") == 2
    assert all(f("rs_behind_B" + x, "rs") == 6 for x in "cCsSiIf") and f("rs_behind_Z", "have") == 1
    assert [f(x, "have") >> 1 for x in ("am_absent", "am_i", "am_empty", "am_no_semicolon", "am_left_only", "am_right_only", "am_both")] == [0, 0, 1, 3, 3, 5, 7]
    assert f("am_second_semicolon", "have") >> 1 == 3 and f("am_twice", "art_tid", 0) == 2 and f("am_i_then_Z", "have") == 0
    assert (f("name_own", "art_tid", 0), f("name_other", "art_tid", 0), f("name_other", "art_tid", 1), f("name_unknown", "art_tid", 0)) == (2, 1, 0, -1)
    assert (f("name_chr1_own_chr10", "art_tid", 0), f("name_chr10_own_chr1", "art_tid", 0), f("name_empty", "art_tid", 0)) == (1, 0, -1)
    assert f("name_empty", "have") == 2 | 4 and f("name_dup_own_second", "art_tid", 0) == f("name_dup_own_first", "art_tid", 0) == f("name_dup_other", "art_tid", 0) == 3
    assert [f("pos_" + x, "have") >> 2 for x in ("0", "above_2_32", "minus", "plus", "empty", "12a", "blank", "20_digits")] == [3, 3, 3, 3, 0, 0, 0, 0]
    assert (f("pos_above_2_32", "art_pos", 0), f("pos_minus", "art_pos", 1), f("pos_plus", "art_pos", 0)) == ((1 << 32) + 5, -5, 5)
    assert [f("pos_" + x, "have") >> 2 for x in ("int64_max", "int64_max_1", "int64_min", "int64_min_1")] == [3, 0, 3, 0]
    n_ops = lambda lab: int(t["cig_off"][2 * by[lab] + 1] - t["cig_off"][2 * by[lab]])
    assert [n_ops("cig_" + x) for x in ("empty", "1", "10", "17", "300", "count_0", "max_count")] == [0, 1, 10, 17, 300, 2, 1]
    assert [f("cig_" + x, "have") >> 2 for x in ("empty", "300", "count_0", "max_count", "count_2_28", "trailing_count", "leading_op", "lower", "third_comma")] == [3, 3, 3, 3, 0, 0, 0, 0, 0]
    assert f("cig_trim_saturates", "trim_left") == (1 << 31) - 1 and f("cig_no_ref_ops", "trim_right") == 0 and f("cig_count_0", "trim_left") == 3
    assert f("cig_left_bad_right_good", "have") == 2 | 8 and f("cig_left_bad_right_good", "trim_right") == 6 and f("cig_left_good_right_bad", "have") == 2 | 4
    assert set(int(x) & 15 for x in t["cig"]) == set(range(10))


def test_every_case_in_one_call_and_on_its_own(ctx):
    recs = [_rec(k, tid, aux) for k, (_, tid, aux) in enumerate(CASES)]
    _same(ctx.tags_batch(recs, NAMES), tm.tags_batch(recs, NAMES), "all")
    for k, (lab, _, _) in enumerate(CASES):
        _same(ctx.tags_batch([recs[k]], NAMES), tm.tags_batch([recs[k]], NAMES), lab)


def test_1500_picks_in_random_order(ctx):
    rng = np.random.default_rng(20261019)
    picks = rng.integers(0, len(CASES), size=1500)
    recs = [_rec(j, CASES[p][1], CASES[p][2]) for j, p in enumerate(picks)]
    want = tm.tags_batch(recs, NAMES)
    assert want["cig_off"][-1] > 3000 and len(set(int(x) % 4 for x in np.cumsum([len(r) for r in recs]))) == 4
    _same(ctx.tags_batch(recs, NAMES), want)
    # no contig table at all: every name is unknown, nothing else changes
    got = ctx.tags_batch(recs, [])
    assert (got["art_tid"] == -1).all()
    want["art_tid"][:] = -1
    _same(got, want)


def test_cig_cap_one_short_names_the_need_and_the_exact_cap_passes(ctx):
    recs = [_rec(k, tid, aux) for k, (_, tid, aux) in enumerate(CASES)]
    want = tm.tags_batch(recs, NAMES)
    need = int(want["cig_off"][-1])
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    cat = np.frombuffer(b"".join(recs), dtype=np.uint8)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.tags_batch_packed(cat, off, NAMES, cig_cap=need - 1)
    assert e.value.code == -1 and ("%d CIGAR ops" % need) in str(e.value), str(e.value)
    _same(ctx.tags_batch_packed(cat, off, NAMES, cig_cap=need), want)
    # nothing is written when the ops do not fit
    o = [np.full(len(off) * 2 * 8, 0x5a, np.uint8) for _ in range(8)]  # rs, have, trim_left, trim_right, art_tid, art_pos, cig_off, cig
    arr = (ctypes.c_char_p * len(NAMES))(*[x.encode() for x in NAMES])
    rc = ctx._L.fadehip_tags_batch(ctx._h, len(recs), cat.ctypes.data, off.ctypes.data, len(NAMES), arr, *[x.ctypes.data for x in o], need - 1)
    assert rc == -1 and all((x == 0x5a).all() for x in o)


def test_refused_records_name_their_index_and_the_context_goes_on(ctx):
    recs = [_rec(k, 1, b"rsC\x06" + _z(b"am", GOOD + b";")) for k in range(6)]
    want = tm.tags_batch(recs, NAMES)

    def refused(batch, k):
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.tags_batch(batch, NAMES)
        assert e.value.code == -1 and ("record %d " % k) in str(e.value), str(e.value)

    # what check_records refuses: block_size beyond the bytes, l_read_name 0, an l_seq that does not fit
    for k, damage in ((4, lambda b: struct.pack("<I", 400) + b[4:]), (0, lambda b: b[:12] + b"\0" + b[13:]), (5, lambda b: b[:20] + struct.pack("<i", 4000) + b[24:]),
                      (2, lambda b: b[:20] + struct.pack("<i", -1) + b[24:])):
        batch = list(recs)
        batch[k] = damage(batch[k])
        refused(batch, k)
    # an aux area cut inside a field — block_size says so too, so the record is whole and only the walk can tell
    for k, aux in ((3, b"rsC"), (1, b"rs"), (5, b"r"), (0, b"rsC\x06amZchr1,5,3M"), (2, b"rsC\x06XBBi\x05\0\0\0\x01\x02\x03"), (4, b"rsC\x06XBB"),
                   (3, b"rsC\x06XBBi\xff\xff\xff\xff"), (1, b"rsC\x06XQQ1"), (5, b"NMC\x01rsS\x06"), (0, b"XHH12")):
        batch = list(recs)
        batch[k] = _rec(k, 1, aux)
        assert tm.read_tags(batch[k], NAMES) is None
        refused(batch, k)
    # two damaged records: the first one is named
    batch = list(recs)
    batch[2], batch[4] = _rec(2, 1, b"rsC"), _rec(4, 1, b"rsC")
    refused(batch, 2)
    _same(ctx.tags_batch(recs, NAMES), want)
    empty = ctx.tags_batch([], NAMES)
    assert all(len(empty[k]) == 0 for k in KEYS if k != "cig_off") and list(empty["cig_off"]) == [0]


@pytest.mark.parametrize("tag", ["anno_c1", "anno_c2", "anno_c5"])
def test_golden_sets_tags_then_clip_eject_extract_all_on_the_device(ctx, tag):
    names, recs, bams = tm.annotated(tag)
    want_x = pyremap.extract_records(recs, names)
    for label, rr, bb in tm.orders(recs, bams):
        off = np.zeros(len(bb) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bb], out=off[1:])
        cat = np.frombuffer(b"".join(bb), dtype=np.uint8)
        t = ctx.tags_batch_packed(cat, off, names)
        _same(t, tm.tags_batch(bb, names), label)
        assert (t["have"] & 1).all() and ((t["rs"] & 2) != 0).any() and ((t["rs"] & 4) != 0).any()
        # fade out -c
        out, oo = ctx.clip_batch_packed(cat, off, t["rs"], t["trim_left"], t["trim_right"])
        want, _ = pyfilter.fade_out(rr, names[0], clip=True)
        assert [tm.bam_to_line(out[oo[k]:oo[k + 1]].tobytes(), names) for k in range(len(bb))] == want
        # fade out: groups on the name-sorted order, record by record on the shuffled one
        grouped = label == "sorted"
        keep = ctx.eject_batch_packed(cat, off, t["rs"], grouped).astype(bool)
        if not grouped:
            keep &= (t["have"] & 1) != 0
        want, _ = pyfilter.fade_out(rr, names[0], clip=False)
        assert [tm.bam_to_line(b, names) for b, k in zip(bb, keep) if k] == want and 0 < len(want) < len(bb)
        # fade extract
        out, oo = ctx.extract_batch_packed(cat, off, t["rs"], t["art_tid"], t["art_pos"], t["cig_off"], t["cig"])
        got = [tm.bam_to_line(out[oo[s]:oo[s + 1]].tobytes(), names) for s in range(2 * len(bb)) if oo[s + 1] > oo[s]]
        assert got == (want_x if grouped else pyremap.extract_records(rr, names)) and len(got) >= 10
