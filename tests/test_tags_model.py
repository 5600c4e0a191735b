"""tests/tags_model.py — the plain-Python statement of the tag reader (fadehip_tags_batch) — held to the oracle on the
annotated golden sets.  Runs without a GPU.

The golden SAM with the golden tags appended (what `fade annotate` writes) is encoded to BAM; the model reads rs and am back
out of the bytes; its arrays are pushed through restatements of clip, eject and extract that take arrays where the oracle
parses tag text; and every record of oracle/pyfilter.fade_out and oracle/pyremap.extract_records must come out."""
import struct

import pytest

import tags_model as tm
from oracle import pyfilter, pyremap

TAGS = ["anno_c1", "anno_c2", "anno_c5"]


@pytest.fixture(scope="module", params=TAGS)
def gold(request):
    names, recs, bams = tm.annotated(request.param)
    return names, recs, bams, tm.tags_batch(bams, names)


def test_the_sets_hold_left_and_right_artifacts_and_round_trip(gold):
    names, recs, bams, t = gold
    assert ((t["rs"] & 2) != 0).sum() >= 1 and ((t["rs"] & 4) != 0).sum() >= 1
    assert (t["have"] & 1).all() and [int(v) for v in t["rs"]] == [int(r["tags"]["rs"][1]) & 0xff for r in recs]
    assert [tm.bam_to_line(b, names) for b in bams] == [pyfilter._fmt(r) for r in recs]
    for k, r in enumerate(recs):  # an artifact side is well-formed, names the read's contig, and carries ops
        for side in range(2):
            if t["rs"][k] & (2 << side):
                s = 2 * k + side
                assert t["have"][k] & (4 << side) and t["art_tid"][s] == names.index(r["rname"]) and t["cig_off"][s + 1] > t["cig_off"][s]


def test_clip_from_the_models_arrays_gives_every_record_of_fade_out_c(gold):
    names, recs, bams, _ = gold
    for label, rr, bb in tm.orders(recs, bams):
        t = tm.tags_batch(bb, names)
        want, _ = pyfilter.fade_out(rr, names[0], clip=True)
        got = [pyfilter._fmt(tm.clip_by_trims(r, int(t["rs"][k]), int(t["trim_left"][k]), int(t["trim_right"][k]), names[0])
                             if t["have"][k] & 1 and t["rs"][k] & 6 else r) for k, r in enumerate(rr)]
        assert len(want) == len(rr) and got == want, label
        assert sum(1 for a, r in zip(got, rr) if a != pyfilter._fmt(r)) >= 2


def test_eject_from_the_models_arrays_gives_every_record_of_fade_out(gold):
    names, recs, bams, _ = gold
    for label, rr, bb in tm.orders(recs, bams):
        t = tm.tags_batch(bb, names)
        want, _ = pyfilter.fade_out(rr, names[0], clip=False)
        keep = tm.eject_keep([r["qname"] for r in rr], t["rs"], t["have"], grouped=label == "sorted")
        got = [pyfilter._fmt(r) for r, k in zip(rr, keep) if k]
        assert got == want and 0 < len(got) < len(rr), label
    # grouped and not differ on these sets: a clean mate leaves with its group only
    t = tm.tags_batch(bams, names)
    q = [r["qname"] for r in recs]
    assert sum(tm.eject_keep(q, t["rs"], t["have"], True)) < sum(tm.eject_keep(q, t["rs"], t["have"], False))


def test_extract_from_the_models_arrays_gives_every_record_of_fade_extract(gold):
    names, recs, bams, t = gold
    want = pyremap.extract_records(recs, names)
    assert tm.extract_lines(recs, t, names) == want and len(want) >= 10


def test_the_grammar_on_hand_built_sides():
    names = ["chr1", "chr10", "chr1"]
    ok = lambda s: tm.parse_side(s, names)
    assert ok(b"chr1,5,3M2D") == (0, 5, [(3 << 4), (2 << 4) | 2]) and ok(b"chr10,+5,") == (1, 5, []) and ok(b",-5,1=") == (-1, -5, [0x17])
    assert ok(b"chrX,0,%dM" % ((1 << 28) - 1))[2] == [((1 << 28) - 1) << 4] and ok(b"chr1,0,%dM" % (1 << 28)) is None
    assert ok(b"c,9223372036854775807,") == (-1, (1 << 63) - 1, []) and ok(b"c,-9223372036854775808,")[1] == -(1 << 63)
    for bad in (b"", b"chr1", b"chr1,5", b"chr1,,1M", b"chr1,12a,1M", b"chr1, 5,1M", b"chr1,9223372036854775808,1M", b"chr1,5,1M,", b"chr1,5,1m",
                b"chr1,5,12", b"chr1,5,M", b"chr1,5,1M2", b"chr1,--5,1M", b"chr1,+,1M", b"chr1,5,1M;"):
        assert ok(bad) is None, bad
    rec = tm.cc.build_rec("q", 0, 7, 0, 0, -1, -1, 0, "4M", "ACGT", "IIII", b"XBBc\x02\0\0\0\x01\x02rsZ7\0rsC\x06amZchr1,5,2M\0rsC\x02")
    assert tm.read_tags(rec, names) == dict(rs=0, have=2 | 4, sides=[(0, 5, [0x20]), None])  # the first rs is a string: no rs
    assert tm.read_tags(rec[:-1], names) is None and tm.read_tags(rec[:-2] + struct.pack("<H", 0), names) is None
