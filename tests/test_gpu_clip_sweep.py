"""The hard clip on the device over tests/clip_sweep.py's generated records (about 28,000: the writer's shifts and tails, the
bin's levels, random CIGARs) — through fadehip_clip_batch (clip_batch_*_kernel) and through the file path from tags
(bam_rewrite_kernel<true> and the from-tags kernels, whole and cut, and under keep_sorted).  Every record is compared AS
BYTES: with clip_cases.expected (oracle/pyfilter.clip_read laid out by build_rec) for the device function, with
tests/tags_model.clip_by_trims by way of test_gpu_bam_from_tags._clip_expect for the file path.  tests/test_clip_sweep.py
asserts without a GPU that the sweep holds what it is for."""
import random
import struct

import pytest

import clip_cases as cc
import clip_sweep as sw
import resort_model as rm
from test_gpu_bam_from_tags import _clip_expect, _clip_trims, _records, _stats_of, _stream
from test_gpu_tags_batch import _z

pytestmark = pytest.mark.gpu

FAMILIES = list(sw.FAMILIES)


def _first_difference(got, want):
    """(field, got, want) of the first field in which two records differ, by decode_rec; the sizes when one does not decode."""
    try:
        d, w = cc.decode_rec(got), cc.decode_rec(want)
    except (AssertionError, struct.error, IndexError, UnicodeDecodeError):
        return "block_size / length", (struct.unpack_from("<I", got, 0)[0] if len(got) >= 4 else None, len(got)), len(want)
    for k in ("qname", "tid", "pos", "bin", "mapq", "flag", "mtid", "mpos", "tlen", "cigar", "seq", "pad", "qual"):
        if d[k] != w[k]:
            return k, d[k], w[k]
    if d["aux"] != w["aux"]:
        at = next((j for j, (x, y) in enumerate(zip(d["aux"], w["aux"])) if x != y), min(len(d["aux"]), len(w["aux"])))
        return "aux (%d and %d bytes) at byte %d" % (len(d["aux"]), len(w["aux"]), at), d["aux"][at:at + 8].hex(), w["aux"][at:at + 8].hex()
    return "bytes", got[:48].hex(), want[:48].hex()


def _mismatches(names, got, want):
    assert len(got) == len(want) == len(names)
    return [(n,) + _first_difference(g, w) for n, g, w in zip(names, got, want) if g != w]


def _clip_batch(ctx, cases):
    return ctx.clip_batch([cc.to_bam(c["rec"], c["aux"]) for c in cases], [c["rs"] for c in cases], [c["tl"] for c in cases], [c["tr"] for c in cases])


@pytest.mark.parametrize("family", FAMILIES)
def test_clip_batch_over_the_sweep_as_bytes_and_the_bin_on_its_own(ctx, family):
    cases, exp = sw.cases(family), sw.expected(family)
    got = _clip_batch(ctx, cases)
    bad = _mismatches([c["name"] for c in cases], got, [b for _, b in exp])
    assert not bad, (len(bad), bad[:8])
    # the bin once more, against reg2bin over the oracle's pos and CIGAR (a reset record: reg2bin(0, 1))
    wrong = []
    for c, g, (new, _) in zip(cases, got, exp):
        ref = sum(n for n, x in cc.cigar_ops(new["cigar"]) if x in cc._RC)
        p0 = max(new["pos"], 0)
        want = cc.reg2bin(p0, p0 + (ref if ref > 0 else 1)) & 0xffff
        if struct.unpack_from("<H", g, 14)[0] != want:
            wrong.append((c["name"], struct.unpack_from("<H", g, 14)[0], want))
    assert not wrong, (len(wrong), wrong[:8])


def test_clip_batch_random_family_in_a_shuffled_order(ctx):
    """Every record at another output alignment and in another block of the kernels."""
    cases, exp = sw.cases("random"), sw.expected("random")
    order = list(range(len(cases)))
    random.Random(7).shuffle(order)
    got = _clip_batch(ctx, [cases[i] for i in order])
    bad = _mismatches([cases[i]["name"] for i in order], got, [exp[i][1] for i in order])
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------------------------------------ the file path
def _tagged(cases):
    """The cases' records with rs:C and the trims as am CIGARs behind their aux bytes, as test_gpu_bam_from_tags has them."""
    return [cc.to_bam(c["rec"], c["aux"] + b"rsC" + bytes([c["rs"]]) + _z(b"am", c["rec"]["tags"]["am"][1].encode())) for c in cases]


def _file_path_expectation(cases, recs):
    want = []
    for c, b in zip(cases, recs):
        rs, trims = _clip_trims(b, cc.CONTIGS)
        assert rs == c["rs"] and trims == [c["tl"] if rs & 2 else 0, c["tr"] if rs & 4 else 0], c["name"]
        want.append(_clip_expect(b, rs, trims[0], trims[1], cc.CONTIGS) if rs & 6 else b)
    return want


@pytest.mark.parametrize("family", FAMILIES)
def test_the_file_path_from_tags_over_the_sweep_whole_and_cut(ctx, family):
    cases = sw.cases(family)
    recs = _tagged(cases)
    want = _file_path_expectation(cases, recs)
    names = [c["name"] for c in cases]
    stats = _stats_of([c["rs"] for c in cases], [1] * len(cases))
    payload = b"".join(recs)
    r = _stream(ctx, cc.CONTIGS, payload, clip=True)
    bad = _mismatches(names, _records(r["out"]), want)
    assert not bad, (len(bad), bad[:8])
    assert r["totals"][:2] == (stats, len(cases))
    cuts = sorted(random.Random(11).sample(range(1, len(payload)), 12))
    r = _stream(ctx, cc.CONTIGS, payload, cuts=cuts, clip=True)
    assert r["out"] == b"".join(want) and r["totals"][:2] == (stats, len(cases))
    assert sum(r["per_call"]) == len(cases) and sum(1 for n in r["per_call"] if n) >= 6


def test_the_bin_family_under_keep_sorted_leaves_in_the_models_order(ctx):
    """The only records of the suite whose sort keys use the high bytes of pos; sorted by the key they come in with first."""
    cases = sw.cases("bins")
    recs = _tagged(cases)
    by_key = sorted(range(len(cases)), key=lambda i: (rm.key_in(recs[i]), i))
    cases, recs = [cases[i] for i in by_key], [recs[i] for i in by_key]
    want = _file_path_expectation(cases, recs)
    keys = [rm.key_out(a, b) for a, b in zip(recs, want)]
    order = rm.stable_order(keys)
    assert order != list(range(len(recs))) and any(rm.is_reset(a, b) for a, b in zip(recs, want))
    assert any(k >> 24 & 0xff for k in keys) and sum(1 for a, k in zip(recs, keys) if rm.key_in(a) != k) >= 100
    payload = b"".join(recs)
    for cuts in ([], sorted(random.Random(13).sample(range(1, len(payload)), 12))):
        r = _stream(ctx, cc.CONTIGS, payload, cuts=cuts, clip=True, keep_sorted=True)
        bad = _mismatches([cases[i]["name"] for i in order], _records(r["out"]), [want[i] for i in order])
        assert not bad, (len(cuts), len(bad), bad[:8])
