"""fadehip_sw_stats_batch (parasail's stats mode, stats.d:87,123,164) against the restatement tests/sw_stats_ref.c, field for
field."""
import numpy as np
import pytest

import sw_stats_ref as S
from helpers import COMP, make_pairs, rand_seq

pytestmark = pytest.mark.gpu

SC = S.SCORING_STATS
KINDS = ("random", "planted", "homopolymer", "tandem", "nrich", "iupac", "related", "lowcomplexity", "refspecial")
FADEHIP_E_UNSUPPORTED = -5


def _as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _compare(ctx, qs, rs, scoring=SC, rules=S.RULES_DEFAULT):
    qs = [_as_bytes(q) for q in qs]
    rs = [_as_bytes(r) for r in rs]
    got = ctx.sw_stats_batch(qs, rs, scoring)
    exp = S.stats_batch(qs, rs, scoring, rules)
    assert got.shape == exp.shape
    diff = np.nonzero(got.view(np.int32).reshape(-1, 6) != exp.view(np.int32).reshape(-1, 6))[0]
    if len(diff):
        k = int(diff[0])
        raise AssertionError("%d/%d pairs differ; first pair %d (lq %d, lr %d): got %r expected %r" % (
            len(np.unique(diff)), len(qs), k, len(qs[k]), len(rs[k]), tuple(got[k]), tuple(exp[k])))
    return got


def d_round_075(n):
    """D's round(0.75 * n): half away from zero (stats.d: the query is stemloop[0 .. round(0.75 * len)])."""
    return (3 * n + 2) // 4


def stemloop_pairs(rng, n, lens=(6, 150)):
    """(query, reference) as `fade stats` makes them from an artifact side: as[0 .. round(0.75 |as|)] against ar = rc(as).
    Every |as| is 2 mod 4, so that round() meets .5."""
    qs, rs = [], []
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for k in range(n):
        L = int(rng.integers(lens[0] // 4, lens[1] // 4 + 1)) * 4 + 2
        stem = int(rng.integers(1, L // 2 + 1))
        left = rand_seq(rng, stem)
        loop = rand_seq(rng, L - 2 * stem)
        right = np.array([COMP[int(x)] for x in left[::-1]], dtype=np.uint8)
        m = rng.random(stem) < 0.08
        right[m] = acgt[rng.integers(0, 4, int(m.sum()))]
        s = np.concatenate([left, loop, right])
        if k % 7 == 3:
            s[rng.random(L) < 0.05] = ord("N")
        ar = np.array([COMP[int(x)] for x in s[::-1]], dtype=np.uint8)
        qs.append(s[:d_round_075(L)].tobytes())
        rs.append(ar.tobytes())
    return qs, rs


def test_stats_stemloop_shaped(ctx):
    rng = np.random.default_rng(11)
    qs, rs = stemloop_pairs(rng, 4000)
    assert all(len(r) % 4 == 2 for r in rs)
    got = _compare(ctx, qs, rs)
    assert (got["score"] > 0).mean() > 0.9


def test_stats_every_query_length_to_512(ctx):
    rng = np.random.default_rng(12)
    qs, rs = [], []
    for lq in range(1, 513):
        for lr in (1, int(rng.integers(2, 200)), int(rng.integers(200, 700))):
            if lq % 3 == 0:  # the reference a mutated slice around the query: long paths that touch every row
                r = np.concatenate([rand_seq(rng, lr // 3), rand_seq(rng, lq), rand_seq(rng, lr // 3)])
                q = r[lr // 3: lr // 3 + lq].copy()
                q[rng.random(lq) < 0.05] = ord("G")
            else:
                q, r = rand_seq(rng, lq), rand_seq(rng, lr)
            qs.append(q)
            rs.append(r)
    _compare(ctx, qs, rs)


def test_stats_class_edges_and_families(ctx):
    # the row classes switch at 64, 128, 256, 512 query bases (1, 2, 4, 8 rows a lane), and beyond 512 to strips
    rng = np.random.default_rng(13)
    qs, rs = [], []
    for lq in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1600):
        q, r = make_pairs(rng, len(KINDS), lq_range=(lq, lq), lr_range=(1, 900), kinds=KINDS)
        qs += q
        rs += r
    _compare(ctx, qs, rs)


def test_stats_across_int16_int32(ctx):
    # match 10 x 4,000 bases: the score leaves the int16 range; several strips of 512 rows; long gaps (ext > open)
    rng = np.random.default_rng(14)
    qs, rs = [], []
    base = rand_seq(rng, 4000)
    qs.append(base)
    rs.append(base.copy())
    rel = base.copy()
    rel[rng.random(4000) < 0.03] = ord("C")
    rel = np.concatenate([rel[:1500], rand_seq(rng, 40), rel[1500:2600], rel[2700:]])
    qs.append(base)
    rs.append(rel)
    qs.append(rand_seq(rng, 4000))
    rs.append(rand_seq(rng, 4000))
    qs.append(rand_seq(rng, 32768))
    rs.append(base[:300].copy())
    qs.append(base[:300].copy())
    rs.append(rand_seq(rng, 32768))
    got = _compare(ctx, qs, rs)
    assert got[0]["score"] == 40000 and got[0]["matches"] == 4000 and got[0]["length"] == 4000


def test_stats_empty_and_iupac(ctx):
    qs = [b"", b"ACGT", b"", b"N", b"NNNN", b"RYKMSWBDHV", b"acgtn", b"ACGT=*.-", b"A" * 600]
    rs = [b"ACGT", b"", b"", b"N", b"NNNN", b"RYKMSWBDHV", b"ACGTN", b"ACGT=*.-", b""]
    got = _compare(ctx, qs, rs)
    for k in (0, 1, 2, 8):
        assert tuple(got[k]) == (0, 0, 0, 0, 0, 0)
    rng = np.random.default_rng(15)
    q, r = make_pairs(rng, 400, lq_range=(1, 200), lr_range=(1, 300), kinds=("nrich", "iupac", "refspecial"))
    _compare(ctx, q, r)


def test_stats_other_scorings(ctx):
    rng = np.random.default_rng(16)
    qs, rs = make_pairs(rng, 300, lq_range=(1, 300), lr_range=(1, 400), kinds=KINDS)
    for scoring in ((10, 2, 2, -3), (1, 1, 1, 0), (5, 20, 3, -1), (32767, 32767, 32767, -32767)):
        _compare(ctx, qs, rs, scoring)


def test_stats_one_call_of_100k_pairs(ctx):
    rng = np.random.default_rng(17)
    qs, rs = stemloop_pairs(rng, 100_000)
    _compare(ctx, qs, rs)


def test_stats_unsupported_scoring(ctx):
    import fade_amd
    for bad in ((0, 8, 10, -5), (3, 0, 10, -5), (3, 8, 0, -5), (3, 8, 10, 1), (32768, 8, 10, -5), (3, 8, 10, -32768)):
        with pytest.raises(fade_amd.FadeHipError) as ei:
            ctx.sw_stats_batch([b"ACGT"], [b"ACGT"], bad)
        assert ei.value.code == FADEHIP_E_UNSUPPORTED, bad
    with pytest.raises(fade_amd.FadeHipError) as ei:
        ctx.sw_stats_batch([b"A" * 32769], [b"ACGT"])
    assert ei.value.code == FADEHIP_E_UNSUPPORTED


def test_stats_under_other_rules():
    import fade_amd
    rng = np.random.default_rng(18)
    qs, rs = make_pairs(rng, 300, lq_range=(1, 200), lr_range=(1, 300), kinds=KINDS)
    # (rules 0 means the defaults to fadehip_create: 0x10, a bit the stats do not read, turns every other one off)
    for rules in (0x10, 0x7f & ~0x2, 0x7f & ~0x4, 0x7f & ~0x8, 0x7f & ~0x1, 0x7f & ~0x40):
        c = fade_amd.Context(device=0, rules=rules)
        try:
            _compare(c, qs, rs, SC, rules)
        finally:
            c.close()


def test_annotate_unchanged_by_a_stats_call():
    import fade_amd
    from fade_amd import synth
    cfg, g, b = synth.make_config("C2", 3000, contig_len=200_000)
    c = fade_amd.Context(device=0)
    try:
        c.genome_upload(g.names, g.ascii_contigs())
        rs0, tags0 = fade_amd.annotate_records(c, b, cfg["floor_len"], cfg["window"])
        rng = np.random.default_rng(19)
        qs, rr = stemloop_pairs(rng, 2000)
        first = c.sw_stats_batch(qs, rr)
        rs1, tags1 = fade_amd.annotate_records(c, b, cfg["floor_len"], cfg["window"])
        assert np.array_equal(np.asarray(rs0), np.asarray(rs1))
        assert tags0 == tags1
        assert np.array_equal(first, c.sw_stats_batch(qs, rr))
    finally:
        c.close()
