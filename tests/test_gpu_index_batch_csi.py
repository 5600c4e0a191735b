"""fadehip_index_batch_csi (Context.index_batch(csi=)): the key kernel of bam_index.hpp that takes a CSI geometry, and the
kernels behind it as they are, held to tests/csi_model.py on records the test brings at virtual offsets the test brings.
Small geometries put every level of the bin tree and thousands of windows within a few hundred bases."""
import numpy as np
import pytest

import fade_amd
import bai_model as bm
import clip_cases as cc
import csi_model as cm
from test_csi_model import seeded_records
from test_gpu_index_batch import SPECS, _batch, _model

pytestmark = pytest.mark.gpu

TILE = 256
MAX_OP = (1 << 28) - 1


def _cigar(reflen):
    """A CIGAR of that many reference bases (an op holds at most 2^28 - 1)."""
    if reflen == 0:
        return "*"
    ops = []
    while reflen > MAX_OP:
        ops.append("%dN" % MAX_OP)
        reflen -= MAX_OP
    return "".join(ops) + "%dM" % reflen


def _specs(recs):
    return [(r["tid"], r["pos"], _cigar(r["reflen"]), r["flag"]) for r in recs]


def _both(ctx, specs, geometry):
    cat, off, voff = _batch(specs)
    return ctx.index_batch(cat, off, voff, csi=geometry), cm.per_call(_model(cat, voff), *geometry), _model(cat, voff)


def _same(got, want):
    assert got["chunks"] == want["chunks"]
    assert got["linear"] == want["linear"]
    assert got["refs"] == want["refs"]
    assert (got["n"], got["first_key"], got["last_key"]) == (want["n"], want["first_key"], want["last_key"])


def test_the_cigar_helper_counts():
    for n in (0, 1, 2, 100, MAX_OP, MAX_OP + 1, (1 << 31) + 2, (1 << 31) + 3):
        ops = cc.cigar_ops(_cigar(n))
        assert sum(k for k, c in ops) == n and all(k <= MAX_OP for k, c in ops), n


def test_hand_cases_at_4_2(ctx):
    specs = [(0, 33, "14M", 0),      # inside one 16-base leaf
             (0, 40, "10M", 0),      # across a 16-base line, inside a 128-base bin
             (0, 85, "30M", 4),      # placed and unmapped: a chunk in its leaf, no window
             (0, 120, "10M", 0),     # across a 128-base line: the root
             (0, 1000, "24M", 0),    # ends at 1024: accepted
             (1, -1, "5M", 0),       # pos -1 with a reference begins at 0
             (1, 0, "*", 0),
             (1, 16, "3M2D3M", 0),
             (3, 500, "5S20M", 0),
             (3, 1023, "1M", 0),
             (-1, -1, "*", 0), (-1, -1, "*", 4), (-1, -1, "*", 4)]
    got, want, recs = _both(ctx, specs, (4, 2))
    _same(got, want)
    assert [c[:2] for c in got["chunks"]][:5] == [(0, 11), (0, 1), (0, 9 + 5), (0, 0), (0, 8)]
    assert [r[0] for r in got["refs"]] == [0, 1, 3, -1] and got["refs"][-1][3:] == (1, 2)
    assert (3, 63, recs[9]["u"]) in got["linear"]
    bad = list(specs)
    bad[4] = (0, 1000, "25M", 0)     # ends at 1025
    cat, off, voff = _batch(bad)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.index_batch(cat, off, voff, csi=(4, 2))
    assert e.value.code == -5 and "record 4:" in str(e.value) and "2^10" in str(e.value) and "CSI" in str(e.value)
    with pytest.raises(cm.IndexError_) as m:
        cm.per_call(_model(cat, voff), 4, 2)
    assert (m.value.kind, m.value.record) == ("span", 4)
    bad[2] = (0, 30, "1M", 0)        # ... and a key that steps back in front of it: the order comes first
    cat, off, voff = _batch(bad)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.index_batch(cat, off, voff, csi=(4, 2))
    assert e.value.code == -1 and "record 2: not in coordinate order" in str(e.value)


@pytest.mark.parametrize("geometry", [(4, 2), (6, 3), (14, 6)])
def test_seeded_records_whose_runs_cross_the_tile_edges(ctx, geometry):
    recs = seeded_records(geometry[0], geometry[1], seed=7)
    assert len(recs) > 2 * TILE + 20
    for edge in (TILE, 2 * TILE):  # a run of one (refID, bin) over each edge of a 256-record tile: copies of one record
        for k in range(edge - 6, edge + 7):
            recs[k] = dict(recs[edge - 6])
    got, want, model = _both(ctx, _specs(recs), geometry)
    _same(got, want)
    bins = [cm.reg2bin(*cm.span_of(r), *geometry) if r["tid"] >= 0 else None for r in model]
    for edge in (TILE, 2 * TILE):
        assert (model[edge - 1]["tid"], bins[edge - 1]) == (model[edge]["tid"], bins[edge])
    assert len({b for b in bins if b is not None}) > 20 and len({cm.bin_level(b, geometry[1])[0] for b in bins if b is not None}) >= 3
    b = fade_amd.CsiBuilder(3, *geometry)
    try:
        b.add(0, got)
        assert b.finish() == cm.build(3, model, *geometry)
    finally:
        b.close()


def test_more_linear_entries_than_records_and_65536(ctx):
    # (4, 2) has 64 windows per reference: 1,100 references with one record over all of them leave 70,400 entries, more than
    # the room a call of the file path starts with (records + 65536; tests/test_gpu_csi_stream.py reaches its second run of
    # the write kernel with the same records).  This call sizes its arrays from the counts.
    specs = [(t, 0, "1024M", 0) for t in range(1100)]
    got, want, _ = _both(ctx, specs, (4, 2))
    assert len(want["linear"]) == 1100 * 64 > len(specs) + 65536
    _same(got, want)


def test_14_5_gives_the_arrays_of_the_call_without_a_geometry(ctx):
    cat, off, voff = _batch(SPECS)
    plain = ctx.index_batch(cat, off, voff)
    assert ctx.index_batch(cat, off, voff, csi=(14, 5)) == plain == bm.per_call(_model(cat, voff))
    specs = list(SPECS)
    specs[10] = (0, (1 << 29) - 100, "101M", 0)
    specs = specs[:11]
    cat, off, voff = _batch(specs)
    for kw, words in ((dict(), "a BAI index cannot hold it"), (dict(csi=(14, 5)), "CSI")):
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.index_batch(cat, off, voff, **kw)
        assert e.value.code == -5 and "record 10: ends beyond 2^29" in str(e.value) and words in str(e.value)


LARGE = [(0, (1 << 29) - 10, 20), (0, 1 << 29, 100), (0, (1 << 30) + 77, 150), (0, (1 << 31) - 2, 1), (0, (1 << 31) - 2, (1 << 31) + 2)]


def test_14_6_at_the_large_positions(ctx):
    specs = [(0, 5, "10M", 0)] + [(t, p, _cigar(n), 0) for t, p, n in LARGE] + [(1, 7, "3M", 0), (-1, -1, "*", 4)]
    got, want, recs = _both(ctx, specs, (14, 6))
    _same(got, want)
    assert cm.span_of(recs[5])[1] == 1 << 32  # end == 2^32 is accepted: the root, windows up to the last
    assert got["chunks"][-2][:2] == (0, 0) and (0, (1 << 18) - 1, recs[5]["u"]) in got["linear"]
    leaf = cm.first_bin(6)
    assert [c[1] for c in got["chunks"]][:5] == [leaf, cm.reg2bin((1 << 29) - 10, (1 << 29) + 10, 14, 6), leaf + (1 << 15), leaf + (((1 << 30) + 77) >> 14),
                                                 leaf + (((1 << 31) - 2) >> 14)]
    with pytest.raises(fade_amd.FadeHipError):  # (what a BAI makes of them)
        cat, off, voff = _batch(specs)
        ctx.index_batch(cat, off, voff)
    specs[5] = (0, (1 << 31) - 2, _cigar((1 << 31) + 3), 0)  # end == 2^32 + 1
    cat, off, voff = _batch(specs)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.index_batch(cat, off, voff, csi=(14, 6))
    assert e.value.code == -5 and "record 5:" in str(e.value) and "2^32" in str(e.value) and "CSI" in str(e.value)
    with pytest.raises(cm.IndexError_) as m:
        cm.per_call(_model(cat, voff), 14, 6)
    assert (m.value.kind, m.value.record) == ("span", 5)


def test_invalid_geometries_and_none(ctx):
    cat, off, voff = _batch([(0, 5, "10M", 0)])
    for geometry in [(3, 2), (14, 0), (14, 9), (14, 7), (30, 1), (4, 10), (-1, 5)]:
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.index_batch(cat, off, voff, csi=geometry)
        assert e.value.code == -1 and "min_shift" in str(e.value), geometry
    cat, off, voff = _batch([])
    assert ctx.index_batch(cat, off, voff, csi=(8, 8)) == dict(chunks=[], linear=[], refs=[], n=0, first_key=0, last_key=0)
    cat, off, voff = _batch([(2, 40_000, "10M20000N10M", 0)])
    assert ctx.index_batch(cat, off, voff, csi=(29, 1)) == cm.per_call(_model(cat, voff), 29, 1)
