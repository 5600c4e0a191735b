"""The class runners of the alignment engine at their chunk boundaries: the single-pass kernels (FADEHIP_KERNEL=pk / int32)
and both long-list kernels under a 4 MiB trace budget, where every list is served in three chunks or more with a partial
last one, at level 2 (annotate) and level 1 (sw_batch); every answer against the oracle.  A runner that hands a chunk the
wrong slice of its work, meta or forward arrays, or files too few timing spans, fails here.

The profile of each level-2 run, and of one default two-pass run, is checked too: the times finite and positive, the
counters equal to what the library gave before the runners shared their helpers (they are deterministic).  Level 1 keeps
no profile (fadehip_last_run_profile wants a collected level-2 run), so its chunk counts are worked out from the pairs."""
import math

import numpy as np
import pytest

import fade_amd
from fade_amd import format_tags, synth
from helpers import concat, make_pairs

pytestmark = pytest.mark.gpu

BUDGET = 4 << 20
COUNTERS = ("alignments", "cells", "trace_bytes", "snapshot_bytes", "candidates")
# Counters of last_profile(0) for each level-2 run below, taken from the library of commit 7e3019c (the parent of the commit
# that gave the runners their shared helpers) with this file's inputs
EXPECTED = {
    "pk": dict(alignments=360, cells=17254350, trace_bytes=10368000, snapshot_bytes=8627175, candidates=0),
    "int32": dict(alignments=360, cells=17254350, trace_bytes=10368000, snapshot_bytes=8627175, candidates=0),
    "long_wave": dict(alignments=40, cells=19761600, trace_bytes=13824000, snapshot_bytes=0, candidates=0),
    "long_thread": dict(alignments=40, cells=19761600, trace_bytes=10008000, snapshot_bytes=0, candidates=0),
    "twopass": dict(alignments=360, cells=17254350, trace_bytes=12672000, snapshot_bytes=0, candidates=0),
}


def _level2_case(oracle, n_reads, seed, floor_len=5, **kw):
    g = synth.Genome(2, 60_000, 17)
    b = synth.make_reads(g, n_reads, seed, p_sc=1.0, **kw)
    b.pop("_truth", None)
    seqs = [a.tobytes().decode() for a in g.ascii_contigs()]
    ors, oam = oracle.annotate_batch_soa(oracle.GenomeHolder(g.names, seqs), b, floor_len, kw["window"], threads=8)
    return dict(names=g.names, seqs=seqs, batch=b, floor_len=floor_len, window=kw["window"], rs=ors, am=oam)


def _level1_case(oracle, n, lq, lr_range, seed):
    # (kinds whose queries have lq bases exactly: the pairs fill ONE list)
    qs, rs = make_pairs(np.random.default_rng(seed), n, lq_range=(lq, lq), lr_range=lr_range, kinds=("planted", "tandem", "random", "homopolymer"))
    qc, qo = concat(qs)
    rc, ro = concat(rs)
    exp, exp_ops = oracle.sw_batch(qc, qo, rc, ro, threads=8, max_ops=16, striped=True)
    return dict(q=(qc, qo), r=(rc, ro), exp=exp, exp_ops=exp_ops, n=n, max_lq=max(len(q) for q in qs), max_lr=max(len(r) for r in rs))


@pytest.fixture(scope="module")
def short_reads(oracle):
    """150-base soft-clipped reads (the 160-row class), and as many level-1 pairs of that class."""
    return (_level2_case(oracle, 360, 31, read_len=150, window=100, clip_min=6, clip_max=50),
            _level1_case(oracle, 360, 150, (300, 350), 32))


@pytest.fixture(scope="module")
def long_reads(oracle):
    """600-base soft-clipped reads (the long list), and as many level-1 pairs."""
    return (_level2_case(oracle, 40, 33, read_len=600, window=120, clip_min=6, clip_max=30, insert_mu=800),
            _level1_case(oracle, 40, 600, (800, 840), 34))


def _annotate(c, case):
    c.genome_upload(case["names"], [s.encode() for s in case["seqs"]])
    rs, aln, stats = c.annotate(case["batch"], case["floor_len"], case["window"])
    tags = format_tags(case["batch"], case["names"], rs, aln)
    assert np.array_equal(rs, case["rs"]), np.nonzero(rs != case["rs"])[0][:10]
    for i, am in enumerate(case["am"]):
        if am is None:
            assert i not in tags
        else:
            assert tags[i]["am"] == am, i
    assert len(tags) > 10
    return c.last_profile(0)


def _sw_batch(c, case):
    got = c.sw_batch_packed(*case["q"], *case["r"])
    for k in range(case["n"]):
        assert tuple(int(got[k][f]) for f in ("score", "end_query", "end_ref", "beg_query", "beg_ref", "n_ops")) == tuple(int(x) for x in case["exp"][k]), k
        m = min(int(case["exp"][k][5]), 16)
        assert list(got[k]["ops"][:m]) == list(case["exp_ops"][k][:m]), k


def _check_profile(name, prof):
    print(name, {k: prof[k] for k in COUNTERS}, {k: prof[k] for k in prof if k.endswith("_ms")})
    for k in ("gate_ms", "forward_ms", "traceback_ms", "total_ms"):
        assert math.isfinite(prof[k]) and prof[k] > 0, (k, prof[k])


def _check_counters(name, prof):
    assert {k: prof[k] for k in COUNTERS} == EXPECTED[name]


def _assert_chunked(n_units, per_chunk):
    """three launches or more, the last one partial"""
    assert per_chunk >= 1 and n_units > 2 * per_chunk and n_units % per_chunk != 0, (n_units, per_chunk)


@pytest.mark.parametrize("kernel", ["pk", "int32"])
def test_single_pass_kernels_in_chunks(short_reads, kernel, monkeypatch):
    level2, level1 = short_reads
    monkeypatch.setenv("FADEHIP_KERNEL", kernel)
    per_wave = 8 if kernel == "pk" else 4  # alignments per wavefront
    c = fade_amd.Context(device=0, trace_bytes=BUDGET)
    try:
        prof = _annotate(c, level2)
        _check_profile(kernel, prof)
        # run_class_single adds waves x (trace bytes of a wave) per chunk, one class here: that gives the bytes of a wave
        waves = -(-prof["alignments"] // per_wave)
        assert prof["trace_bytes"] % waves == 0
        _assert_chunked(waves, BUDGET // (prof["trace_bytes"] // waves))
        # level 1: quad_bytes = n_blocks * (packed ? R : R / 2) * 64 * 4 with R = 10 rows per lane
        n_blocks = (level1["max_lr"] + 15 + 3) // 4
        _assert_chunked(-(-level1["n"] // per_wave), BUDGET // (n_blocks * (10 if kernel == "pk" else 5) * 64 * 4))
        _sw_batch(c, level1)
        _check_counters(kernel, prof)
    finally:
        c.close()


@pytest.mark.parametrize("kernel", ["long_wave", "long_thread"])
def test_long_list_in_chunks(long_reads, kernel, monkeypatch):
    level2, level1 = long_reads
    if kernel == "long_thread":
        monkeypatch.setenv("FADEHIP_LONG_THREAD", "1")
    c = fade_amd.Context(device=0, trace_bytes=BUDGET)
    try:
        prof = _annotate(c, level2)
        _check_profile(kernel, prof)
        # both runners add (alignments of the chunk) x (trace bytes of one) per chunk
        n = prof["alignments"]
        assert prof["trace_bytes"] % n == 0
        item = prof["trace_bytes"] // n
        if kernel == "long_wave":
            _assert_chunked(n, BUDGET // item)
        else:
            # run_long: item = max_lq * lhalf with max_lq = 600 and lhalf = (max_lr + 1) / 2; a chunk is sized with the row
            # buffers on top, 8 bytes per window column (max_lr is one of two values: either must give a partial last chunk)
            assert item % 600 == 0
            for max_lr in (2 * (item // 600) - 1, 2 * (item // 600)):
                _assert_chunked(n, BUDGET // (item + 8 * max_lr))
        max_lq, max_lr = level1["max_lq"], level1["max_lr"]
        if kernel == "long_wave":  # item_bytes of run_long_wave at 12 rows per lane
            item = ((max_lr + 63 + 3) // 4) * 6 * 64 * 4
        else:  # per_item of run_long
            item = max_lq * ((max_lr + 1) // 2) + 8 * max_lr
        _assert_chunked(level1["n"], BUDGET // item)
        _sw_batch(c, level1)
        _check_counters(kernel, prof)
    finally:
        c.close()


def test_two_pass_profile(short_reads):
    c = fade_amd.Context(device=0)
    try:
        prof = _annotate(c, short_reads[0])
        _check_profile("twopass", prof)
        _check_counters("twopass", prof)
    finally:
        c.close()
