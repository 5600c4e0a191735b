"""fadehip_intervals_* / Context.intervalset, Context.load_bed: the interval set on the device against tests/intervals_model.py
— set sizes at the edges of the 256-wide scan block and of the 2048-item sort tile, intervals over three contigs plus an empty
one, with duplicates, added unsorted in 1 and in 7 calls, from a first capacity of 16 and from the default; 4000 seeded queries
per case beside the hand cases; the long interval at the front of a contig and at the end of the one before; every error."""
import numpy as np
import pytest

import fade_amd
import intervals_model as im
import repeats_cases as rc

pytestmark = pytest.mark.gpu


def _arrays(triples):
    return (np.array([t[0] for t in triples], np.int32), np.array([t[1] for t in triples], np.int64), np.array([t[2] for t in triples], np.int64))


def _sealed(ctx, ivs, adds=1, names=rc.NAMES):
    s = ctx.intervalset(names)
    edges = [len(ivs) * k // adds for k in range(adds + 1)]
    for a, b in zip(edges, edges[1:]):
        s.add(*_arrays(ivs[a:b]))
    s.seal()
    return s


_WANT = {}


def _case(n):
    """the intervals, the queries and the model's answers of one set size: computed once, shared, left unchanged"""
    if n not in _WANT:
        ivs = rc.intervals(n, 100 + n)
        qs = rc.queries(ivs, 4000, 200 + n) + [q for _, (_, hq) in sorted(rc.hand_cases().items()) for q, _ in hq]
        _WANT[n] = (ivs, qs, rc.expect(rc.as_model(ivs), qs))
    return _WANT[n]


@pytest.mark.parametrize("cap", ["16", None], ids=["cap16", "cap_default"])
@pytest.mark.parametrize("adds", [1, 7])
@pytest.mark.parametrize("n", rc.COUNTS)
def test_seeded_sets_and_queries_equal_the_model(ctx, monkeypatch, n, adds, cap):
    if cap is None:
        monkeypatch.delenv("FADEHIP_INTERVALS_CAP", raising=False)
    else:
        monkeypatch.setenv("FADEHIP_INTERVALS_CAP", cap)
    ivs, qs, want = _case(n)
    s = _sealed(ctx, ivs, adds)
    try:
        assert s.count() == (n, len(rc.NAMES))
        got = s.overlaps(*_arrays(qs))
        bad = [(q, int(g), w) for q, g, w in zip(qs, got, want) if int(g) != w]
        assert not bad, bad[:5]
        if n >= 255:
            assert 0 < sum(want) < len(want)
        assert len(s.overlaps([], [], [])) == 0
    finally:
        s.close()


@pytest.mark.parametrize("label", sorted(rc.hand_cases()))
def test_hand_cases(ctx, label):
    ivs, qs = rc.hand_cases()[label]
    s = _sealed(ctx, ivs)
    try:
        assert [int(x) for x in s.overlaps(*_arrays([q for q, _ in qs]))] == [h for _, h in qs]
    finally:
        s.close()


@pytest.mark.parametrize("adds", [1, 7])
def test_one_interval_of_the_whole_contig_in_front_of_scan_blocks_of_short_ones(ctx, monkeypatch, adds):
    """[0, 2^31 - 1) sorts to the front of its contig; behind it lie four scan blocks of short intervals: the query far beyond
    them is covered by it alone, through the running maximum carried across the blocks"""
    monkeypatch.setenv("FADEHIP_INTERVALS_CAP", "16")
    ivs, qs = rc.long_at_front(4)
    s = _sealed(ctx, ivs[::-1] if adds == 1 else ivs, adds)
    try:
        assert [int(x) for x in s.overlaps(*_arrays([q for q, _ in qs]))] == [h for _, h in qs]
    finally:
        s.close()


def test_the_last_interval_of_a_contig_does_not_reach_into_the_next(ctx):
    """Contig cA's last interval ends at 2^31 - 1; cB's short intervals follow it in the sorted order.  A naive, unsegmented
    running maximum of the ends carries that end into every entry of cB, and every query on cB that starts behind cB's first
    start then hits: the queries here between and behind cB's intervals, which no interval of cB covers, fail under it.  The
    chrom id in the high word of the maximum is what keeps the contigs apart."""
    ivs, qs = rc.long_at_end_of_a(4)
    s = _sealed(ctx, ivs, 7)
    try:
        got = [int(x) for x in s.overlaps(*_arrays([q for q, _ in qs]))]
        assert got == [h for _, h in qs]
        assert sum(1 for (c, _, _), h in qs if c == 1 and h == 0) >= 4
    finally:
        s.close()


def test_errors(ctx, monkeypatch):
    monkeypatch.setenv("FADEHIP_INTERVALS_CAP", "16")
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.intervalset(["a", "b", "a"])
    assert e.value.code == -1 and '"a"' in str(e.value)
    good = [(0, 10 * k, 10 * k + 5) for k in range(10)]
    s = ctx.intervalset(rc.NAMES)
    try:
        s.add(*_arrays(good))
        with pytest.raises(fade_amd.FadeHipError) as e:  # a query before seal
            s.overlaps([0], [0], [5])
        assert e.value.code == -1
        # a bad interval is named by its index, and nothing of its call is added (the call here outgrows the first arrays)
        for k, bad in ((0, (-1, 1, 2)), (7, (len(rc.NAMES), 1, 2)), (57, (0, -1, 2)), (99, (1, 5, 5)), (31, (1, 6, 5)), (64, (2, 0, im.MAX_END + 1)), (3, (2, 1 << 40, (1 << 40) + 1))):
            call = [(1, 7, 9)] * 100
            call[k] = bad
            with pytest.raises(fade_amd.FadeHipError) as e:
                s.add(*_arrays(call))
            assert e.value.code == -1 and ("interval %d:" % k) in str(e.value), str(e.value)
            assert s.count() == (10, len(rc.NAMES))
        call = [(1, 7, 9)] * 100
        call[40], call[41] = (0, 3, 3), (0, 4, 4)
        with pytest.raises(fade_amd.FadeHipError) as e:  # the first of two
            s.add(*_arrays(call))
        assert "interval 40:" in str(e.value)
        s.seal()
        qs = [(1, 0, 100), (0, 0, 100), (0, 5, 10), (0, 95, 200)]
        assert [int(x) for x in s.overlaps(*_arrays(qs))] == rc.expect(rc.as_model(good), qs) == [0, 1, 0, 0]
        for again in (lambda: s.add(*_arrays(good)), lambda: s.add([], [], []), s.seal):  # an add after seal, a second seal
            with pytest.raises(fade_amd.FadeHipError) as e:
                again()
            assert e.value.code == -6
        assert s.count() == (10, len(rc.NAMES))
    finally:
        s.close()


@pytest.mark.parametrize("cap", ["16", None], ids=["cap16", "cap_default"])
def test_load_bed_of_a_file_written_from_the_same_cases_equals_add_of_the_arrays(ctx, monkeypatch, tmp_path, cap):
    if cap is None:
        monkeypatch.delenv("FADEHIP_INTERVALS_CAP", raising=False)
    else:
        monkeypatch.setenv("FADEHIP_INTERVALS_CAP", cap)
    ivs, qs, want = _case(5000)
    f = tmp_path / "cases.bed"
    f.write_bytes(b"#chrom\tstart\tend\tname\n" + im.bed_text([(rc.NAMES[c], s, e) for c, s, e in ivs]).replace(b"\n", b"\tAluY\r\n"))
    order = []  # the file's names get their ids in order of first appearance
    for c, _, _ in ivs:
        if c not in order:
            order.append(c)
    s = ctx.load_bed(str(f))
    try:
        assert s.count() == (5000, 3)
        mapped = [(order.index(c) if c in order else -1, a, b) for c, a, b in qs]
        assert [int(x) for x in s.overlaps(*_arrays(mapped))] == want
        with pytest.raises(fade_amd.FadeHipError) as e:  # it comes sealed
            s.add([0], [1], [2])
        assert e.value.code == -6
    finally:
        s.close()
    empty = tmp_path / "empty.bed"
    empty.write_bytes(b"track name=none\n")
    s = ctx.load_bed(str(empty))
    try:
        assert s.count() == (0, 0) and [int(x) for x in s.overlaps([0, -1], [0, 0], [10, 10])] == [0, 0]
    finally:
        s.close()


def test_load_bed_names_the_line_and_refuses_compressed_files_by_name(ctx, tmp_path):
    f = tmp_path / "bad.bed"
    f.write_bytes(b"c\t1\t2\n" * 4999 + b"c\t9\t3\n")
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.load_bed(str(f))
    assert e.value.code == -1 and "line 5000: start is not below end" in str(e.value) and "bad.bed" in str(e.value)
    z = tmp_path / "r.bed.gz"
    z.write_bytes(b"\x1f\x8b\x08")
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.load_bed(str(z))
    assert e.value.code == -1 and "r.bed.gz" in str(e.value) and "plain text" in str(e.value)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.load_bed(str(tmp_path / "missing.bed"))
    assert e.value.code == -1 and "missing.bed" in str(e.value)
