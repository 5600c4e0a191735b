"""tests/intervals_model.py, the interval set's rule in plain Python, on the hand cases the GPU tests share
(tests/repeats_cases.py) — the model itself is checked here, against the rule's own words and against an independent
restatement (a set of covered bases).  Runs without a GPU."""
import pytest

import intervals_model as im
import repeats_cases as rc


@pytest.mark.parametrize("label", sorted(rc.hand_cases()))
def test_hand_cases(label):
    ivs, qs = rc.hand_cases()[label]
    m = rc.as_model(ivs)
    for q, want in qs:
        assert rc.expect(m, [q]) == [want], (label, q)


def test_the_hand_cases_say_what_their_names_say():
    h = rc.hand_cases()
    # touch on either side misses, one base of overlap on either side hits
    assert h["touch_misses_one_base_hits"][1][:4] == [((0, 50, 100), 0), ((0, 200, 250), 0), ((0, 50, 101), 1), ((0, 199, 250), 1)]
    # qs == qe inside an interval
    assert ((0, 150, 150), 0) in h["empty_query_inside"][1]
    assert any(q[1] < 0 and hit for q, hit in h["negative_start"][1])
    # a query beyond a thousand later-starting intervals that only the early one covers
    ivs, qs = h["long_early_interval"]
    (c, s, e), hit = qs[0]
    assert hit == 1 and sum(1 for ci, si, ei in ivs if ci == c and si < e and s < ei) == 1 and sum(1 for ci, si, ei in ivs if ci == c and si < s) == 1001
    # contig A's last interval reaches far beyond the query on contig B, which sits before B's first start
    ivs, qs = h["last_of_A_reaches_far"]
    (c, s, e), hit = qs[0]
    assert hit == 0 and c == 1 and e <= min(si for ci, si, _ in ivs if ci == 1) and max(ei for ci, _, ei in ivs if ci == 0) > e


def test_against_covered_bases():
    """an independent statement: a query hits iff one of its bases is covered"""
    ivs = [(c, s % 3000, s % 3000 + (e - s) % 40 + 1) for c, s, e in rc.intervals(300, 5)]
    m = rc.as_model(ivs)
    covered = [set(), set(), set(), set()]
    for c, s, e in ivs:
        covered[c].update(range(s, e))
    for c in range(4):
        for s in range(-3, 3050, 7):
            for w in (0, 1, 2, 9, 60):
                assert m.hit(rc.NAMES[c], s, s + w) == any(b in covered[c] for b in range(s, s + w)), (c, s, w)


def test_the_bounds_and_the_names():
    m = im.IntervalModel(["a", "b"])
    m.add([("a", 0, 1), ("b", im.MAX_END - 1, im.MAX_END)])
    assert m.count() == 2
    for k, bad in enumerate([("a", -1, 5), ("a", 5, 5), ("a", 6, 5), ("a", 0, im.MAX_END + 1), ("c", 1, 2)]):
        with pytest.raises(im.BadInterval) as e:
            m.add([("a", 1, 2)] * k + [bad] + [("b", 1, 2)])
        assert e.value.index == k and m.count() == 2  # named by its index, and nothing of that add is taken
    with pytest.raises(ValueError):
        im.IntervalModel(["a", "a"])
    # names are bytes as they stand
    assert m.hit(b"a", 0, 1) and m.hit("a", 0, 1) and not m.hit("A", 0, 1) and not m.hit("a ", 0, 1) and not m.hit("", 0, 1)


def test_seeded_cases_hit_and_miss():
    """the queries the GPU tests draw do both, at every kind of edge"""
    ivs = rc.intervals(5000, 11)
    want = rc.expect(rc.as_model(ivs), rc.queries(ivs, 4000, 12))
    assert 800 < sum(want) < 3200
    for blocks_case in (rc.long_at_front(), rc.long_at_end_of_a()):
        ivs, qs = blocks_case
        assert rc.expect(rc.as_model(ivs), [q for q, _ in qs]) == [h for _, h in qs]


def test_rpm_columns_are_per_row():
    m = im.IntervalModel(["chr1"])
    m.add([("chr1", 100, 110)])
    row = b"\t".join([b"q", b"chr1", b"3", b"8S50M", b"-8", b"0", b"chr1", b"105", b"117"] + [b"x"] * 12)
    assert im.rpm_columns(m, row) == b"\t0\t1"
    row2 = b"\t".join([b"q", b"chr1", b"3", b"8S50M", b"109", b"120", b"chrU", b"105", b"117"] + [b"x"] * 12)
    assert im.rpm_columns(m, row2) == b"\t1\t0"
    assert im.bed_text([("chr1", 1, 2), (b"c", 3, 4)]) == b"chr1\t1\t2\nc\t3\t4\n"
