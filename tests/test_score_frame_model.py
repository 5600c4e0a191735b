"""The column-drift frame of the eight-lane score pass, on the CPU: a numpy model of the packed arithmetic the device does
(tests/score_frame_model.py: 16-bit halves, scale 8, the key that wraps mod 2^16, 32-step folds) against the oracle's scalar
Smith-Waterman on score and end cell, framed and unframed; ties; and windows up to the bound the host frames and past it."""
import numpy as np
import pytest

import score_frame_model as M

DEFAULT = dict(match=2, mismatch=-3, open_=10, ext=2)
STEEP = dict(match=2, mismatch=-3, open_=12, ext=6)   # a large ext: the drift reaches the bound near 600 columns


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[k] for k in rng.integers(0, len(letters), size=n))


def _params(oracle, sc):
    p = oracle.default_params()
    p.open, p.ext, p.match, p.mismatch = sc["open_"], sc["ext"], sc["match"], sc["mismatch"]
    return p


def _check(oracle, pairs, R, sc, expect_peak_below=M.F16_INF):
    framed, peak = M.score_pass(pairs, R, frame=True, **sc)
    plain, _ = M.score_pass(pairs, R, frame=False, **sc)
    assert framed == plain
    assert peak < expect_peak_below, peak
    p = _params(oracle, sc)
    for i, (q, r) in enumerate(pairs):
        o = oracle.sw(q, r, params=p, ops_cap=4)
        if o["score"] == 0:
            assert framed[i][0] == 0, (i, framed[i])
        else:
            assert framed[i] == (o["score"], o["end_query"], o["end_ref"]), (i, framed[i], o)
    return framed


def _with_indel(rng, q, gap, in_ref):
    """A copy of q for the window: `gap` bases inserted into it (a gap in the query) or cut from it (a gap in the window)."""
    at = int(rng.integers(10, len(q) - 10 - gap))
    return q[:at] + _seq(rng, gap) + q[at:] if in_ref else q[:at] + q[at + gap:]


@pytest.mark.parametrize("R,lq", [(5, 36), (7, 50), (10, 76), (13, 101), (19, 150)])
def test_random_pairs_and_planted_copies_with_indels(oracle, R, lq):
    rng = np.random.default_rng(100 + R)
    pairs = []
    for k in range(12):  # unrelated query and window, four letters and two
        letters = "ACGT" if k % 3 else "AC"
        pairs.append((_seq(rng, lq - k % 3, letters), _seq(rng, 60 + 11 * k, letters)))
    for gap in (1, 2, 3, 5, 7, 11, 15, 20):
        for in_ref in (False, True):
            if gap + 22 > lq:
                continue
            q = _seq(rng, lq)
            copy = _with_indel(rng, q, gap, in_ref)
            left = int(rng.integers(0, 60))
            pairs.append((q, _seq(rng, left) + copy + _seq(rng, int(rng.integers(0, 60)))))
    for sc in (DEFAULT, STEEP, dict(match=1, mismatch=-1, open_=2, ext=1), dict(match=3, mismatch=-4, open_=10, ext=10)):
        _check(oracle, pairs, R, sc)


def test_ties_take_the_smallest_reference_index_then_the_smallest_query_index(oracle):
    rng = np.random.default_rng(7)
    R, lq = 19, 150
    q = _seq(rng, lq)
    sep = "T" * 40 if q[0] != "T" else "A" * 40
    pairs, firsts = [], []
    # two equal copies of the whole query, and of a piece of it, at every lane offset of the first copy
    for left in range(0, 24, 3):
        pairs.append((q, _seq(rng, left) + q + sep + q + _seq(rng, 9)))
        firsts.append((2 * lq, lq - 1, left + lq - 1))
    piece = q[31:99]
    for left in (0, 5, 16):
        pairs.append((q, "G" * left + piece + sep + piece))
        firsts.append(None)
    # the same best score ending in two rows of one column: a query that repeats itself against one copy of the unit
    unit = _seq(rng, 30)
    pairs.append((unit + "T" * 25 + unit, "G" * 12 + unit + "G" * 12))
    firsts.append((60, 29, 12 + 29))
    got = _check(oracle, pairs, R, DEFAULT)
    for g, f in zip(got, firsts):
        if f is not None:
            assert g == f, (g, f)


@pytest.mark.parametrize("R,sc", [(19, STEEP), (5, DEFAULT), (19, DEFAULT)])
def test_windows_up_to_the_bound_and_one_past_it(oracle, R, sc):
    rows = M.LG * R
    L = M.longest_framed_window(sc["match"], sc["open_"], sc["ext"], rows)
    assert 200 < L < 2044
    fits = lambda lr: M.frame_fits(sc["match"], sc["open_"], sc["ext"], rows, M.host_steps(lr))  # noqa: E731
    assert fits(L) and not fits(L + 1) and not fits(2044) and fits(300)
    # the bound is the inequality itself: the last steps it admits, and the first it refuses
    s = M.host_steps(L)
    top = lambda steps: 8 * sc["match"] * rows + 8 * sc["ext"] * (steps + M.LG + 1) + 8 * sc["open_"] + 120  # noqa: E731
    assert top(s) < M.F16_INF <= top(M.host_steps(L + 1))
    # a full-length copy of the query at the very end of the longest framed window: the highest score under the largest drift
    rng = np.random.default_rng(R)
    q = _seq(rng, rows)
    pairs = [(q, _seq(rng, L - rows) + q), (q, q + _seq(rng, L - rows)), (q[:rows - 3], _seq(rng, L))]
    got = _check(oracle, pairs, R, sc)
    assert got[0] == (sc["match"] * rows, rows - 1, L - 1)
    # one column past it the model still runs (the bound keeps a margin), but the host must not frame the launch
    _check(oracle, [(q, _seq(rng, L + 1 - rows) + q)], R, sc, expect_peak_below=1 << 15)


def test_the_frame_refuses_scorings_it_cannot_hold():
    assert M.frame_fits(2, 10, 2, 152, 360)
    assert not M.frame_fits(2, 2, 3, 152, 360)       # ext > open: floorE would fall below the drift
    assert not M.frame_fits(-1, 10, 2, 152, 360)
    assert not M.frame_fits(15, 0, 0, 304, 360)      # the score alone passes the f16 infinity
