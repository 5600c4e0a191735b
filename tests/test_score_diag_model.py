"""The row-and-step drift frame of the eight-lane score pass, on the CPU: tests/score_diag_model.py against the oracle's scalar
Smith-Waterman and against the unframed model (score_frame_model.score_pass(frame=False)) on score and end cell; ties inside
a row pair, across lanes and across key windows; gaps over the lane hand-off; open == ext and ext == 0; and the bound."""
import numpy as np
import pytest

import score_diag_model as D
import score_frame_model as M

DEFAULT = dict(match=2, mismatch=-3, open_=10, ext=2)
SCORINGS = [DEFAULT, dict(match=2, mismatch=-3, open_=12, ext=6), dict(match=1, mismatch=-1, open_=2, ext=1),
            dict(match=2, mismatch=-4, open_=10, ext=10), dict(match=2, mismatch=-3, open_=6, ext=0)]


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[k] for k in rng.integers(0, len(letters), size=n))


def _params(oracle, sc):
    p = oracle.default_params()
    p.open, p.ext, p.match, p.mismatch = sc["open_"], sc["ext"], sc["match"], sc["mismatch"]
    return p


def _check(oracle, pairs, R, sc):
    assert D.diag_fits(sc["match"], sc["open_"], sc["ext"], 8 * R, M.host_steps(max(len(r) for _, r in pairs)))
    got, peak = D.score_pass_diag(pairs, R, **sc)
    plain, _ = M.score_pass(pairs, R, frame=False, **sc)
    assert got == plain
    assert peak < M.F16_INF, peak
    p = _params(oracle, sc)
    for i, (q, r) in enumerate(pairs):
        o = oracle.sw(q, r, params=p, ops_cap=4)
        if o["score"] == 0:
            assert got[i][0] == 0, (i, got[i])
        else:
            assert got[i] == (o["score"], o["end_query"], o["end_ref"]), (i, got[i], o)
    return got, peak


@pytest.mark.parametrize("R,lq", [(5, 36), (7, 50), (10, 76), (13, 101), (19, 150)])
def test_random_pairs_and_planted_copies_with_indels(oracle, R, lq):
    rng = np.random.default_rng(200 + R)
    pairs = []
    for k in range(12):  # unrelated query and window; two letters make ties everywhere
        letters = "ACGT" if k % 3 else "AC"
        pairs.append((_seq(rng, lq - k % 3, letters), _seq(rng, 60 + 11 * k, letters)))
    for gap in (1, 2, 3, 5, 7, 11, 15, 20):
        for in_ref in (False, True):
            if gap + 22 > lq:
                continue
            q = _seq(rng, lq)
            at = int(rng.integers(10, lq - 10 - gap))
            copy = q[:at] + _seq(rng, gap) + q[at:] if in_ref else q[:at] + q[at + gap:]
            pairs.append((q, _seq(rng, int(rng.integers(0, 60))) + copy + _seq(rng, int(rng.integers(0, 60)))))
    for sc in SCORINGS:
        _check(oracle, pairs, R, sc)


def test_ties_inside_a_pair_across_lanes_and_across_key_windows(oracle):
    rng = np.random.default_rng(11)
    R, lq = 19, 150
    q = _seq(rng, lq)
    sep = "T" * 40 if q[0] != "T" else "A" * 40
    pairs, want = [], []
    # two equal copies of the whole query more than 32 steps apart (two key windows), at every lane offset of the first
    for left in range(0, 24, 3):
        pairs.append((q, _seq(rng, left) + q + sep + q + _seq(rng, 9)))
        want.append((2 * lq, lq - 1, left + lq - 1))
    # the same best score in two neighbouring rows of one column: 31 A in the query against 30 in the window score 60 in rows
    # first + 29 and first + 30 of the window's last A.  first = 0, 9: the even and the odd row of one pair (lane-local rows
    # 10 / 11 and 0 / 1); 1: two pairs of a lane; 8, 27: the last row of a lane and the first of the next (rows 37 / 38, 56 / 57)
    for first in (0, 9, 1, 8, 27):
        qq = "T" * first + "A" * 31
        pairs.append((qq + "T" * (lq - len(qq)), "G" * 12 + "A" * 30 + "G" * 12))
        want.append((60, first + 29, 12 + 29))
    got, _ = _check(oracle, pairs, R, DEFAULT)
    for g, f in zip(got, want):
        if f is not None:
            assert g == f, (g, f)


@pytest.mark.parametrize("sc", SCORINGS, ids=lambda s: "%(match)d_%(mismatch)d_%(open_)d_%(ext)d" % s)
def test_gaps_over_the_lane_hand_off_and_along_a_row(oracle, sc):
    rng = np.random.default_rng(5 + sc["ext"])
    R, lq = 7, 56
    pairs = []
    for gap in (1, 2, 6, 9):
        q = _seq(rng, lq)
        for cut in (R - 1, R, 2 * R, 3 * R - 1):   # F runs down `gap` rows from row `cut`: over one or two lane boundaries
            pairs.append((q, _seq(rng, 13) + q[:cut] + q[cut + gap:] + _seq(rng, 8)))
        # E runs along one row for `gap` and for 40 columns (a long horizontal gap: the decay is the frame's own)
        pairs.append((q, _seq(rng, 5) + q[:25] + _seq(rng, gap) + q[25:]))
    q = _seq(rng, lq)
    pairs.append((q, q[:28] + _seq(rng, 40) + q[28:]))
    pairs.append((q, q[:28] + "".join("ACGT"[("ACGT".index(c) + 1) % 4] for c in q[:40]) + q[28:]))
    _check(oracle, pairs, R, sc)


@pytest.mark.parametrize("R,sc", [(19, DEFAULT), (5, DEFAULT), (19, SCORINGS[1]), (13, SCORINGS[3])])
def test_windows_up_to_the_bound_and_one_past_it(oracle, R, sc):
    rows = M.LG * R
    m, o, e = sc["match"], sc["open_"], sc["ext"]
    L = D.longest_diag_window(m, o, e, rows)
    assert 200 < L < 2044
    fits = lambda lr: D.diag_fits(m, o, e, rows, M.host_steps(lr))  # noqa: E731
    assert fits(L) and not fits(L + 1) and fits(300)
    # the bound is the host's inequality, term for term
    top = lambda steps: 8 * m * rows + 8 * e * (steps + R - 1 + D.C0) + 8 * o + 8 * (15 + e)  # noqa: E731
    keytop = 64 * m * rows + 63 + 128 * e * (R - 1) // 2
    assert keytop < M.F16_INF and 8 * (15 + e) <= 255
    assert top(M.host_steps(L)) < M.F16_INF <= top(M.host_steps(L + 1))
    # at 19 rows per lane it is the tighter of the two frames: past it the host still has the column-drift frame
    if R == 19:
        assert M.frame_fits(m, o, e, rows, M.host_steps(L + 1))
    rng = np.random.default_rng(R)
    q = _seq(rng, rows)
    pairs = [(q, _seq(rng, L - rows) + q), (q, q + _seq(rng, L - rows)), (q[:rows - 3], _seq(rng, L))]
    got, peak = _check(oracle, pairs, R, sc)
    assert got[0] == (m * rows, rows - 1, L - 1)
    assert peak < M.F16_INF


def test_the_frame_refuses_scorings_it_cannot_hold():
    assert D.diag_fits(2, 10, 2, 152, 360)
    assert not D.diag_fits(3, 12, 6, 152, 360)       # the offset key passes the f16 infinity (the column-drift frame still fits)
    assert M.frame_fits(3, 12, 6, 152, 360)
    assert not D.diag_fits(2, 2, 3, 152, 360)        # ext > open
    assert not D.diag_fits(-1, 10, 2, 152, 360)
    assert not D.diag_fits(1, 20, 17, 40, 100)       # a table byte of 8 (15 + 17) = 256
    assert D.diag_fits(1, 20, 16, 40, 100)
    assert D.diag_fits(2, 6, 0, 152, 4000)           # ext == 0: no drift, any window
