"""The eight-lane score pass with the drift along the row as well (sw_pk_kernel<R8, 1, false, 8, false, 0, true, true>) against
the column-drift frame (FADEHIP_SCORE_DIAG=0), the unframed pass (FADEHIP_SCORE_FRAME=0) and the oracle: every batch runs three
times, rs / aln / stats must agree byte for byte, rs and am must be the oracle's, and the library's debug line names the tier
each run took.  One library per eight-lane instantiation; constructed 150-base records whose windows are written out column by
column (best cells in the first and last row and column and on the lane seam, the ties of tests/test_score_diag_model.py, gaps
over the hand-off, an N in the query), held cell for cell to the oracle's Smith-Waterman through trace_all; a scoring that fits
the frame's bound and one that must fall back; and windows on both sides of the bound."""
import os

import numpy as np
import pytest

import fade_amd
import samutil
import score_diag_model as D
import score_frame_model as M
from fade_amd import format_tags

pytestmark = pytest.mark.gpu

TIER_ENV = {2: {}, 1: {"FADEHIP_SCORE_DIAG": "0"}, 0: {"FADEHIP_SCORE_FRAME": "0"}}


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTNRYKMSWBDHV", "TGCANYRMKSWVHDB"))


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[k] for k in rng.integers(0, len(letters), size=n))


def _annotate(names, seqs, batch, floor_len, window, tier, capfd, trace_all=False, **scoring):
    """One context, one batch: (rs, aln sorted by record, stats, the context's debug output)."""
    env = dict(TIER_ENV[tier], FADEHIP_DEBUG="1")
    os.environ.update(env)
    try:
        c = fade_amd.Context(device=0, trace_all=trace_all, **scoring)
    finally:
        for k in env:
            del os.environ[k]
    try:
        capfd.readouterr()
        c.genome_upload(names, [s.encode() if isinstance(s, str) else s for s in seqs])
        rs, aln, st = c.annotate(batch, floor_len, window)
    finally:
        c.close()
    err = capfd.readouterr().err
    return rs, aln[np.argsort(aln["read_idx"], kind="stable")], list(st), err


def _three_and_oracle(oracle, names, seqs, batch, floor_len, window, capfd, tier, column_fits=True, rows16=None, **scoring):
    """tier: what the unrestricted run must take (2 row drift, 1 column drift, 0 unframed; None: the scoring is outside the
    two-pass path altogether, the library takes its single-pass kernels and no score pass runs)."""
    runs = [_annotate(names, seqs, batch, floor_len, window, t, capfd, **scoring) for t in (2, 1, 0)]
    want = [tier, min(tier, 1) if column_fits else 0, 0] if tier is not None else [None] * 3
    for (rs, aln, st, err), w in zip(runs, want):
        if w is None:
            assert "single-pass kernels" in err and "eight-lane groups" not in err and "row drift on" not in err, err[-300:]
            continue
        assert "eight-lane groups" in err, err[-300:]
        assert ("column-drift frame on, row drift %s" % ("on" if w == 2 else "off") in err) == (w >= 1), (w, err[-300:])
        assert ("column-drift frame off, row drift off" in err) == (w == 0), (w, err[-300:])
    rs2, aln2, st2, err2 = runs[0]
    if rows16 is not None and tier is not None:
        assert "class of %d rows" % rows16 in err2 and "longest read of the batch: %d)" % int(batch["l_seq"].max()) in err2, err2[-300:]
    for rs, aln, st, _ in runs[1:]:
        assert np.array_equal(rs2, rs) and st2 == st
        assert aln2.tobytes() == aln.tobytes()
    p = oracle.default_params()
    for k, v in scoring.items():
        setattr(p, k, v)
    G = oracle.GenomeHolder(names, seqs)
    ors, oam = oracle.annotate_batch_soa(G, batch, floor_len, window, threads=8, params=p)
    assert np.array_equal(rs2, ors), np.nonzero(rs2 != ors)[0][:10]
    tags = format_tags(batch, names, rs2, aln2)
    for i in range(len(ors)):
        if oam[i] is None:
            assert i not in tags
        else:
            assert tags[i]["am"] == oam[i], i
    return rs2, aln2, tags


@pytest.mark.parametrize("read_len,rows16", [(36, 64), (50, 64), (76, 96), (100, 128), (150, 160)])
def test_every_eight_lane_instantiation_three_ways(oracle, capfd, read_len, rows16):
    """<5>, <7>, <10>, <13>, <19>: a library of one read length picks each."""
    from fade_amd import synth
    cfg = synth.config("C5")
    cfg.update(read_len=read_len, contig_len=40_000, insert_mu=max(cfg["insert_mu"], read_len + 150),
               clip_max=min(cfg["clip_max"], read_len // 2), window=100, p_sc=0.9)
    g = synth.Genome(2, cfg["contig_len"], 29)
    b = synth.make_reads(g, 400, 700 + read_len, **{k: v for k, v in cfg.items() if k in (
        "read_len", "window", "p_sc", "clip_min", "clip_max", "insert_mu", "insert_sd")})
    b.pop("_truth", None)
    seqs = [a.tobytes().decode() for a in g.ascii_contigs()]
    rs, aln, tags = _three_and_oracle(oracle, g.names, seqs, b, cfg["floor_len"], 100, capfd, 2, rows16=rows16)
    assert len(tags) > 5


class _Records:
    """Records whose windows are given column by column: the contig is the windows laid end to end between spacers, a record
    with `clip` soft-clipped bases at one end is placed so that the library's window (w columns either side of its aligned
    bases) is exactly the string it was given."""

    def __init__(self, rng, w, lq=150):
        self.rng, self.w, self.lq = rng, w, lq
        self.contig, self.recs, self.windows = _seq(rng, 300, "CG"), [], []

    def win_len(self, clip):
        return self.lq - clip + 2 * self.w

    def add(self, q, window, clip=20, right=False):
        assert len(q) == self.lq and len(window) == self.win_len(clip), (len(q), len(window))
        p = len(self.contig) + self.w
        self.contig += window + _seq(self.rng, 40, "CG")
        al = self.lq - clip
        self.recs.append(("c1", p, ("%dM%dS" % (al, clip)) if right else ("%dS%dM" % (clip, al)), q))
        self.windows.append(window)

    def batch(self):
        lines = ["\t".join(["r%d" % i, "0", c, str(pos + 1), "60", cig, "*", "0", "0", _rc(q), "I" * len(q)])
                 for i, (c, pos, cig, q) in enumerate(self.recs)]
        self.contig += _seq(self.rng, 300, "CG")
        text = "@SQ\tSN:c1\tLN:%d\n" % len(self.contig) + "\n".join(lines) + "\n"
        names, lens, batch, qnames = samutil.sam_to_batch(text)
        return names, [self.contig], batch


def _put(q, at, piece):
    return q[:at] + piece + q[at + len(piece):]


def _cells_against_the_oracle(oracle, R, names, seqs, batch, w, capfd, **scoring):
    """trace_all reports the score pass's end cell of every re-aligned record: each is the oracle's Smith-Waterman of (query as
    the score pass sees it, the record's window).  Returns {record: (score, end_query, end_ref)}."""
    rs, aln, st, err = _annotate(names, seqs, batch, 5, w, 2, capfd, trace_all=True, **scoring)
    assert "row drift on" in err, err[-300:]
    p = oracle.default_params()
    for k, v in scoring.items():
        setattr(p, k, v)
    got = {}
    for a in aln:
        i = int(a["read_idx"])
        if set(R.recs[i][3]) - set("ACGT"):   # (wildcards: held to the oracle's records above, not to its plain Smith-Waterman)
            continue
        assert R.windows[i] == R.contig[int(a["win_start"]):int(a["win_start"]) + int(a["win_len"])], i
        o = oracle.sw(R.recs[i][3], R.windows[i], params=p, ops_cap=4)
        cell = (int(a["sw"]["score"]), int(a["sw"]["end_query"]), int(a["sw"]["end_ref"]))
        assert cell == ((o["score"], o["end_query"], o["end_ref"]) if o["score"] else (0, 0, 0)), (i, cell, o)
        got[i] = cell
    return got


def test_constructed_records_cell_for_cell(oracle, capfd):
    rng = np.random.default_rng(31)
    w, lq = 100, 150
    R = _Records(rng, w)
    L = R.win_len(20)
    cg = lambda n: _seq(rng, n, "CG")  # noqa: E731
    expect = {}

    def single(row, col):
        """One A in the query (row `row`) and one in the window (column `col`): the best cell is that cell, score = match."""
        expect[len(R.recs)] = (2, row, col)
        R.add("T" * row + "A" + "T" * (lq - 1 - row), _put(cg(L), col, "A"))

    for row in (0, 18, 19, 149):            # the first row, both sides of the first lane seam, the last row
        for col in (0, L - 1, 57):          # the first and the last column of the window
            single(row, col)
    # copies that start in row 0 / column 0 and that end in the last row / last column; through every lane; over the seams
    q = _seq(rng, lq)
    R.add(q, q[:140] + _seq(rng, L - 140), right=True)
    R.add(q, _seq(rng, L - 140) + q[10:])
    R.add(q, _seq(rng, 33) + q + _seq(rng, L - 33 - lq))
    R.add(_put(_seq(rng, lq), 5, q[5:40]), _seq(rng, 60) + q[5:40] + _seq(rng, L - 95), right=True)     # rows 5 .. 39: over rows 18 / 19
    R.add(_put(_seq(rng, lq), 60, q[60:95]), _seq(rng, 150) + q[60:95] + _seq(rng, L - 185))           # rows 60 .. 94: over 75 / 76
    # the ties of the model: equal scores in neighbouring rows of one column (inside a pair, across pairs, across lanes) ...
    for first in (0, 9, 1, 8, 27):
        expect[len(R.recs)] = (60, first + 29, 12 + 29)
        qq = "T" * first + "A" * 31
        R.add(qq + "T" * (lq - len(qq)), "G" * 12 + "A" * 30 + cg(L - 42))
    # ... and two equal copies of a piece more than 32 steps apart (two key windows), at several lane offsets
    piece = q[31:99]
    for left in (0, 5, 16, 23):
        expect[len(R.recs)] = (2 * len(piece), 98, left + len(piece) - 1)
        R.add(_put("T" * lq, 31, piece.replace("T", "A")), cg(left) + piece.replace("T", "A") + cg(50) + piece.replace("T", "A") + cg(L - left - 50 - 2 * len(piece)))
    # gaps: bases missing from the query (E runs along a row) and bases the window lacks (F runs down rows, across lane seams)
    for gap in (1, 7, 20):
        W = _seq(rng, L)
        R.add(_put(_seq(rng, lq), 15, W[70:130] + W[130 + gap:205 + gap]), W)
        R.add(_put(_seq(rng, lq), 15, W[70:125] + _seq(rng, gap) + W[125:125 + 80 - gap]), W)
        R.add(_put(_seq(rng, lq), 3, W[40:55] + _seq(rng, gap) + W[55:55 + 100 - gap]), W, right=True)   # the cut sits at rows 18 ..
    W = _seq(rng, L)
    R.add(_put(_seq(rng, lq), 10, W[20:80] + W[140:200]), W)                       # a long horizontal gap: 60 columns
    # an N and an IUPAC base in the query: the octet takes the general sweep
    W = _seq(rng, L)
    R.add(_put(_put(_put(_seq(rng, lq), 20, W[90:220]), 40, "N"), 90, "R"), W)
    R.add(_put(_put(_seq(rng, lq), 0, W[:60]), 7, "Y"), W, right=True)
    R.add("T" * lq, cg(L))                                                          # nothing matches
    names, seqs, batch = R.batch()
    rs, aln, tags = _three_and_oracle(oracle, names, seqs, batch, 5, w, capfd, 2, rows16=160)
    cells = _cells_against_the_oracle(oracle, R, names, seqs, batch, w, capfd)
    assert len(cells) >= 8
    for i, e in expect.items():   # (a record the library does not report has no cell to show)
        if i in cells:
            assert cells[i] == e, (i, cells[i], e)


@pytest.mark.parametrize("scoring,tier,w", [(dict(open=10, ext=4, match=2, mismatch=-4), 2, 100), (dict(open=12, ext=6, match=3, mismatch=-1), None, 100),
                                            (dict(open=12, ext=11, match=2, mismatch=-3), 1, 20), (dict(open=4, ext=4, match=2, mismatch=-3), 2, 100)],
                         ids=["fits", "falls_back", "key_bound", "open_eq_ext"])
def test_other_scorings_fit_or_fall_back(oracle, capfd, scoring, tier, w):
    """2 / -4 / 10 / 4 fits the bound.  3 / -1 / 12 / 6 at 152 rows does not (its offset key passes the f16 infinity) and must fall
    back with the same bytes: a match above 2 takes the library out of the two-pass path, so what it falls back to are the
    single-pass kernels, whatever the switches say.  2 / -3 / 12 / 11 fails the same key bound inside the two-pass path and runs in
    the column-drift frame (at -w 20, where that frame's own bound still holds).  With open == ext the floor of E is the drift itself."""
    lq = 150
    steps = M.host_steps(lq - 10 + 2 * w)
    assert D.diag_fits(scoring["match"], scoring["open"], scoring["ext"], 152, steps) == (tier == 2)
    assert M.frame_fits(scoring["match"], scoring["open"], scoring["ext"], 152, steps)
    rng = np.random.default_rng(scoring["ext"] + 40)
    R = _Records(rng, w)
    for k in range(240):
        clip = 10 + k % 3 * 10
        L = R.win_len(clip)
        W = _seq(rng, L)
        q = _seq(rng, lq)
        if k % 4 == 0:
            q = _put(q, 10, W[L - 140 - k % 5:L - k % 5])
        elif k % 4 == 1:
            q = _put(q, 0, W[k % 7:k % 7 + 120])
        elif k % 4 == 2:
            g = 1 + k % 9
            q = _put(q, 20, W[20:80] + W[80 + g:150 + g]) if k % 8 == 2 else _put(q, 20, W[20:75] + _seq(rng, g) + W[75:75 + 75 - g])
        R.add(q, W, clip=clip, right=(k % 4 == 1))
    names, seqs, batch = R.batch()
    rs, aln, tags = _three_and_oracle(oracle, names, seqs, batch, 5, w, capfd, tier, rows16=160, **scoring)
    assert len(aln) >= 100
    if tier == 2:
        assert len(_cells_against_the_oracle(oracle, R, names, seqs, batch, w, capfd, **scoring)) >= 100


def test_windows_on_both_sides_of_the_bound(oracle, capfd):
    """200 reads at the largest -w whose launch the host still sweeps with the row drift, and at the next: the debug line shows it
    on, then off with the column-drift frame on (at 152 rows that frame's bound is the wider one), and the bytes do not move."""
    rng = np.random.default_rng(77)
    lq, clip = 150, 6
    aligned = lq - clip
    fits = lambda w: D.diag_fits(2, 10, 2, 152, M.host_steps(aligned + 2 * w))  # noqa: E731
    w_in = max(w for w in range(50, 1000) if fits(w))
    w_out = w_in + 1
    assert not fits(w_out) and M.frame_fits(2, 10, 2, 152, M.host_steps(aligned + 2 * w_out)) and 800 < w_in < 830
    ref = _seq(rng, 60_000)
    recs = []
    for k in range(200):
        p = 2_000 + 270 * k
        W = ref[p - w_in:p + aligned + w_in]
        q = _seq(rng, lq)
        if k % 4 == 0:    # a copy of most of the query at the far end of the window: a high score under the largest drift
            q = _put(q, 10, W[len(W) - 140 - k % 3:len(W) - k % 3])
        elif k % 4 == 1:  # ... at its start (an artifact under a right clip)
            q = _put(q, 0, W[:120])
        elif k % 4 == 2:  # ... with a gap
            q = _put(q, 20, W[len(W) // 2:len(W) // 2 + 60] + W[len(W) // 2 + 67:len(W) // 2 + 137])
        recs.append(("c1", p, ("%dM%dS" % (aligned, clip)) if k % 4 == 1 else ("%dS%dM" % (clip, aligned)), q))
    lines = ["\t".join(["r%d" % i, "0", c, str(pos + 1), "60", cig, "*", "0", "0", _rc(q), "I" * len(q)])
             for i, (c, pos, cig, q) in enumerate(recs)]
    names, lens, batch, qnames = samutil.sam_to_batch("@SQ\tSN:c1\tLN:%d\n" % len(ref) + "\n".join(lines) + "\n")
    for w, tier in ((w_in, 2), (w_out, 1)):
        rs, aln, tags = _three_and_oracle(oracle, names, [ref], batch, 5, w, capfd, tier, rows16=160)
        assert len(aln) >= 140 and int(aln["win_len"].max()) == aligned + 2 * w
