"""The eight-lane score pass in its column-drift frame (sw_pk_kernel<R8, 1, false, 8, false, 0, true>) against the same pass
without it (FADEHIP_SCORE_FRAME=0) and against the oracle: every batch runs twice, rs / aln / stats must agree byte for
byte, rs and am must be the oracle's, and the library's debug line says which kernel each run took.  One library per
eight-lane instantiation; constructed 150-base records at the places where the frame has a boundary of its own; and
windows on both sides of the bound past which the host must fall back (default scoring, and a steep ext)."""
import os

import numpy as np
import pytest

import fade_amd
import samutil
import score_frame_model as M
from fade_amd import format_tags, synth

pytestmark = pytest.mark.gpu

IUPAC = "NRYKMSWBDHV"


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTNRYKMSWBDHV", "TGCANYRMKSWVHDB"))


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[k] for k in rng.integers(0, len(letters), size=n))


def _annotate(names, seqs, batch, floor_len, window, frame, capfd, **scoring):
    """One context, one batch: (rs, aln sorted by record, stats, the context's debug output)."""
    os.environ["FADEHIP_DEBUG"] = "1"
    if not frame:
        os.environ["FADEHIP_SCORE_FRAME"] = "0"
    try:
        c = fade_amd.Context(device=0, **scoring)
    finally:
        del os.environ["FADEHIP_DEBUG"]
        os.environ.pop("FADEHIP_SCORE_FRAME", None)
    try:
        capfd.readouterr()
        c.genome_upload(names, [s.encode() if isinstance(s, str) else s for s in seqs])
        rs, aln, st = c.annotate(batch, floor_len, window)
    finally:
        c.close()
    err = capfd.readouterr().err
    return rs, aln[np.argsort(aln["read_idx"], kind="stable")], list(st), err


def _both_and_oracle(oracle, names, seqs, batch, floor_len, window, capfd, expect_framed, rows16=None, **scoring):
    rs1, aln1, st1, err1 = _annotate(names, seqs, batch, floor_len, window, True, capfd, **scoring)
    rs0, aln0, st0, err0 = _annotate(names, seqs, batch, floor_len, window, False, capfd, **scoring)
    assert "eight-lane groups" in err1 and "eight-lane groups" in err0, (err1[-300:], err0[-300:])
    assert ("column-drift frame on" in err1) == expect_framed and "column-drift frame on" not in err0, err1[-300:]
    assert ("column-drift frame off" in err1) == (not expect_framed) and "column-drift frame off" in err0, err0[-300:]
    if rows16 is not None:
        assert "class of %d rows" % rows16 in err1 and "longest read of the batch: %d)" % int(batch["l_seq"].max()) in err1, err1[-300:]
    assert np.array_equal(rs1, rs0) and st1 == st0
    assert aln1.tobytes() == aln0.tobytes()
    p = oracle.default_params()
    for k, v in scoring.items():
        setattr(p, k, v)
    G = oracle.GenomeHolder(names, seqs)
    ors, oam = oracle.annotate_batch_soa(G, batch, floor_len, window, threads=8, params=p)
    assert np.array_equal(rs1, ors), np.nonzero(rs1 != ors)[0][:10]
    tags = format_tags(batch, names, rs1, aln1)
    for i in range(len(ors)):
        if oam[i] is None:
            assert i not in tags
        else:
            assert tags[i]["am"] == oam[i], i
    return rs1, aln1, tags


@pytest.mark.parametrize("read_len,rows16", [(36, 64), (50, 64), (76, 96), (101, 128), (150, 160)])
def test_every_eight_lane_instantiation_framed_and_unframed(oracle, capfd, read_len, rows16):
    """<5>, <7>, <10>, <13>, <19>: a library of one read length picks each (the debug line names the sixteen-lane class and
    the longest read, which together decide the instantiation: g8_kernel)."""
    cfg = synth.config("C5")
    cfg.update(read_len=read_len, contig_len=40_000, insert_mu=max(cfg["insert_mu"], read_len + 150),
               clip_max=min(cfg["clip_max"], read_len // 2), window=100, p_sc=0.9)
    g = synth.Genome(2, cfg["contig_len"], 23)
    b = synth.make_reads(g, 400, 500 + read_len, **{k: v for k, v in cfg.items() if k in (
        "read_len", "window", "p_sc", "clip_min", "clip_max", "insert_mu", "insert_sd")})
    b.pop("_truth", None)
    seqs = [a.tobytes().decode() for a in g.ascii_contigs()]
    rs, aln, tags = _both_and_oracle(oracle, g.names, seqs, b, cfg["floor_len"], 100, capfd, True, rows16)
    assert len(tags) > 5


def _sam_batch(contigs, recs):
    """recs: (contig, pos, cigar, query) with the query as the score pass sees it (the read is its reverse complement)."""
    lines = ["\t".join(["r%d" % i, "0", c, str(pos + 1), "60", cig, "*", "0", "0", _rc(q), "I" * len(q)])
             for i, (c, pos, cig, q) in enumerate(recs)]
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in contigs) + "\n".join(lines) + "\n"
    names, lens, batch, qnames = samutil.sam_to_batch(text)
    return names, [s for _, s in contigs], batch


def _put(q, at, piece):
    return q[:at] + piece + q[at + len(piece):]


def test_constructed_records_at_the_frames_boundaries(oracle, capfd):
    rng = np.random.default_rng(19)
    ref = _seq(rng, 40_000)
    acg = _seq(rng, 4_000, "ACG")
    contigs = [("c1", ref), ("c2", acg)]
    w, lq = 100, 150
    recs = []
    pos = [2_000]

    def add(clip, build, right=False):
        """A record whose window is ref[p - w : p + lq - clip + w]; build(q, W) plants what the case needs.  What the score pass
        finds shows in the output where the record is an artifact: a copy that runs to the end of the query under a left clip,
        one that starts at its first base under a right clip (right=True)."""
        p = pos[0]
        pos[0] += 700
        W = ref[p - w:p + (lq - clip) + w]
        q = build(_seq(rng, lq), W)
        assert len(q) == lq
        recs.append(("c1", p, ("%dM%dS" if right else "%dS%dM") % ((lq - clip, clip) if right else (clip, lq - clip)), q))

    add(20, lambda q, W: _put(q, 0, W[:40]), right=True)                  # row 0, column 0: the exact hd boundary
    add(20, lambda q, W: _put(q, lq - 40, W[-40:]))                       # ends in the last row and the last column
    add(20, lambda q, W: _put(q, 0, W[:140]), right=True)                 # nearly the whole query from column 0
    add(20, lambda q, W: _put(q, 10, W[-140:]))                           # ... and into the last column
    add(20, lambda q, W: _put(q, 0, W[60:95]), right=True)                # across rows 18 / 19 (a lane boundary)
    add(20, lambda q, W: _put(q, 60, W[150:240]))                         # across rows 75 / 76 (a DPP-row boundary)
    add(20, lambda q, W: _put(q, 10, W[33:33 + 140]))                     # through every lane
    for gap in (1, 7, 20):
        # bases missing from the query (E runs along the row for `gap` columns) ...
        add(20, lambda q, W, gap=gap: _put(q, 15, W[70:130] + W[130 + gap:205 + gap]))
        # ... and bases the window lacks (F runs down `gap` rows, across a lane boundary: the cut sits at row 70 .. 90)
        add(20, lambda q, W, gap=gap: _put(q, 15, W[70:125] + _seq(rng, gap) + W[125:125 + 80 - gap]))
        add(30, lambda q, W, gap=gap: _put(q, 0, W[40:113] + _seq(rng, gap) + W[113:113 + 67 - gap]), right=True)
    add(20, lambda q, W: _put(_put(_put(q, 20, W[90:220]), 40, "N"), 90, "R"))      # N and an IUPAC base: the general sweep
    add(20, lambda q, W: _put(_put(q, 0, W[:60]), 7, "Y"), right=True)
    recs.append(("c2", 1_000, "20S130M", "T" * lq))                        # nothing matches: score 0, an all-zero Fwd
    recs.append(("c2", 2_000, "130M20S", "T" * lq))
    names, seqs, batch = _sam_batch(contigs, recs)
    rs, aln, tags = _both_and_oracle(oracle, names, seqs, batch, 5, w, capfd, True, 160)
    assert len(aln) >= 18
    zero = aln[aln["read_idx"] >= len(recs) - 2]["sw"]  # nothing matches: where the record is reported at all, its Fwd is all zero
    assert not zero["score"].any() and not zero["end_query"].any() and not zero["end_ref"].any()

    # the two alignments of a lane pair sweep windows that differ by more than 40 columns: a batch too small for the gate's
    # ordering by window length to bring neighbours together
    recs, pos[0] = [], 3_000
    for clip in (10, 120, 16, 100):
        add(clip, lambda q, W: _put(q, 30, W[len(W) - 125:len(W) - 5]))
    names, seqs, batch = _sam_batch(contigs, recs)
    rs, aln, tags = _both_and_oracle(oracle, names, seqs, batch, 5, w, capfd, True, 160)
    assert sorted(int(x) for x in aln["win_len"]) == [230, 250, 334, 340]


@pytest.mark.parametrize("scoring", [dict(open=10, ext=2, match=2, mismatch=-3), dict(open=12, ext=6, match=2, mismatch=-3)],
                         ids=["default", "steep_ext"])
def test_windows_on_both_sides_of_the_bound(oracle, capfd, scoring):
    """200 reads at the largest -w whose launch the host still frames, and at the next: the debug line must show the frame on
    and off as the bound (score_frame_model.frame_fits, the host's own inequality) says, and the bytes must not move."""
    rng = np.random.default_rng(scoring["ext"])
    lq, clip = 150, 6
    aligned = lq - clip
    fits = lambda w: M.frame_fits(scoring["match"], scoring["open"], scoring["ext"], 152, M.host_steps(aligned + 2 * w))  # noqa: E731
    w_in = max(w for w in range(50, 1000) if fits(w))
    w_out = w_in + 1
    assert not fits(w_out) and aligned + 2 * w_out < 2044
    assert (w_in > 800) == (scoring["ext"] == 2) and (200 < w_in < 230) == (scoring["ext"] == 6)
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
    names, seqs, batch = _sam_batch([("c1", ref)], recs)
    for w, framed in ((w_in, True), (w_out, False)):
        rs, aln, tags = _both_and_oracle(oracle, names, seqs, batch, 5, w, capfd, framed, 160, **scoring)
        assert len(aln) >= 140 and int(aln["win_len"].max()) == aligned + 2 * w
