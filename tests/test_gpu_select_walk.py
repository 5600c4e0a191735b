"""The forced-diagonal walk of the score pass (select_one), four lanes per alignment: constructed artifacts whose walk ends
on and beside 8-, 32- and 128-cell boundaries, ends at the window's first column or the read's first base (the matrix
border), goes negative, or has 9, 10, 11 runs of = / X, with N and IUPAC bases on either side, on both strands, under
both settings of the = / X rules, in the eight-lane (150-base reads) and the sixteen-lane (158-base reads) score kernels.
Every batch is held to the oracle (rs and am) and, byte for byte, to the same batch with the shortcut off
(FADEHIP_NO_SHORTCUT=1: every candidate through the traced pass)."""
import numpy as np
import pytest

import fade_amd
import samutil
from fade_amd import format_tags

pytestmark = pytest.mark.gpu

EQ_BY_CHAR, N_EQ_N = 1 << 3, 1 << 6
DEFAULT = 0x7F
IUPAC = "NRYKMSWBDHV"


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTNRYKMSWBDHV", "TGCANYRMKSWVHDB"))


def _sub(rng, s, k, alphabet="ACGT"):
    """s with positions k changed to another letter of alphabet."""
    s = list(s)
    for p in k:
        s[p] = rng.choice([c for c in alphabet if c != s[p]])
    return "".join(s)


def _records(rng, ref, lq, window):
    """Left and right artifacts of the shapes the walk has to get right; yields (cigar, seq, pos, flag)."""
    out = []
    spans = [1, 7, 8, 9, 16, 31, 32, 33, 40, 63, 64, 65, 96, 100, 120, 127, 128, 129]
    pos = 400
    for L in [s for s in spans if s <= lq - 10] * 3:
        for variant in range(7):
            flag = 16 if (variant & 1) else 0
            seg = pos - (window if variant == 2 else int(rng.integers(L, window + 1)))  # variant 2: the window's first column
            clip = _rc(ref[seg:seg + L])
            if variant == 3 and L >= 12:  # 4, 5 interior mismatches: 9 or 11 runs
                clip = _sub(rng, clip, rng.choice(np.arange(1, L - 1), size=4 + (L % 2), replace=False))
            elif variant == 4 and L >= 12:  # mismatches at both ends and inside: 10 runs or the walk goes negative
                clip = _sub(rng, clip, [0, L - 1] + list(rng.choice(np.arange(2, L - 2), size=3, replace=False)))
            elif variant == 5:  # N / IUPAC in the clip
                clip = _sub(rng, clip, rng.choice(np.arange(L), size=max(1, L // 10), replace=False), IUPAC)
            elif variant == 6 and L >= 4:  # a mismatch or two near the start of the read: P negative before the border
                clip = _sub(rng, clip, sorted(rng.choice(np.arange(min(L, 6)), size=min(2, L // 2), replace=False)))
            body = ref[pos:pos + lq - L]
            if variant & 1:  # right artifact: clip after the aligned part
                seg2 = pos + (lq - L) + int(rng.integers(0, window - L + 1)) if window > L else pos + lq - L
                clip_r = _rc(ref[seg2:seg2 + L])
                if variant == 5:
                    clip_r = _sub(rng, clip_r, rng.choice(np.arange(L), size=max(1, L // 10), replace=False), IUPAC)
                out.append(("%dM%dS" % (lq - L, L), body + clip_r, pos, flag))
            out.append(("%dS%dM" % (L, lq - L), clip + body, pos, flag))
            pos += lq + 2 * window + 50
    return out


def _batch(rng, lq, window):
    n = 330_000
    ref = list("".join("ACGT"[k] for k in rng.integers(0, 4, size=n)))
    for p in rng.choice(n, size=n // 200, replace=False):  # IUPAC in the reference
        ref[p] = rng.choice(list(IUPAC))
    ref = "".join(ref)
    recs = _records(rng, ref, lq, window)
    assert recs[-1][2] + 2 * lq + window < n
    q = "I" * lq
    lines = ["\t".join(["r%d" % i, str(flag), "c1", str(pos + 1), "60", cig, "*", "0", "0", seq, q])
             for i, (cig, seq, pos, flag) in enumerate(recs)]
    text = "@SQ\tSN:c1\tLN:%d\n" % n + "\n".join(lines) + "\n"
    names, lens, batch, qnames = samutil.sam_to_batch(text)
    return names, [ref], batch


@pytest.mark.parametrize("rules", [DEFAULT, DEFAULT & ~EQ_BY_CHAR, DEFAULT & ~N_EQ_N], ids=["default", "eq_by_sign", "n_mismatches_n"])
@pytest.mark.parametrize("lq", [150, 158], ids=["eight_lane", "sixteen_lane"])
def test_walk_against_oracle_and_traced_path(oracle, monkeypatch, capfd, lq, rules):
    import os
    rng = np.random.default_rng(lq * 31 + rules)
    window = 200
    names, seqs, batch = _batch(rng, lq, window)
    os.environ["FADEHIP_DEBUG"] = "1"
    try:
        c = fade_amd.Context(device=0, rules=rules)
    finally:
        del os.environ["FADEHIP_DEBUG"]
    try:
        c.genome_upload(names, [s.encode() for s in seqs])
        rs0, aln0, st0 = c.annotate(batch, 5, window)
        monkeypatch.setenv("FADEHIP_NO_SHORTCUT", "1")
        rs1, aln1, st1 = c.annotate(batch, 5, window)
        monkeypatch.delenv("FADEHIP_NO_SHORTCUT")
    finally:
        c.close()
    err = capfd.readouterr().err
    assert ("eight-lane groups" in err) == (lq == 150), err[-300:]
    assert np.array_equal(rs0, rs1) and list(st0) == list(st1)
    assert aln0[np.argsort(aln0["read_idx"], kind="stable")].tobytes() == aln1[np.argsort(aln1["read_idx"], kind="stable")].tobytes()
    tags = format_tags(batch, names, rs0, aln0)
    G = oracle.GenomeHolder(names, seqs)
    ors, oam = oracle.annotate_batch_soa(G, batch, 5, window, threads=8, params=oracle.default_params(rules=rules))
    assert np.array_equal(rs0, ors), np.nonzero(rs0 != ors)[0][:10]
    n_art = 0
    for i in range(len(ors)):
        if oam[i] is None:
            assert i not in tags
        else:
            assert tags[i]["am"] == oam[i], i
            n_art += 1
    assert n_art > 200
