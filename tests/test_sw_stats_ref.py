"""The stats-mode restatement (tests/sw_stats_ref.c) against the scalar oracle and against hand-worked answers (CPU)."""
import numpy as np

import sw_stats_ref as S
from helpers import make_pairs

KINDS = ("random", "planted", "homopolymer", "tandem", "nrich", "iupac", "related", "lowcomplexity", "refspecial")

SC = S.SCORING_STATS  # (open 3, ext 8, match 10, mismatch -5): stats.d:87


def _oracle_params(oracle, rules=S.RULES_DEFAULT):
    p = oracle.default_params(rules)
    p.open, p.ext, p.match, p.mismatch = SC
    return p


def _check_against_oracle(oracle, qs, rs, rules=S.RULES_DEFAULT):
    got = S.stats_batch(qs, rs, SC, rules)
    p = _oracle_params(oracle, rules)
    bad = []
    for k, (q, r) in enumerate(zip(qs, rs)):
        e = oracle.sw(q if isinstance(q, str) else bytes(q), r if isinstance(r, str) else bytes(r), p)
        g = got[k]
        if (int(g["score"]), int(g["end_query"]), int(g["end_ref"])) != (e["score"], e["end_query"], e["end_ref"]):
            bad.append((k, tuple(int(x) for x in g), (e["score"], e["end_query"], e["end_ref"])))
        # the statistics of any path are bounded by its cells
        assert 0 <= g["matches"] <= g["length"] and 0 <= g["similar"] <= g["length"]
        assert g["length"] <= len(q) + len(r)
        if g["score"] > 0:
            assert g["similar"] >= 1 and g["length"] >= 1
    assert not bad, "%d/%d differ from oracle.sw, first: %r" % (len(bad), len(qs), bad[:3])


def test_score_and_end_cell_match_oracle_on_families(oracle):
    rng = np.random.default_rng(20261016)
    qs, rs = make_pairs(rng, 360, lq_range=(1, 120), lr_range=(1, 160), kinds=KINDS)
    _check_against_oracle(oracle, qs, rs)


def test_score_and_end_cell_match_oracle_under_other_rules(oracle):
    rng = np.random.default_rng(7)
    qs, rs = make_pairs(rng, 126, lq_range=(1, 60), lr_range=(1, 80), kinds=KINDS)
    for rules in (0, 0x7f & ~0x1, 0x7f & ~0x2, 0x7f & ~0x4, 0x7f & ~0x40):
        _check_against_oracle(oracle, qs, rs, rules)


def test_ext_above_open_decides_the_path(oracle):
    # one long gap: open 3 then 8 a base, against the ungapped halves
    rng = np.random.default_rng(3)
    qs, rs = [], []
    for gap in (1, 2, 3, 4, 6):
        a = rng.integers(0, 4, 12)
        b = rng.integers(0, 4, 12)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        q = np.concatenate([acgt[a], acgt[b]])
        r = np.concatenate([acgt[a], acgt[rng.integers(0, 4, gap)], acgt[b]])
        qs += [q, r]
        rs += [r, q]
    _check_against_oracle(oracle, qs, rs)
    got = S.stats_batch(qs, rs, SC)
    # a 1-base gap is worth taking (12 x 10 on both sides, -3), so the path spans both halves and the gap
    assert got[0]["length"] == 25 and got[0]["matches"] == 24


def test_zero_score_pairs(oracle):
    qs = ["A", "AAAA", "ACAC", "N", "RYK"]
    rs = ["C", "CCCCCC", "GTGT", "A", "RYK"]
    _check_against_oracle(oracle, qs, rs)
    for g in S.stats_batch(qs, rs, SC):
        assert tuple(int(x) for x in g) == (0, 0, 0, 0, 0, 0)


def test_hand_worked_answers():
    cases = [
        # (q, r) -> score, end_query, end_ref, matches, similar, length
        ("ACGT", "ACGT", (40, 3, 3, 4, 4, 4)),
        ("ACGTA", "ACCTA", (35, 4, 4, 4, 4, 5)),       # one mismatch inside: 4 x 10 - 5
        ("AAAA", "AATAA", (37, 3, 4, 4, 4, 5)),        # one ref-only gap base: 4 x 10 - 3
        ("ACGTAC", "ACGTTTAC", (54, 5, 7, 6, 6, 8)),   # a gap of two: 6 x 10 - 3 - 3 (ext > open: the gap re-opens)
        ("ARA", "ARA", (20, 2, 2, 3, 2, 3)),           # R vs R scores 0 (wildcard) but is an equal residue
        ("ANA", "ANA", (30, 2, 2, 3, 3, 3)),           # N vs N scores match (A.1, FADEHIP_RULE_N_MATCHES_N)
        ("acgt", "ACGT", (40, 3, 3, 0, 4, 4)),         # case-insensitive scores, residue equality by byte
        ("", "ACGT", (0, 0, 0, 0, 0, 0)),
        ("ACGT", "", (0, 0, 0, 0, 0, 0)),
    ]
    for q, r, want in cases:
        g = S.stats(q, r, SC)
        assert tuple(g[k] for k in S.DTYPE.names) == want, (q, r, g)
    # with equality by the sign of the matrix entry, R vs R is not a match and a vs A is
    assert S.stats("ARA", "ARA", SC, rules=0x7f & ~0x8)["matches"] == 2
    assert S.stats("acgt", "ACGT", SC, rules=0x7f & ~0x8)["matches"] == 4
