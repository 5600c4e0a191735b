"""The rule switches (fadehip_params.rules) and other scoring on the long-list kernels and on windows of more than one staged
chunk: tests/test_gpu_rules.py holds each switch to the oracle on reads of up to 260 bases and windows of up to 900 columns,
where sw_pk_kernel serves everything.  Here the same comparison (exact, with the oracle under the same setting) runs where
sw_forward64_kernel (one alignment per wavefront, 12 .. 64 rows per lane) and sw_long_kernel (a thread per alignment) serve,
at both ends of every rows-per-lane class, at the 65,000 / 65,001-column hand-over between the two, and across the 2,048-column
chunks that sw_pk_kernel stages.  The inputs plant the ties that the switches decide (long_rule_lists.py;
test_long_rule_inputs.py holds them to that on the CPU), and every case checks, from the library's FADEHIP_DEBUG line, that
the runner it was written for served it: sw_forward64_kernel writes its trace flags for the default Appendix A.3 / A.4 rules
alone, so run_long sends a list there only when END_MIN_REF_THEN_QUERY, GAP_TIE_EXTENDS and HDIR_DIAG_F_E are all set."""
import re

import numpy as np
import pytest

import fade_amd
from fade_amd import format_tags
from helpers import concat
import long_rule_lists as LL
from long_rule_lists import ALL_SETTINGS, DEFAULT, END_MIN_REF, FADE, HDIR_F_E, TIE_EXTENDS

pytestmark = pytest.mark.gpu

WAVE_RULES = END_MIN_REF | HDIR_F_E | TIE_EXTENDS
LINE = re.compile(r"\[fadehip\] long list of (\d+) alignments \(longest read (\d+), widest window (\d+)\): (wave64 R=(\d+)|thread)\n")
IDS = [s[0] for s in ALL_SETTINGS]


def _context(monkeypatch, **kw):
    monkeypatch.setenv("FADEHIP_DEBUG", "1")
    monkeypatch.delenv("FADEHIP_LONG_THREAD", raising=False)
    return fade_amd.Context(device=0, **kw)


def _runner(rows, rules):
    """the runner's name in the debug line: `rows` per lane on the wave kernel where the rules allow it, else the thread kernel"""
    return "wave64 R=%d" % rows if rows is not None and rules & WAVE_RULES == WAVE_RULES else "thread"


def _level1(oracle, monkeypatch, capfd, tag, qs, rs, scoring, rules, rows):
    """One sw_batch_packed call under (scoring, rules) against the oracle under the same; then the runner of its long list."""
    exp = LL.expected(oracle, tag, qs, rs, scoring, rules)
    qc, qo = concat(qs)
    rc, ro = concat(rs)
    capfd.readouterr()
    c = _context(monkeypatch, open=scoring[0], ext=scoring[1], match=scoring[2], mismatch=scoring[3], rules=rules)
    try:
        got = c.sw_batch_packed(qc, qo, rc, ro)
    finally:
        c.close()
    err = capfd.readouterr().err
    for k in range(len(qs)):
        g = tuple(int(got[k][f]) for f in ("score", "end_query", "end_ref", "beg_query", "beg_ref", "n_ops"))
        assert g == exp[k][:6], (tag, k, len(qs[k]), len(rs[k]), g, exp[k])
        assert tuple(int(x) for x in got[k]["ops"][:len(exp[k][6])]) == exp[k][6], (tag, k, len(qs[k]), len(rs[k]))
    long_ones = [k for k in range(len(qs)) if len(qs[k]) > 512 or len(rs[k]) > 32000]
    lines = LINE.findall(err)
    if not long_ones:
        assert lines == [], lines
    else:
        assert len(lines) == 1, err[-600:]
        n, max_lq, max_lr, runner, _ = lines[0]
        assert (int(n), int(max_lq), int(max_lr)) == (len(long_ones), max(len(qs[k]) for k in long_ones), max(len(rs[k]) for k in long_ones))
        assert runner == _runner(rows, rules), (tag, hex(rules), lines[0])
    return exp


@pytest.mark.parametrize("name,rules", ALL_SETTINGS, ids=IDS)
@pytest.mark.parametrize("lst", LL.LISTS)
def test_level1_under_rule(oracle, monkeypatch, capfd, lst, name, rules):
    qs, rs = LL.pairs(oracle, lst)
    _level1(oracle, monkeypatch, capfd, lst, qs, rs, FADE, rules, LL.RUNNER[lst])


@pytest.mark.parametrize("name,rules", [s for s in ALL_SETTINGS if s[0] in LL.A3_A4], ids=list(LL.A3_A4))
@pytest.mark.parametrize("scoring", LL.RULE_SCORINGS, ids=str)
@pytest.mark.parametrize("lst", ["short", "r12"])
def test_level1_other_scoring_under_rule(oracle, monkeypatch, capfd, lst, scoring, name, rules):
    qs, rs = LL.short_pairs(oracle, scoring) if lst == "short" else LL.pairs(oracle, lst, scoring)
    _level1(oracle, monkeypatch, capfd, lst, qs, rs, scoring, rules, 12)


@pytest.mark.parametrize("scoring", LL.LONG_SCORINGS, ids=str)
@pytest.mark.parametrize("lst", ["r12", "r64", "thread"])
def test_level1_other_scoring_on_the_long_list(oracle, monkeypatch, capfd, lst, scoring):
    """Default rules; the list also holds an exact match of its longest read: match * lq is the largest score the list's kernel
    has to hold (14 * 4,096 = 57,344 fills the 16 score bits of sw_forward64_kernel's end-cell key)."""
    qs, rs = LL.pairs(oracle, lst)
    lq = max(LL.READ_LISTS[lst])
    q, r = LL.full_length_match(lq)
    exp = _level1(oracle, monkeypatch, capfd, lst + "+full", qs + [q], rs + [r], scoring, DEFAULT, LL.RUNNER[lst])
    assert exp[-1][0] == scoring[2] * lq  # (and the device gave the same: _level1 compared it)


@pytest.mark.parametrize("name,rules", ALL_SETTINGS, ids=IDS)
@pytest.mark.parametrize("batch", list(LL.LEVEL2))
def test_level2_under_rule(oracle, monkeypatch, capfd, batch, name, rules):
    names, seqs, b = LL.level2_batch(batch)
    cfg = LL.LEVEL2[batch]
    ors, oam = LL.level2_expected(oracle, batch, rules)
    capfd.readouterr()
    c = _context(monkeypatch, rules=rules)
    try:
        c.genome_upload(names, [s.encode() for s in seqs])
        rs, aln, stats = c.annotate(b, LL.FLOOR_LEN, cfg["window"])
        prof = c.last_profile(0)
    finally:
        c.close()
    err = capfd.readouterr().err
    tags = format_tags(b, names, rs, aln)
    assert np.array_equal(rs, ors), (batch, name, np.nonzero(rs != ors)[0][:10])
    for i in range(len(ors)):
        assert (tags[i]["am"] if i in tags else None) == oam[i], (batch, name, i, tags.get(i), oam[i])
    # one runner serves the long list in one launch: its trace bytes are (alignments) x (what run_long_wave / run_long
    # reserve for one), from the figures of the debug line
    lines = LINE.findall(err)
    assert len(lines) == 1, err[-600:]
    n, max_lq, max_lr, runner, rows = lines[0]
    n, max_lq, max_lr = int(n), int(max_lq), int(max_lr)
    assert runner == _runner(cfg["runner"], rules), (batch, name, lines[0])
    assert max_lq == cfg["read_len"] and (max_lq > 512 or max_lr > 32000) and 0 < prof["alignments"] <= n
    if runner == "thread":
        item = max_lq * ((max_lr + 1) // 2)
    else:
        item = ((max_lr + 63 + 3) // 4) * (int(rows) // 2) * 64 * 4
    if cfg.get("also_short"):  # the 16-lane kernels add the trace of the windows they served
        assert prof["trace_bytes"] > n * item, (batch, name, prof["trace_bytes"], n, item)
    else:
        assert prof["trace_bytes"] == n * item, (batch, name, prof["trace_bytes"], n, item)
