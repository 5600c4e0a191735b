"""Conditions on the INPUTS of tests/test_gpu_rules_long.py, checked with the oracle alone (no device): a list in which a rule
switch decides nothing would let the GPU test of that switch pass whatever the kernels do.  For every list and every
single-switch setting, at least two pairs of the list give another result than under the default rules; the Appendix A.4
settings also have at least four pairs with an I or a D among the first 16 ops (the switch acts on gaps); the level-2 batches
give the gapped am tags they were made for.  Where a condition fails the list has to grow: the shapes stay."""
import pytest

import long_rule_lists as LL

SINGLE = LL.SETTINGS[:7]  # (the eighth flips five switches at once)


def _exercised(oracle, lst, qs, rs, scoring, settings):
    dflt = LL.expected(oracle, lst, qs, rs, scoring, LL.DEFAULT)
    for name, rules in settings:
        exp = LL.expected(oracle, lst, qs, rs, scoring, rules)
        differ = sum(a != b for a, b in zip(dflt, exp))
        gaps = sum(LL.gapped(x) for x in exp)
        print("%-18s %-16s %-36s %3d pairs, %3d differ from the default rules, %3d gapped" % (lst, scoring, name, len(qs), differ, gaps))
        assert differ >= 2, (lst, scoring, name, differ)
        if name in LL.A4_NAMES:
            assert gaps >= 4, (lst, scoring, name, gaps)


@pytest.mark.parametrize("lst", LL.LISTS)
def test_every_switch_decides_something_in_the_list(oracle, lst):
    qs, rs = LL.pairs(oracle, lst)
    lqs = sorted(set(len(q) for q in qs))
    if lst in LL.READ_LISTS:  # the list holds both ends of its class, and nothing longer: its longest read picks the kernel
        # (an end-cell tie needs an even length: at an odd one it has a base less)
        ends = LL.READ_LISTS[lst]
        assert set(ends) <= set(lqs) and max(lqs) == max(ends) and set(lqs) - set(lq - lq % 2 for lq in ends) - set(ends) <= set(range(513)), lqs
        assert all(len(q) + 60 <= len(r) <= len(q) + 300 for q, r in zip(qs, rs) if len(q) > 512)
    _exercised(oracle, lst, qs, rs, LL.FADE, SINGLE)


@pytest.mark.parametrize("scoring", LL.RULE_SCORINGS, ids=str)
@pytest.mark.parametrize("lst", ["short", "r12"])
def test_the_switches_decide_something_under_other_scoring(oracle, lst, scoring):
    qs, rs = LL.short_pairs(oracle, scoring) if lst == "short" else LL.pairs(oracle, lst, scoring)
    _exercised(oracle, lst, qs, rs, scoring, [s for s in SINGLE if s[0] in LL.A3_A4])


@pytest.mark.parametrize("name", list(LL.LEVEL2))
def test_level2_batches_give_gapped_tags(oracle, name):
    for sname, rules in LL.ALL_SETTINGS:
        rs, am = LL.level2_expected(oracle, name, rules)
        n = LL.gapped_am(am)
        print("%-18s %-36s %3d am tags, %3d gapped" % (name, sname, sum(a is not None for a in am), n))
        if rules & LL.PAD_S:
            assert n >= LL.LEVEL2[name]["gapped"], (name, sname, n)
        else:  # no S ops in the result: analysis.d:78-80 / 102-104 call nothing an artifact, there is no am tag at all
            assert all(a is None for a in am)
