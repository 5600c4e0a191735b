"""tests/clip_sweep.py holds what it is for — asserted from oracle/pyfilter.clip_read's answers alone, without a GPU, before
any device or host path is held to the sweep (tests/test_gpu_clip_sweep.py, tests/test_cli_clip.py)."""
import collections

import clip_cases as cc
import clip_sweep as sw
from oracle import pyfilter


def _clipped(family):
    """(case, pyfilter's record) of the records the clip changes without resetting them."""
    return [(c, new) for c, (new, _) in zip(sw.cases(family), sw.expected(family)) if c["rs"] & 6 and not sw.is_reset(c, new)]


def test_the_cases_have_the_shape_of_clip_cases_and_the_families_their_sizes():
    n = {f: len(sw.cases(f)) for f in sw.FAMILIES}
    print("records per family:", n)
    assert 5000 <= n["writer"] <= 9000 and 300 <= n["bins"] <= 1000 and n["random"] == 20000
    for f in sw.FAMILIES:
        cs = sw.cases(f)
        assert len({c["name"] for c in cs}) == len(cs)
        assert all(set(c) == {"name", "rec", "aux", "rs", "tl", "tr"} for c in cs)
        assert sw.cases(f) == cs  # fixed seeds
        assert all(len(c["rec"]["seq"]) == len(c["rec"]["qual"]) for c in cs)
        assert not any(n == 0 for c in cs for n, _ in cc.cigar_ops(c["rec"]["cigar"]))
        assert all(len(c["aux"]) < 1000 for c in sw.cases(f, sam_only=True))
    a = sw.cases("writer")
    assert {len(c["rec"]["qname"]) + 1 for c in a} == {2, 3, 4, 5}
    assert {len(c["rec"]["seq"]) for c in a} == set(sw.A_LQ)
    assert set("".join(c["rec"]["seq"] for c in a[:200])) == set(cc.NT16)
    big = sum(1 for c in a if len(c["aux"]) > 3000)
    assert len(a) // 60 <= big <= len(a) // 40 and any(not c["aux"] for c in a) and any(0 < len(c["aux"]) < 100 for c in a)
    assert {c["rs"] for c in a} == {2, 4, 6}


def test_the_writer_family_reaches_every_shift_tail_and_trip_count():
    """(parity of the first surviving base) x (packed bytes mod 4) x (odd or even rest), each with the surviving bytes all
    in the byte tail (nb <= 3), in a lane's first trip of the dword loop (4..64) and beyond it (> 64).  No nb <= 3 is a
    multiple of four: those eight cells do not exist."""
    seen = collections.Counter()
    for c, new in _clipped("writer"):
        ops = cc.cigar_ops(new["cigar"])
        sb = ops[0][0] if c["rs"] & 2 else 0
        assert sb == c["tl"] * bool(c["rs"] & 2) and len(new["seq"]) == len(c["rec"]["seq"]) - sb - c["tr"] * bool(c["rs"] & 4)
        lseq = len(new["seq"])
        nb = (lseq + 1) // 2
        seen[(sb % 2, nb % 4, lseq % 2, 0 if nb <= 3 else 1 if nb <= 64 else 2)] += 1
    want = [(p, m, r, size) for p in (0, 1) for m in range(4) for r in (0, 1) for size in (0, 1, 2) if not (size == 0 and m == 0)]
    print("writer cells: %d, fewest records in one: %d" % (len(want), min(seen[w] for w in want)))
    assert all(seen[w] > 0 for w in want), [w for w in want if not seen[w]]
    assert set(seen) == set(want)


def test_the_bin_family_reaches_every_outcome_of_reg2bin():
    """Every one of reg2bin's six outcomes among the clipped records, and records that fall to a finer level.  A record that
    moves to a COARSER level does not exist: a hard clip takes reference bases off the ends of the span and adds none (an
    unmapped record's pos -1 counts as 0 before and after), so the clipped span lies inside the incoming one and every bin
    that holds the one holds the other.  That is asserted in its place."""
    out_levels, finer, coarser, crossed, on_line = collections.Counter(), 0, 0, 0, 0
    for c, new in _clipped("bins"):
        before, after = sw.level(c["rec"]["pos"], c["rec"]["cigar"]), sw.level(new["pos"], new["cigar"])
        out_levels[after] += 1
        rank = lambda lv: 99 if lv == 0 else lv
        finer += rank(after) < rank(before)
        coarser += rank(after) > rank(before)
        ref = sum(n for n, x in cc.cigar_ops(new["cigar"]) if x in cc._RC)
        for s in sw.B_SHIFTS:
            crossed += c["rec"]["pos"] >> s != new["pos"] >> s and new["pos"] >= 0 and c["rec"]["pos"] >= 0
            on_line += (new["pos"] + ref) % (1 << s) == 0
    print("bin family: clipped records per outgoing level", dict(out_levels), "finer", finer, "coarser", coarser)
    assert set(out_levels) == {14, 17, 20, 23, 26, 0} and min(out_levels.values()) >= 3
    assert finer >= 20 and coarser == 0 and crossed >= 12 and on_line >= 12
    b = sw.cases("bins")
    assert max(n for c in b for n, x in cc.cigar_ops(c["rec"]["cigar"]) if x == "N") == 1 << 27
    assert sum(1 for c in b if c["rec"]["pos"] >= 1 << 29) >= 20
    # from 2^29 on a fine bin's number is past the five levels' ranges, from 997 Mb on past 16 bits
    assert any(cc.reg2bin(new["pos"], new["pos"] + 1) > 37449 for _, new in _clipped("bins"))
    assert any(cc.reg2bin(new["pos"], new["pos"] + 1) > 65535 for _, new in _clipped("bins"))
    un = [(c, new) for c, (new, _) in zip(b, sw.expected("bins")) if c["rec"]["rname"] == "*"]
    assert all(c["rec"]["pos"] == -1 and c["rec"]["flag"] == 4 and c["rec"]["cigar"] != "*" for c, _ in un)
    assert {new["pos"] for c, new in un if c["rs"] == 2 and not sw.is_reset(c, new)} == {-1, 0, 4, 18}
    assert any(c["rs"] == 4 and new["pos"] == -1 and new["cigar"].endswith("3H") for c, new in un)
    keys = [(cc.CONTIGS.index(c["rec"]["rname"]) if c["rec"]["rname"] != "*" else 1 << 32, c["rec"]["pos"]) for c in b]
    assert keys != sorted(keys)  # (the order the family comes in is not coordinate order: --keep-sorted's test sorts it)


def _walk_ends(rec):
    """Of a both-sides call, by the oracle's one-sided answers: (index of the op the left walk stops in, partly eaten?,
    index of the op the right walk stops in, partly eaten?), the right walk alone."""
    ops = cc.cigar_ops(rec["cigar"])
    left = cc.cigar_ops(pyfilter.clip_read(rec, 2, cc.CONTIGS[0])["cigar"])[1:]
    right = cc.cigar_ops(pyfilter.clip_read(rec, 4, cc.CONTIGS[0])["cigar"])[:-1]
    il, ir = len(ops) - len(left), len(right) - 1
    return il, left[0][0] < ops[il][0], ir, right[-1][0] < ops[ir][0]


def test_the_random_family_holds_the_meetings_the_resets_and_the_short_sequences():
    cs, exp = sw.cases("random"), sw.expected("random")
    n = collections.Counter()
    for c, (new, _) in zip(cs, exp):
        rec, rs = c["rec"], c["rs"]
        ops = cc.cigar_ops(rec["cigar"])
        claimed = sum(x for x, o in ops if o in cc._QC)
        n["rs%d" % rs] += 1
        n["short"] += len(rec["seq"]) < claimed
        assert 0 <= claimed - len(rec["seq"]) <= 3 and 1 <= len(ops) <= 8 and all(1 <= x <= 12 for x, _ in ops)
        if not rs & 6:
            assert new == rec
            continue
        if sw.is_reset(c, new):
            n["reset"] += 1
            left_resets = bool(rs & 2) and pyfilter.clip_read(rec, 2, cc.CONTIGS[0])["tags"] == {}
            n["reset_left" if left_resets else "reset_right_alone" if rs == 4 else "reset_right_after_left"] += 1
            continue
        out = cc.cigar_ops(new["cigar"])
        hard = (out[0][0] if rs & 2 else 0) + (out[-1][0] if rs & 4 else 0)
        gone = len(rec["seq"]) - len(new["seq"])
        assert gone <= hard
        if len(rec["seq"]) < claimed and gone < hard:  # the H ops say more bases than there were to take
            n["short_reached"] += 1
        if rs == 6:
            il, pl, ir, pr = _walk_ends(rec)
            if il == ir and pl and pr:
                n["meet_in_one_op"] += 1
                n["meet_in_" + ops[il][1]] += 1
            if il == ir and pl and ops[il][1] != "M":  # the right walk works on what the left one left of an op that is no M
                n["right_reaches_a_partly_eaten_" + ops[il][1]] += 1
            if ir > il and any(o in "IPS" for _, o in ops[il + 1:ir]):
                n["I_P_or_S_between_the_ends"] += 1
    print("random family:", dict(sorted(n.items())))
    assert n["meet_in_one_op"] >= 200 and n["meet_in_D"] >= 20 and n["meet_in_N"] >= 20
    assert min(n["reset_left"], n["reset_right_alone"], n["reset_right_after_left"]) >= 500
    assert n["reset"] <= 0.4 * len(cs)
    assert n["short_reached"] >= 300
    assert 1600 <= n["short"] <= 2400 and n["rs0"] > 0 and n["rs1"] > 0 and n["rs0"] + n["rs1"] < 0.05 * len(cs)
    assert n["I_P_or_S_between_the_ends"] >= 200
    assert all(n["right_reaches_a_partly_eaten_" + o] >= 5 for o in "DN=X")
