"""tests/mates_model.py, the rule by which mate fields follow the hard clip, held to numbers typed in by hand and to its
own invariants.  No GPU."""
import clip_cases as cc
import mates_cases as mc
import mates_model as mm
import tags_model as tm


def _fix_all(records, rs, tl, tr):
    return mm.fix_batch(mm.insert({}, records, rs, tl, tr), records, rs, tl, tr)


def test_the_worked_example():
    """R1 99 at 100 50M, R2 147 at 300 50M: before any clip tlen is 250 / -250; R1 loses ten reference bases on the left."""
    r1 = cc.build_rec("pair", 0, 100, 30, 99, -1, -1, 0, "50M", "A" * 50, "I" * 50)
    r2 = cc.build_rec("pair", 0, 300, 30, 147, -1, -1, 0, "50M", "C" * 50, "I" * 50, b"MCZ50M\0")
    before, fixed, _ = _fix_all([r1, r2], [0, 0], [0, 0], [0, 0])
    assert fixed == [1, 1]
    d1, d2 = cc.decode_rec(before[0]), cc.decode_rec(before[1])
    assert (d1["mtid"], d1["mpos"], d1["tlen"], d1["flag"]) == (0, 300, 250, 99)
    assert (d2["mtid"], d2["mpos"], d2["tlen"], d2["flag"], d2["aux"]) == (0, 100, -250, 147, b"MCZ50M\0")
    after, fixed, classes = _fix_all(before, [3, 0], [10, 0], [0, 0])
    assert fixed == [1, 1]
    d1, d2 = cc.decode_rec(after[0]), cc.decode_rec(after[1])
    assert (d1["pos"], d1["cigar"], d1["mpos"], d1["tlen"], d1["flag"]) == (110, "10H40M", 300, 240, 99)
    assert (d2["pos"], d2["cigar"], d2["mpos"], d2["tlen"], d2["flag"], d2["aux"]) == (300, "50M", 110, -240, 147, b"MCZ10H40M\0")
    assert classes["mc_replaced"] == 1 and classes["fixed"] == 2


def test_a_reset_mate_by_hand():
    r1 = cc.build_rec("pair", 0, 100, 30, 99, 0, 300, 250, "50M", "A" * 50, "I" * 50)
    r2 = cc.build_rec("pair", 0, 300, 30, 147, 0, 100, -250, "50M", "C" * 50, "I" * 50, b"NMC\x01MCZ50M\0")
    after, fixed, classes = _fix_all([r1, r2], [2, 0], [50, 0], [0, 0])
    assert fixed == [0, 1] and classes["reset_mate"] == 1 and classes["mc_removed"] == 1
    d1, d2 = cc.decode_rec(after[0]), cc.decode_rec(after[1])
    assert (d1["flag"], d1["tid"], d1["pos"], d1["cigar"], d1["aux"]) == (0, 0, 0, "*", b"")
    assert (d2["flag"], d2["mtid"], d2["mpos"], d2["tlen"], d2["aux"]) == ((147 | 8) & ~0x22, 0, 300, 0, b"NMC\x01")


def test_pair_up_is_a_fixed_point_of_the_rule_without_clips():
    sets = [tm.annotated(tag)[2] for tag in ("anno_c1", "anno_c2", "anno_c5", "anno_floor0")] + [mc.flat()[0]]
    n_fixed = 0
    for records in sets:
        paired = mm.pair_up(records, mc=lambda rec: rec[36] % 2 == 0)
        zero = [0] * len(paired)
        out, fixed, _ = _fix_all(paired, zero, zero, zero)
        assert out == paired
        n_fixed += fixed.count(1)
    assert n_fixed > 100


def test_the_tlens_of_a_fixed_pair_are_negatives_of_each_other_unless_d_is_zero():
    records, rs, tl, tr = mc.flat()
    out, fixed, _ = _fix_all(records, rs, tl, tr)
    by_key = {}
    for rec, f in zip(out, fixed):
        if f == 1 and not mm.flag_of(rec) & 0x900:
            by_key[mm.key(rec)] = cc.decode_rec(rec)
    pairs = zero = 0
    for (ln, name, seg), d in by_key.items():
        other = by_key.get((ln, name, seg ^ 0xC0))
        if other is None or seg != 0x40:
            continue
        pairs += 1
        if d["tlen"] == 1 and other["tlen"] == 1:  # d == 0: both 5' ends at one base
            zero += 1
        else:
            assert d["tlen"] == -other["tlen"], (name, d["tlen"], other["tlen"])
    assert pairs >= 20 and zero == 1


def test_the_case_list_reaches_every_class():
    records, rs, tl, tr = mc.flat()
    _, _, classes = _fix_all(records, rs, tl, tr)
    assert all(classes[c] >= 1 for c in mm.CLASSES), classes
