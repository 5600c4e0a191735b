"""The mate map on the device (fadehip_mateset_* / fadehip_mates_fix_batch, bam_mates.hpp) against tests/mates_model.py, byte
for byte, on the hand-built records of tests/mates_cases.py.  Every case runs with the hash whole, cut to three bits and cut
to none (FADEHIP_MATESET_HASH_BITS), and from the default table and from sixteen slots (FADEHIP_MATESET_SLOTS): the answers
are the same."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import fade_amd
import mates_cases as mc
import mates_model as mm

pytestmark = pytest.mark.gpu

SWITCHES = [(bits, slots) for bits in ("64", "3", "0") for slots in (None, "16")]


@pytest.fixture(params=SWITCHES, ids=lambda p: "bits%s-slots%s" % (p[0], p[1] or "default"))
def make_set(request, ctx, monkeypatch):
    bits, slots = request.param
    monkeypatch.setenv("FADEHIP_MATESET_HASH_BITS", bits)
    if slots is None:
        monkeypatch.delenv("FADEHIP_MATESET_SLOTS", raising=False)
    else:
        monkeypatch.setenv("FADEHIP_MATESET_SLOTS", slots)
    made = []

    def make():
        made.append(ctx.mateset())
        return made[-1]

    yield make
    for s in made:
        s.close()


def _first_difference(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return k, g.hex(), w.hex()
    return None


def _run(s, model, records, rs, tl, tr, add=True):
    """One add call and one fix call on the device and in the model; returns the model's class counts."""
    if add:
        s.add_batch(records, rs, tl, tr)
        mm.insert(model, records, rs, tl, tr)
    assert s.count == mm.count(model)
    got, fixed = s.fix_batch(records, rs, tl, tr)
    want, want_fixed, classes = mm.fix_batch(model, records, rs, tl, tr)
    assert fixed.dtype == np.uint8 and fixed.tolist() == want_fixed
    assert len(got) == len(want) and _first_difference(got, want) is None
    return classes


def test_every_case_in_one_batch_and_every_class_reached(make_set):
    records, rs, tl, tr = mc.flat()
    classes = _run(make_set(), {}, records, rs, tl, tr)
    assert all(classes[c] >= 1 for c in mm.CLASSES), classes


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_each_case_alone(make_set, name):
    _run(make_set(), {}, *mc.flat([name]))


def test_the_worked_example_by_hand(make_set):
    import clip_cases as cc
    records, rs, tl, tr = mc.flat(["example_mate_behind"])
    s = make_set()
    s.add_batch(records, rs, tl, tr)
    got, fixed = s.fix_batch(records, rs, tl, tr)
    d1, d2 = cc.decode_rec(got[0]), cc.decode_rec(got[1])
    assert fixed.tolist() == [1, 1] and s.count == (2, 0)
    assert (d1["pos"], d1["cigar"], d1["mpos"], d1["tlen"], d1["flag"]) == (110, "10H40M", 300, 240, 99)
    assert (d2["pos"], d2["cigar"], d2["mpos"], d2["tlen"], d2["flag"], d2["aux"]) == (300, "50M", 110, -240, 147, b"MCZ10H40M\0")


def test_a_duplicated_key_is_ambiguous_whichever_insert_comes_first(make_set):
    records, rs, tl, tr = mc.flat(["duplicated_key", "example_mate_behind"])
    assert mm.key(records[0]) == mm.key(records[1])
    swap = [1, 0] + list(range(2, len(records)))
    outs = []
    for order in (list(range(len(records))), swap):
        s, model = make_set(), {}
        sel = lambda a: [a[k] for k in order]
        s.add_batch(sel(records), sel(rs), sel(tl), sel(tr))
        mm.insert(model, sel(records), sel(rs), sel(tl), sel(tr))
        assert s.count == mm.count(model) and s.count[1] == 1
        got, fixed = s.fix_batch(records, rs, tl, tr)
        want, want_fixed, _ = mm.fix_batch(model, records, rs, tl, tr)
        assert got == want and fixed.tolist() == want_fixed
        assert fixed.tolist()[:4] == [1, 1, 2, 2]  # (the two lines of the other segment: their mate's key is ambiguous)
        outs.append(got)
    assert outs[0] == outs[1]
    # the same key once more, in a later call: the entry stays ambiguous and is counted once
    s.add_batch(records[:1], rs[:1], tl[:1], tr[:1])
    assert s.count == mm.count(model)


def test_pick_and_the_lines_that_do_not_insert(make_set):
    records, rs, tl, tr = mc.flat(["secondary_and_supplementary", "unpaired_and_odd_segment_bits", "names"])
    pick = np.array([(3 * k) % 4 != 1 for k in range(len(records))], np.uint8) * 7  # (any non-zero byte picks)
    s, model = make_set(), {}
    s.add_batch(records, rs, tl, tr, pick=pick)
    mm.insert(model, records, rs, tl, tr, pick=pick)
    assert 0 < s.count[0] < len(records)
    _run(s, model, records, rs, tl, tr, add=False)
    s.add_batch(records, rs, tl, tr, pick=np.zeros(len(records), np.uint8))  # nothing picked: nothing changes
    _run(s, model, records, rs, tl, tr, add=False)


@pytest.mark.parametrize("n", [63, 64, 65, 256, 257])
def test_batch_sizes_with_the_fixed_record_in_the_first_and_the_last_lane(make_set, n):
    """The mates come in a call of their own; the batch that is fixed holds them at its two ends."""
    (a1, a2), (b1, b2) = mc.CASES["example_mate_behind"], mc.CASES["left_of_reverse"]
    s, model = make_set(), {}
    first = [a1, b1]
    cols = lambda rows: ([r["rec"] for r in rows], [r["rs"] for r in rows], [r["tl"] for r in rows], [r["tr"] for r in rows])
    s.add_batch(*cols(first))
    mm.insert(model, *cols(first))
    batch = [a2] + [mc.filler(k) for k in range(n - 2)] + [b2]
    got, fixed = s.fix_batch(*cols(batch))
    want, want_fixed, classes = mm.fix_batch(model, *cols(batch))
    assert got == want and fixed.tolist() == want_fixed
    assert want_fixed[0] == 1 and want_fixed[-1] == 1 and sum(want_fixed) == 2 and classes["mc_replaced"] == 2


@functools.lru_cache(maxsize=None)
def _growth():
    """2,000 fragments in three add calls, and what the model makes of them: computed once for every table geometry."""
    model, at, calls, counts = {}, 0, [], []
    seen = ([], [], [], [])
    for n in (30, 400, 1570):
        rows = []
        for k in range(at, at + n):
            rows.append(mc.R("grow%05d" % k, 99, 0, 100 + k, "50M", mc.MC50, rs=2, tl=1 + k % 40))
            rows.append(mc.R("grow%05d" % k, 147, 0, 300 + k, "20M1D30M", mc.MC50, rs=4 * (k % 2), tr=1 + k % 30))
        at += n
        cols = ([r["rec"] for r in rows], [r["rs"] for r in rows], [r["tl"] for r in rows], [r["tr"] for r in rows])
        mm.insert(model, *cols)
        calls.append(cols)
        counts.append(mm.count(model))
        for a, b in zip(seen, cols):
            a += b
    want, want_fixed, _ = mm.fix_batch(model, *seen)
    return calls, counts, seen, want, want_fixed


def test_growth_from_sixteen_slots_and_a_moved_arena(make_set):
    """The table is hashed again several times from sixteen slots, the arena (64 KiB at first) moves; every mate is found
    afterwards."""
    calls, counts, seen, want, want_fixed = _growth()
    s = make_set()
    for cols, cnt in zip(calls, counts):
        s.add_batch(*cols)
        assert s.count == cnt
    got, fixed = s.fix_batch(*seen)
    assert fixed.tolist() == want_fixed == [1] * 4000 and _first_difference(got, want) is None


def test_out_cap_one_byte_short_is_refused_and_nothing_is_written(make_set, ctx):
    records, rs, tl, tr = mc.flat(["example_mate_behind", "mc_grows_and_shrinks"])
    s = make_set()
    s.add_batch(records, rs, tl, tr)
    got, _ = s.fix_batch(records, rs, tl, tr)
    need = sum(len(g) for g in got)
    cat, off, rs_a, tl_a, tr_a = s._arrays(records, rs, tl, tr)
    n = len(records)
    out = np.full(need, 0xAA, np.uint8)
    out_off = np.full(n + 1, -7, np.int64)
    fixed = np.full(n, 0xAA, np.uint8)
    args = (s._h, n, cat.ctypes.data, off.ctypes.data, rs_a.ctypes.data, tl_a.ctypes.data, tr_a.ctypes.data, out.ctypes.data)
    assert ctx._L.fadehip_mates_fix_batch(*args, need - 1, out_off.ctypes.data, fixed.ctypes.data) == -1
    assert ("%d bytes" % need) in ctx._L.fadehip_last_error(ctx._h).decode()
    assert (out == 0xAA).all() and (out_off == -7).all() and (fixed == 0xAA).all()
    assert ctx._L.fadehip_mates_fix_batch(*args, need, out_off.ctypes.data, fixed.ctypes.data) == 0
    assert out.tobytes() == b"".join(got) and out_off[n] == need
    with pytest.raises(fade_amd.FadeHipError):
        s.fix_batch(records, rs, tl, tr, out_cap=need - 1)
    assert s.fix_batch(records, rs, tl, tr, out_cap=need)[0] == got


def test_a_malformed_record_fails_with_its_index_and_leaves_the_set_as_it_was(make_set):
    records, rs, tl, tr = mc.flat(["example_mate_behind", "reset_mate"])
    s, model = make_set(), {}
    classes = _run(s, model, records, rs, tl, tr)
    assert classes["fixed"] >= 3
    more, rs2, tl2, tr2 = mc.flat(["names"])
    bad = bytearray(more[5])
    struct.pack_into("<i", bad, 20, 10 ** 6)  # l_seq beyond the record
    more[5] = bytes(bad)
    for call in (s.add_batch, s.fix_batch):
        with pytest.raises(fade_amd.FadeHipError) as e:
            call(more, rs2, tl2, tr2)
        assert e.value.code == -1 and "record 5" in str(e.value), str(e.value)
    with pytest.raises(fade_amd.FadeHipError) as e:
        s.add_batch(records, rs, [-1] + tl[1:], tr)
    assert e.value.code == -1 and "record 0" in str(e.value)
    _run(s, model, records, rs, tl, tr, add=False)


def test_null_arguments_are_refused(make_set, ctx):
    s = make_set()
    L = ctx._L
    off = (C.c_int64 * 2)(0, 40)
    buf = (C.c_uint8 * 48)()
    i32 = (C.c_int32 * 1)(0)
    n64 = C.c_int64(0)
    assert L.fadehip_mateset_create(ctx._h, None) == -1
    assert L.fadehip_mateset_create(None, C.byref(C.c_void_p())) == -1
    assert L.fadehip_mateset_add_batch(None, 1, buf, off, buf, i32, i32, None) == -1
    assert L.fadehip_mateset_add_batch(s._h, 1, None, off, buf, i32, i32, None) == -1
    assert L.fadehip_mateset_add_batch(s._h, 1, buf, None, buf, i32, i32, None) == -1
    assert L.fadehip_mateset_add_batch(s._h, 1, buf, off, None, i32, i32, None) == -1
    assert L.fadehip_mateset_add_batch(s._h, 1, buf, off, buf, None, i32, None) == -1
    assert L.fadehip_mates_fix_batch(None, 1, buf, off, buf, i32, i32, buf, 48, off, buf) == -1
    assert L.fadehip_mates_fix_batch(s._h, 1, buf, off, buf, i32, i32, None, 48, off, buf) == -1
    assert L.fadehip_mates_fix_batch(s._h, 1, buf, off, buf, i32, i32, buf, 48, None, buf) == -1
    assert L.fadehip_mates_fix_batch(s._h, 1, buf, off, buf, i32, i32, buf, 48, off, None) == -1
    assert L.fadehip_mateset_count(None, C.byref(n64), C.byref(n64)) == -1
    assert L.fadehip_mateset_count(s._h, None, C.byref(n64)) == -1
    assert "NULL" in L.fadehip_last_error(ctx._h).decode()
    assert s.count == (0, 0)
    got, fixed = s.fix_batch([], [], [], [])  # n = 0
    s.add_batch([], [], [], [])
    assert got == [] and len(fixed) == 0 and s.count == (0, 0)
