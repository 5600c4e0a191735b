"""The name set on the device (fadehip_nameset_*, bam_names.hpp) against tests/nameset_model.py, through contains and count:
names the dword compare can get wrong, duplicates within a wave, a block, a call and across calls, growth from sixteen slots
through several rehashes and a moved arena, the corner cases, a malformed record in the middle of an add, and independence
of the order and the cut of the calls.  Every case runs with the hash whole, cut to three bits and cut to none
(FADEHIP_NAMESET_HASH_BITS), and from the default table and from sixteen slots (FADEHIP_NAMESET_SLOTS): the answers are the
same."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import fade_amd
import nameset_model as nm

pytestmark = pytest.mark.gpu

SWITCHES = [(bits, slots) for bits in ("64", "3", "0") for slots in (None, "16")]


@pytest.fixture(params=SWITCHES, ids=lambda p: "bits%s-slots%s" % (p[0], p[1] or "default"))
def make_set(request, ctx, monkeypatch):
    bits, slots = request.param
    monkeypatch.setenv("FADEHIP_NAMESET_HASH_BITS", bits)
    if slots is None:
        monkeypatch.delenv("FADEHIP_NAMESET_SLOTS", raising=False)
    else:
        monkeypatch.setenv("FADEHIP_NAMESET_SLOTS", slots)
    made = []

    def make():
        made.append(ctx.nameset())
        return made[-1]

    yield make
    for s in made:
        s.close()


def _check(s, names, probes):
    """contains over the probes and count, against the model's set."""
    got = s.contains(probes)
    assert got.dtype == np.uint8 and got.tolist() == nm.contains(names, probes)
    assert s.count == len(names)


def _never_added(n, tag):
    return [nm.rec(b"absent_%s_%d" % (tag.encode(), k)) for k in range(n)]


def test_names_the_compare_can_get_wrong(make_set):
    s = make_set()
    long_a = bytes(65 + k % 26 for k in range(254))
    added = [b"a", b"ab", b"abc", b"abcd", b"abcde", long_a,        # lengths 1 .. 5 and 254 characters
             b"read10", b"q/1", b"wxyzA", b"0123456789abcdefX"]      # last byte; prefix; bytes behind a dword boundary
    close = [b"b", b"aa", b"abd", b"abce", b"abcdf", long_a[:-1] + b"!", long_a[:-1], long_a[:128] + b"!" + long_a[129:],
             b"read11", b"read1", b"read100", b"q/2", b"q/", b"q", b"wxyzB", b"wxyz", b"0123456789abcdefY", b"0123456789abcdeXf",
             b"0123456789abXdef", b"0123X56789abcdefX", b"abcd\x01", b"ab\x00c"]
    recs = [nm.rec(n) for n in added]
    s.add(recs)
    names = nm.name_set(recs)
    assert len(names) == len(added)
    _check(s, names, recs + [nm.rec(n) for n in close])
    # the same name behind other aux bytes (the bytes behind the name must not matter), and in the other direction
    _check(s, names, [nm.rec(n, b"XXZjunk\0") for n in added + close])
    s2 = make_set()
    recs2 = [nm.rec(n) for n in close]
    s2.add(recs2)
    _check(s2, nm.name_set(recs2), recs2 + recs)


def test_duplicates_in_a_wave_a_block_a_call_and_across_calls_count_once(make_set):
    s = make_set()
    names = [b"frag%d" % k for k in range(700)]
    # lanes 3 and 40 of one wave; waves 0 and 2 of one block; blocks 0 and 2 of one call
    names[40] = names[3]
    names[130] = names[5]
    names[600] = names[7]
    names[601] = names[300]
    recs = [nm.rec(n) for n in names]
    s.add(recs)
    model = nm.name_set(recs)
    assert len(model) == 696
    _check(s, model, recs + _never_added(300, "d"))
    s.add(recs[100:400])  # a second call: nothing new
    _check(s, model, recs + _never_added(300, "d"))
    more = [nm.rec(b"frag%d" % k) for k in range(650, 900)] * 2  # names the set holds and new ones, each twice
    s.add(more)
    model |= nm.name_set(more)
    assert len(model) > 696 + 190
    _check(s, model, recs + more + _never_added(300, "e"))
    # one name in every lane of several blocks
    same = [nm.rec(b"everyone")] * 600
    s.add(same)
    model |= nm.name_set(same)
    _check(s, model, same[:3] + recs[:50] + _never_added(50, "f"))


def test_growth_from_sixteen_slots_through_rehashes_and_a_moved_arena(make_set):
    s = make_set()
    model, seen, at = set(), [], 0
    for n in (40, 400, 1500):
        # names of 60 characters: 1,500 of them do not fit the first arena (64 KiB), which has to move
        recs = [nm.rec(b"grow_%06d_" % k + b"x" * 48) for k in range(at, at + n)]
        at += n
        s.add(recs)
        seen += recs
        model |= nm.name_set(recs)
        _check(s, model, seen + _never_added(len(seen), "g%d" % n))
    assert s.count == 1940


def test_corner_cases(make_set):
    s = make_set()
    recs = [nm.rec(b"r%d" % k) for k in range(300)]
    assert s.count == 0 and s.contains(recs).tolist() == [0] * 300   # an empty set
    s.add([])                                                       # n = 0
    assert s.contains([]).tolist() == [] and s.count == 0
    s.add(recs, pick=np.zeros(300, np.uint8))                        # pick all zero
    assert s.count == 0 and s.contains(recs).tolist() == [0] * 300
    pick = np.zeros(300, np.uint8)
    pick[[0, 63, 64, 255, 256, 299]] = [1, 2, 255, 1, 128, 1]        # (any non-zero byte picks)
    s.add(recs, pick=pick)
    _check(s, nm.name_set(recs, pick), recs)
    s.add(recs)                                                      # pick = NULL: every record
    _check(s, nm.name_set(recs), recs + _never_added(100, "c"))


def test_null_arrays_are_refused_and_leave_the_set_alone(make_set, ctx):
    s = make_set()
    s.add([nm.rec(b"kept")])
    L = ctx._L
    off = (C.c_int64 * 2)(0, 40)
    buf = (C.c_uint8 * 48)()
    assert L.fadehip_nameset_add_batch(s._h, 1, None, off, None) == -1
    assert L.fadehip_nameset_add_batch(s._h, 1, buf, None, None) == -1
    assert L.fadehip_nameset_contains_batch(s._h, 1, buf, off, None) == -1
    assert L.fadehip_nameset_contains_batch(s._h, 1, None, off, buf) == -1
    assert L.fadehip_nameset_count(s._h, None) == -1
    assert s.count == 1 and s.contains([nm.rec(b"kept"), nm.rec(b"kepu")]).tolist() == [1, 0]


def test_a_record_whose_name_runs_past_its_block_size_fails_the_add_and_leaves_the_set_as_it_was(make_set):
    s = make_set()
    first = [nm.rec(b"before%d" % k) for k in range(300)]
    s.add(first)
    model = nm.name_set(first)
    probes = first + _never_added(100, "b")
    _check(s, model, probes)
    recs = [nm.rec(b"after%d" % k) for k in range(500)]
    bad = bytearray(recs[257])
    bad[12] = len(bad) - 36 + 1  # l_read_name: one byte more than the record holds
    recs[257] = bytes(bad)
    with pytest.raises(fade_amd.FadeHipError) as e:
        s.add(recs)
    assert e.value.code == -1 and "record 257" in str(e.value), str(e.value)
    with pytest.raises(fade_amd.FadeHipError) as e:
        s.contains(recs)
    assert e.value.code == -1 and "record 257" in str(e.value)
    bad_bs = bytearray(recs[3])
    struct.pack_into("<I", bad_bs, 0, len(bad_bs))  # block_size: four bytes more than the record holds
    with pytest.raises(fade_amd.FadeHipError) as e:
        s.add(recs[:3] + [bytes(bad_bs)])
    assert "record 3" in str(e.value)
    _check(s, model, probes + recs[:257] + recs[258:])


def test_the_order_and_the_cut_of_the_calls_do_not_matter(make_set):
    rng = random.Random(20261019)
    recs = [nm.rec(b"n%d" % rng.randrange(900), b"XYZ%d\0" % k) for k in range(1500)]  # (~900 distinct names, most of them twice)
    pick = [1 if rng.random() < 0.6 else 0 for _ in recs]
    model = nm.name_set(recs, pick)
    probes = recs + _never_added(300, "o")
    a = make_set()
    a.add(recs, pick=np.array(pick, np.uint8))
    _check(a, model, probes)
    order = list(range(len(recs)))
    rng.shuffle(order)
    b = make_set()
    b.add([recs[k] for k in order], pick=np.array([pick[k] for k in order], np.uint8))
    _check(b, model, probes)
    c = make_set()
    for lo, hi in ((0, 1), (1, 65), (65, 700), (700, 700), (700, 1500)):
        c.add(recs[lo:hi], pick=np.array(pick[lo:hi], np.uint8))
    _check(c, model, probes)
    assert a.contains(probes).tolist() == b.contains(probes).tolist() == c.contains(probes).tolist()
