"""fadehip_eject_batch / Context.eject_batch: filter.d:209-265 (plain `fade out`) over records brought to the device — the
kernels the file path runs under FADEHIP_BAM_EJECT / FADEHIP_BAM_EJECT_GROUPS — against the restatement in `_ref` below.
The records are minimal (36 bytes and the name, l_seq 0): the kernels look at l_read_name, the name and rs only."""
import struct

import numpy as np
import pytest

import fade_amd

pytestmark = pytest.mark.gpu

TAG_BLOCK = 256  # records per block of the kernels; 1,024 blocks per thread range of the block scan


def _rec(name):
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, 0, -1, -1, 0) + name + b"\0"
    return struct.pack("<I", len(body)) + body


def _ref(names, rs, grouped):
    art = [bool(v & 6) for v in rs]
    if not grouped:
        return [not a for a in art]
    keep, k = [], 0
    while k < len(names):
        e = k
        while e < len(names) and names[e] == names[k]:
            e += 1
        keep += [not any(art[k:e])] * (e - k)
        k = e
    return keep


def _check(ctx, names, rs):
    """Both modes against _ref; returns the grouped answer."""
    recs = [_rec(n) for n in names]
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    cat = np.frombuffer(b"".join(recs), dtype=np.uint8)
    got = {}
    for grouped in (0, 1):
        keep = ctx.eject_batch_packed(cat, off, rs, grouped).astype(bool)
        want = np.array(_ref(names, rs, grouped), dtype=bool)
        bad = np.nonzero(keep != want)[0]
        assert not len(bad), (grouped, len(names), bad[:5], [(names[k], rs[k]) for k in bad[:5]])
        got[grouped] = keep
    assert (got[0] == [not (v & 6) for v in rs]).all()
    return got[1]


SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262144 + 300]  # the last: the block scan's threads take two blocks each


@pytest.mark.parametrize("n", SIZES)
def test_every_size_singletons_one_group_and_groups_that_start_at_64_and_256(ctx, n):
    rs_some = [(2, 4, 6, 7, 39)[i % 5] if i % 7 == 3 else (0, 1, 33, 9)[i % 4] for i in range(n)]  # (bits other than 2 and 4 never eject)
    # all singletons
    keep = _check(ctx, [b"s%d" % i for i in range(n)], rs_some)
    assert n < 8 or (keep.any() and not keep.all())
    # one group over everything: its only artifact in the middle, then none
    one = [b"*"] * n
    assert not _check(ctx, one, [4 if i == n // 2 else 1 for i in range(n)]).any()
    assert _check(ctx, one, [1] * n).all()
    # groups that start exactly at records 64 and 256, the artifact the last record of a group
    bounds = [b for b in (0, 64, 256) if b < n] + [n]
    names = [b"g%d" % sum(i >= b for b in bounds[1:-1]) for i in range(n)]
    heads = [i for i in range(n) if i == 0 or names[i] != names[i - 1]]
    assert heads == bounds[:-1]
    for hit in range(len(heads)):
        rs = [0] * n
        rs[bounds[hit + 1] - 1] = 2
        keep = _check(ctx, names, rs)
        for g in range(len(heads)):
            assert keep[bounds[g]:bounds[g + 1]].all() == (g != hit) and keep[bounds[g]:bounds[g + 1]].any() == (g != hit)


@pytest.mark.parametrize("where", ["first", "last", "middle", "absent"])
def test_a_600_record_group_over_three_blocks(ctx, where):
    lo, hi = 100, 700
    assert lo // TAG_BLOCK == 0 and (lo + 300) // TAG_BLOCK == 1 and (hi - 1) // TAG_BLOCK == 2
    names = [b"a%d" % i for i in range(lo)] + [b"grp"] * (hi - lo) + [b"z%d" % i for i in range(100)]
    rs = [1] * len(names)
    at = {"first": lo, "last": hi - 1, "middle": lo + 300, "absent": None}[where]
    if at is not None:
        rs[at] = 6
    keep = _check(ctx, names, rs)
    assert keep[:lo].all() and keep[hi:].all()
    assert keep[lo:hi].all() if at is None else not keep[lo:hi].any()


@pytest.mark.parametrize("seed", range(10))
def test_random_groups_of_1_to_5_with_five_per_cent_artifacts(ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    n = 20000
    lens = rng.integers(1, 6, size=n)
    gid = np.repeat(np.arange(n), lens)[:n]
    names = [b"q%d" % g for g in gid]
    rs = [int(v) for v in np.where(rng.random(n) < 0.05, rng.choice([2, 4, 6, 35], size=n), rng.choice([0, 1, 33], size=n))]
    keep = _check(ctx, names, rs)
    # the case's own content: kept and ejected groups across a 256 boundary, ejected records that are no artifact themselves
    starts = np.nonzero(np.r_[True, gid[1:] != gid[:-1]])[0]
    ends = np.r_[starts[1:], n]
    across = [(s, e) for s, e in zip(starts, ends) if s // TAG_BLOCK != (e - 1) // TAG_BLOCK]
    n_kept = sum(1 for s, e in across if keep[s])
    n_ej = sum(1 for s, e in across if not keep[s])
    innocent = sum(1 for k in range(n) if not keep[k] and not rs[k] & 6)
    assert n_kept >= 3 and n_ej >= 3 and innocent >= 300, (n_kept, n_ej, innocent)
    assert all(keep[s:e].all() or not keep[s:e].any() for s, e in zip(starts, ends))


def test_names_that_differ_late_or_in_length(ctx):
    long_a, long_b = b"N" * 253 + b"a", b"N" * 253 + b"b"  # 254 bytes: l_read_name 255, the last byte differs
    pairs = [
        (b"a", b"b"),                                   # length 1
        (long_a, long_b),
        (b"read_0001x", b"read_0001y"),                 # the last byte, in the third dword
        (b"abcx", b"abcy"), (b"abcdefgx", b"abcdefgy"),  # ... at the end of a dword (l_read_name 5 and 9: the NUL starts the next)
        (b"abx", b"aby"), (b"x", b"y"), (b"abcdx", b"abcdy"),
        (b"P" * 64 + b"tail1", b"P" * 64 + b"tail2"),   # only beyond byte 64
        (b"P" * 70 + b"1" + b"Q" * 20, b"P" * 70 + b"2" + b"Q" * 20),
        (b"r1", b"r10"),
        (b"ab", b"ab\0"), (b"abc", b"abc\0"), (b"abcd", b"abcd\0\0"),  # equal bytes, another l_read_name
    ]
    assert len(_rec(long_a)) == 36 + 255 and _rec(b"ab")[12 + 0] == 3 and _rec(b"ab\0")[12] == 4
    names, rs, want = [], [], []
    for a, b in pairs:
        assert a != b
        # a and b are two groups, whichever carries the artifact; a next to a is one
        names += [a, b, b"sep", b, a, b"sep2", a, a, b"sep3", b, b]
        rs += [2, 0, 0, 0, 4, 0, 6, 1, 0, 0, 2]
        want += [False, True, True, True, False, True, False, False, True, False, False]
    keep = _check(ctx, names, rs)
    assert list(keep) == want
    # every pair on its own, too: the name of the batch's last record ends the buffer
    for a, b in pairs:
        assert list(_check(ctx, [a, b], [2, 0])) == [False, True]
        assert list(_check(ctx, [b, b], [0, 2])) == [False, False]


def test_a_damaged_l_read_name_is_refused_with_the_records_index(ctx):
    recs = [_rec(b"r%d" % i) for i in range(6)]
    for k, ln in ((3, 200), (5, 255), (0, 0), (2, len(recs[2]) - 36 + 1)):
        batch = list(recs)
        batch[k] = batch[k][:12] + bytes([ln]) + batch[k][13:]
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.eject_batch(batch, [0] * 6, True)
        assert e.value.code == -1 and ("record %d " % k) in str(e.value), str(e.value)
    short = list(recs)
    short[4] = struct.pack("<I", 400) + short[4][4:]  # block_size beyond the bytes
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.eject_batch(short, [0] * 6, False)
    assert e.value.code == -1 and "record 4 " in str(e.value)
    # the context still works, and an empty batch is no error
    assert list(ctx.eject_batch(recs, [0, 2, 0, 4, 1, 0], True)) == [True, False, True, False, True, True]
    assert len(ctx.eject_batch([], [], True)) == 0
