"""fadehip_coord_order_batch / Context.coord_order_batch: the sort kernels of bam_resort.hpp over records the caller brings,
against sorted() in Python — stable order by (refID as uint32, pos + 1 as uint32)."""
import random
import struct

import numpy as np
import pytest

import clip_cases as cc
import resort_model as rm

pytestmark = pytest.mark.gpu


def _rec(tid, pos, k=0, lseq=0):
    """A record of 36 bytes and up: one-letter name when k is None, else a name that tells the records of one key apart."""
    name = "" if k is None else "r%d" % k
    seq = "ACGT" * (lseq // 4) + "ACGT"[:lseq % 4]
    rec = bytearray(cc.build_rec(name, 0, 0, 0, 0, -1, -1, 0, "*", seq or "*", "I" * lseq))
    struct.pack_into("<ii", rec, 4, tid, pos)  # (any refID and pos: the bin, which no key reads, stays that of 0:0)
    return bytes(rec)


def _order(ctx, recs):
    off = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    cat = np.frombuffer(b"".join(recs), np.uint8) if recs else np.zeros(0, np.uint8)
    return [int(x) for x in ctx.coord_order_batch(cat, off)]


def _want(recs):
    return sorted(range(len(recs)), key=lambda i: (rm.key_in(recs[i]), i))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2048, 2049, 5000])
def test_random_keys_with_many_ties(ctx, n):
    rng = random.Random(n)
    recs = [_rec(rng.choice([0, 0, 1, 2, 300]), rng.choice([0, 1, 2, 3, 255, 256, 65535, 65536, (1 << 24) + 1, (1 << 31) - 2, rng.randrange(1 << 31)]), k) for k in range(n)]
    assert _order(ctx, recs) == _want(recs)


def test_sorted_reversed_and_equal(ctx):
    n = 4500  # (more than two tiles of the sort, not a multiple of one)
    up = [_rec(k // 2000, 7 * k, k) for k in range(n)]
    assert _order(ctx, up) == list(range(n))
    down = up[::-1]  # every record displaced
    assert _order(ctx, down) == list(range(n - 1, -1, -1))
    same = [_rec(1, 12345, k) for k in range(n)]
    assert _order(ctx, same) == list(range(n))


def test_unmapped_sorts_last(ctx):
    rng = random.Random(5)
    recs = [_rec(rng.choice([-1, -1, 0, 7, 2 ** 31 - 1]), rng.choice([-1, 0, 5, 2 ** 31 - 1]), k) for k in range(700)]
    got = _order(ctx, recs)
    assert got == _want(recs)
    keys = [rm.key_in(recs[i]) for i in got]
    first = next(j for j, k in enumerate(keys) if k >= rm.KEY_UNMAPPED)
    assert all(cc.decode_rec(recs[i])["tid"] == -1 for i in got[first:]) and all(cc.decode_rec(recs[i])["tid"] >= 0 for i in got[:first])
    assert rm.key(-1, -1) < rm.key(-1, 0)  # (pos -1 takes the low word 0: in front of pos 0 of the same refID)


def test_record_sizes_from_36_bytes_to_70_kb(ctx):
    rng = random.Random(9)
    recs = [_rec(0, rng.randrange(50), None, 0) for _ in range(40)]
    assert len(recs[0]) == 36 + 1
    small = cc.build_rec("", 0, 3, 0, 0, -1, -1, 0, "*", "*", "")
    assert len(small) == 37
    recs += [_rec(0, 25, 1000, 46000)]  # 36 + name + 23,000 + 46,000 bytes
    assert len(recs[-1]) > 69000
    recs += [_rec(rng.randrange(2), rng.randrange(50), 2000 + k, rng.randrange(0, 300)) for k in range(300)]
    rng.shuffle(recs)
    assert _order(ctx, recs) == _want(recs)


def test_malformed_record_and_null_arguments(ctx):
    import ctypes as C
    import fade_amd
    recs = [_rec(0, 5, 0), _rec(0, 4, 1)]
    bad = bytearray(recs[1])
    bad[0:4] = (len(bad) + 50).to_bytes(4, "little")
    with pytest.raises(fade_amd.FadeHipError) as e:
        _order(ctx, [recs[0], bytes(bad)])
    assert "record 1 is malformed" in str(e.value)
    off = np.zeros(2, np.int64)
    assert ctx._L.fadehip_coord_order_batch(ctx._h, 1, None, off.ctypes.data, None) == -1
    assert b"NULL argument" in ctx._L.fadehip_last_error(ctx._h)
