"""(no GPU) tests/sorted_out_model.py on hand cases — bucket edges at pos + 1 = 65535 / 65536, a pos beyond the contig, refID -1
with a pos, contigs shorter than one bucket, empty buckets between windows, a bucket alone over the budget — and
build/sortwin_selftest (host/recstore_host.hpp's bucket_layout / choose_windows on the same cases and on random tables against
a plain loop), a stand-alone program built with ASan + UBSan."""
import os
import struct
import subprocess

import pytest

import sorted_out_model as sm

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fade_amd", "csrc")
LEN = [200000, 10, 65535, 65534, 0]   # the selftest's header


def _key(tid, pos):
    return ((tid & 0xffffffff) << 32) | ((pos + 1) & 0xffffffff)


def _rec(tid, pos, size=40):
    return struct.pack("<Iii", size - 4, tid, pos) + bytes(size - 12)


def test_layout():
    assert sm.layout(LEN) == ([0, 4, 5, 7, 8], [4, 1, 2, 1, 1], 10)
    assert sm.layout([]) == ([], [], 1)
    assert sm.layout([0xffffffff])[1] == [65537]


@pytest.mark.parametrize("tid, pos, want", [
    (0, -1, 0), (0, 65534, 0), (0, 65535, 1), (0, 199999, 3),
    (0, 2000000000, 3), (0, -2, 3),                      # beyond the contig: its last bucket
    (1, 0, 4), (1, 70000, 4),                            # a contig shorter than one bucket
    (2, 65534, 5), (2, 65535, 6), (3, 65535, 7), (4, 5, 8),
    (-1, -1, 9), (-1, 77, 9), (5, 0, 9), (0x7fffffff, 0, 9),   # refID -1 with and without a pos; a refID outside the header
])
def test_bucket_hand_cases(tid, pos, want):
    assert sm.bucket(LEN, _key(tid, pos)) == want
    assert sm.key(_rec(tid, pos)) == _key(tid, pos)


def test_bucket_ranges_are_inclusive_abut_and_map_back():
    assert sm.bucket_range(LEN, 0) == (0, 65535, 0)
    assert sm.bucket_range(LEN, 1) == (65536, 131071, 0)
    assert sm.bucket_range(LEN, 3) == (3 * 65536, 0xffffffff, 0)
    assert sm.bucket_range(LEN, 4) == (1 << 32, (1 << 32) | 0xffffffff, 1)
    assert sm.bucket_range(LEN, 6) == ((2 << 32) | 65536, (2 << 32) | 0xffffffff, 2)
    assert sm.bucket_range(LEN, 9) == (5 << 32, sm.ALL, -1)
    nxt = 0
    for b in range(10):
        lo, hi, _ = sm.bucket_range(LEN, b)
        assert lo == nxt and sm.bucket(LEN, lo) == b == sm.bucket(LEN, hi)
        nxt = hi + 1
    assert nxt == 1 << 64
    assert sm.bucket_range([], 0) == (0, sm.ALL, -1) and sm.bucket([], _key(0, 5)) == 0
    assert sm.KEY_UNMAPPED == _key(-1, -1) and sm.bucket(LEN, sm.KEY_UNMAPPED) == 9


def test_bucket_is_monotone_in_the_key():
    keys = sorted(_key(t, p) for t in (-1, 0, 1, 2, 3, 4, 5) for p in (-2, -1, 0, 9, 10, 65533, 65534, 65535, 65536, 131070, 131071, 199999, 200000, 1 << 30))
    bs = [sm.bucket(LEN, k) for k in keys]
    assert bs == sorted(bs) and set(bs) == set(range(10))


def test_windows_hand_cases():
    by, rc = [100, 0, 0, 300, 0, 136, 0], [1, 0, 0, 2, 0, 1, 0]       # costs 164, 0, 0, 428, 0, 200, 0
    assert sm.windows(by, rc, 1000) == [(0, 7)]
    assert sm.windows(by, rc, 428) == [(0, 3), (3, 5), (5, 7)]          # empty buckets stay with the window in front
    assert sm.windows(by, rc, 592) == [(0, 5), (5, 7)]
    assert sm.windows(by, rc, 591) == [(0, 3), (3, 5), (5, 7)]
    for budget, bad in ((427, 3), (199, 3), (163, 0), (0, 0)):          # a bucket alone over the budget is named
        with pytest.raises(sm.BucketOverBudget) as e:
            sm.windows(by, rc, budget)
        assert e.value.bucket == bad
    assert sm.windows([0] * 4, [0] * 4, 0) == [(0, 4)]
    assert sm.cost(100, 1) == 164


def test_the_window_loop_yields_the_one_window_order_at_every_budget():
    import random
    rng = random.Random(3)
    recs = [_rec(rng.choice([-1, 0, 0, 0, 1, 2, 3, 4, 7]), rng.randrange(-1, 210000), 40 + rng.randrange(60)) for _ in range(600)]
    want = sm.order(recs)
    nbytes, nrec = sm.histogram(LEN, recs)
    assert sum(nbytes) == sum(map(len, recs)) and sum(nrec) == len(recs)
    most = max(sm.cost(b, n) for b, n in zip(nbytes, nrec))
    seen = set()
    for budget in (1 << 40, 3 * most, most):
        per = sm.in_windows(LEN, recs, budget)
        seen.add(len(per))
        assert [r for w in per for r in w] == want
    assert len(seen) == 3 and min(seen) == 1   # (three different cuts of the same order)


def test_sortwin_selftest_under_asan_and_ubsan():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/sortwin_selftest"])
    p = subprocess.run([os.path.join(CSRC, "build", "sortwin_selftest")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout.decode().strip() == "sortwin_selftest ok", p.stdout.decode() + p.stderr.decode()
