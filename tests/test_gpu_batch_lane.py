"""fadehip_clip_batch, fadehip_extract_batch and fadehip_eject_batch share one stream and one set of device buffers per
context, under one lock.  What that can get wrong, and what the three functions' own tests (a function at a time) cannot see:
a buffer another function has grown and left its bytes in, and two functions in the buffers at once.  Every call here must
return, byte for byte, what the same call returns on a context that has seen no other call; those single calls are held to
the oracle by test_gpu_clip_batch / test_gpu_extract_batch / test_gpu_eject_batch, whose records these are."""
import threading

import pytest

import clip_cases as cc
import fade_amd
import test_gpu_eject_batch as ej
import test_gpu_extract_batch as xb

pytestmark = pytest.mark.gpu

CLIP = cc.cases()


def _clip(c, n, r):
    pick = [CLIP[(r + 3 * k) % len(CLIP)] for k in range(n)]
    return c.clip_batch([cc.to_bam(p["rec"], p["aux"]) for p in pick], [p["rs"] for p in pick], [p["tl"] for p in pick], [p["tr"] for p in pick])


def _eject(c, n, r):
    names = [b"g%d" % ((k + r) // 3) for k in range(n)]  # groups of three, the first and last cut short
    rs = [(2, 4, 6)[k % 3] if (k + r) % 11 == 0 else (0, 1, 33)[k % 3] for k in range(n)]
    return c.eject_batch([ej._rec(m) for m in names], rs, True).tobytes()


def _extract(c, n, r):
    pick = [xb.CASES[(r + 5 * k) % len(xb.CASES)] for k in range(n)]
    return c.extract_batch([p["rec"] for p in pick], [p["rs"] for p in pick], [xb._sides_arg(p) for p in pick])


CALLS = (_clip, _eject, _extract)
ROUNDS = ((300, 0), (1, 1), (300, 2))  # (records, which ones): the buffers grow, are larger than needed, are full again with other bytes


@pytest.fixture(scope="module")
def alone():
    """Every call of this file on a context of its own."""
    want = {}
    for f in CALLS:
        for n, r in ROUNDS:
            c = fade_amd.Context(device=0)
            want[f, n, r] = f(c, n, r)
            c.close()
    assert all(len(want[f, 300, 0]) >= 300 and want[f, 300, 0] != want[f, 300, 2] for f in CALLS)
    assert 0 < want[_eject, 300, 0].count(b"\0") < 300
    return want


def test_interleaved_calls_on_one_context_equal_the_calls_alone(alone):
    c = fade_amd.Context(device=0)
    got = {(f, n, r): f(c, n, r) for n, r in ROUNDS for f in CALLS}
    c.close()
    assert [key[0].__name__ for key in got if got[key] != alone[key]] == []


def test_concurrent_calls_on_one_context_equal_the_calls_alone(alone):
    c = fade_amd.Context(device=0)
    got, errors = {}, []

    def run(f):
        try:
            got[f] = f(c, 300, 0)
        except Exception as e:  # (a thread's exception would otherwise be lost)
            errors.append((f.__name__, repr(e)))

    threads = [threading.Thread(target=run, args=(f,)) for f in CALLS]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    c.close()
    assert not errors, errors
    assert [f.__name__ for f in CALLS if got[f] != alone[f, 300, 0]] == []
