"""tests/resort_model.py against the sentences it states (FADEHIP_BAM_KEEP_SORTED): whatever the cut into calls, the calls'
output one behind the other is the stream in stable key order; what is held behind a call depends on where the call ends
and on nothing else; a key that decreases is reported at its record.  No GPU."""
import random

import pytest

import resort_model as rm


def _stream(rng, n):
    """n records of non-decreasing keys as they came in; some move up a little, some a lot, some are reset; ties abound."""
    recs, tid, pos = [], 0, 0
    for _ in range(n):
        r = rng.random()
        if r < 0.02 and tid < 3:
            tid, pos = tid + 1, 0
        elif r < 0.7:
            pos += rng.randrange(0, 4)
        k_in = rm.key(tid, pos)
        r = rng.random()
        k_out = k_in if r < 0.6 else rm.key(tid, pos + rng.randrange(0, 30)) if r < 0.9 else rm.KEY_UNMAPPED if r < 0.95 else rm.key(tid, pos + 5000)
        recs.append((k_in, k_out, rng.randrange(36, 400)))
    for _ in range(rng.randrange(0, 5)):  # the input's own unmapped tail
        recs.append((rm.KEY_UNMAPPED, rm.KEY_UNMAPPED, 80))
    return recs


def _cut(recs, edges):
    edges = [0] + sorted(edges) + [len(recs)]
    return [recs[a:b] for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("seed", range(6))
def test_output_is_the_stable_key_order_whatever_the_cut(seed):
    rng = random.Random(seed)
    recs = _stream(rng, 400)
    want = rm.stable_order([r[1] for r in recs])
    cuts = [[], list(range(1, len(recs))), [len(recs)], [0], sorted(rng.sample(range(len(recs) + 1), 7)), [5, 5, 5, 200]]
    for edges in cuts:
        res = rm.run(_cut(recs, edges))
        assert [s for c in res for s in c["emitted"]] == want, edges
        assert res[-1]["held"] == [] and res[-1]["held_bytes"] == 0
        assert sum(c["bytes"] for c in res) == sum(r[2] for r in recs)


def test_held_depends_on_where_the_call_ends_only():
    rng = random.Random(11)
    recs = _stream(rng, 300)
    seen = {}
    for trial in range(20):
        edges = sorted(rng.sample(range(1, len(recs)), rng.randrange(1, 12)))
        res = rm.run(_cut(recs, edges) + [[]])  # (an empty last call: every cut call is a call that holds)
        for end, c in zip(edges + [len(recs)], res):
            w = recs[end - 1][0]
            assert sorted(c["held"]) == [i for i in range(end) if recs[i][1] > w], (trial, end)
            assert seen.setdefault(end, c["held"]) == c["held"]
            assert c["held_bytes"] == sum(recs[i][2] for i in c["held"])
        assert res[-1]["held"] == []


def test_a_pile_up_holds_only_what_moved():
    k = rm.key(0, 100)
    recs = [(k, k, 50)] * 10 + [(k, rm.key(0, 130), 50)] + [(k, k, 50)] * 1000 + [(rm.key(0, 131), rm.key(0, 131), 50)]
    res = rm.run(_cut(recs, [300, 600, 900]))
    assert [c["held"] for c in res] == [[10], [10], [10], []]
    assert res[-1]["emitted"][-2:] == [10, 1011]


def test_a_decreasing_key_is_reported_at_its_record():
    recs = [(rm.key(0, p), rm.key(0, p), 40) for p in (1, 2, 3, 5, 4, 6)]
    for edges, call in (([], 0), ([4], 1), ([2, 5], 1), ([1, 2, 3, 4, 5], 4)):
        with pytest.raises(rm.OrderError) as e:
            rm.run(_cut(recs, edges))
        assert (e.value.index, e.value.call) == (4, call) and "record 4: not in coordinate order" in str(e.value)
    # a record that was moved up does not make the input unsorted: only the keys as they came in count
    rm.run([[(rm.key(0, 1), rm.key(0, 9), 40), (rm.key(0, 2), rm.key(0, 2), 40)]])
    # refID -1 sorts last, and pos -1 in front of pos 0
    assert rm.key(5, 1 << 30) < rm.key(-1, -1) == rm.KEY_UNMAPPED < rm.key(-1, 0)
