"""Intervals and queries for the interval-set tests (test_intervals_model.py, test_gpu_intervals.py), built by seed: the
smallest shapes at which the sort, the running maximum and the binary search of bam_intervals.hpp can go wrong.  Intervals
are (chrom id, start, end) over NAMES; queries likewise, with ids outside NAMES among them."""
import random

import intervals_model as im

NAMES = ["cA", "cB", "cC", "cEmpty"]  # the last one never gets an interval
SPAN = 2_000_000
# the edges of the 256-wide scan block and of the 2048-item sort tile
COUNTS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 5000)
MAX_END = im.MAX_END


def intervals(n, seed):
    """n short intervals over the first three contigs, every tenth a copy of an earlier one, in no order"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        if out and len(out) % 10 == 9:
            out.append(rng.choice(out))
            continue
        s = rng.randrange(SPAN)
        out.append((rng.randrange(3), s, s + rng.choice([1, 2, 50, 300, 5000])))
    rng.shuffle(out)
    return out


def queries(ivs, n, seed):
    """n queries: at random, and at the edges of intervals drawn from ivs — touching on either side, one base of overlap on
    either side, empty inside, a negative start — and on ids the set does not have"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        kind = rng.randrange(10)
        if kind < 3 or not ivs:
            s = rng.randrange(-500, SPAN + 6000)
            out.append((rng.randrange(4), s, s + rng.choice([0, 1, 7, 150, 400, 20_000])))
            continue
        c, s, e = rng.choice(ivs)
        w = rng.choice([1, 2, 100])
        q = ((c, s - w, s), (c, e, e + w), (c, s - w, s + 1), (c, e - 1, e + w), (c, s, s), (c, -rng.randrange(1, 1 << 40), s + rng.randrange(2)),
             (rng.choice([-1, 4, 9, -(1 << 31), (1 << 31) - 1]), s, e))[kind - 3]
        out.append(q)
    return out


def as_model(ivs, names=NAMES):
    m = im.IntervalModel(names)
    m.add([(names[c], s, e) for c, s, e in ivs])
    return m


def expect(model, qs, names=NAMES):
    return [int(model.hit(names[c] if 0 <= c < len(names) else b"?", s, e)) for c, s, e in qs]


# ---- the hand cases: (intervals, [(query, hit)])
def hand_cases():
    cases = {}
    iv = [(0, 100, 200)]
    cases["touch_misses_one_base_hits"] = (iv, [((0, 50, 100), 0), ((0, 200, 250), 0), ((0, 50, 101), 1), ((0, 199, 250), 1), ((0, 100, 200), 1), ((0, 0, 1 << 40), 1)])
    cases["empty_query_inside"] = (iv, [((0, 150, 150), 0), ((0, 151, 150), 0), ((0, 150, 151), 1)])
    cases["negative_start"] = ([(0, 0, 5), (0, 100, 200)], [((0, -8, 0), 0), ((0, -8, 1), 1), ((0, -(1 << 62), -1), 0), ((0, -(1 << 62), 1 << 62), 1), ((1, -8, 1), 0)])
    cases["unknown_name"] = (iv, [((1, 100, 200), 0), ((3, 100, 200), 0), ((-1, 100, 200), 0), ((4, 100, 200), 0), ((1 << 30, 100, 200), 0)])
    # a long early interval covers a query that lies beyond many later-starting ones
    early = [(1, 10, 1_000_000)] + [(1, 20 + 10 * k, 25 + 10 * k) for k in range(1000)]
    cases["long_early_interval"] = (early, [((1, 500_000, 500_001), 1), ((1, 999_999, 1_000_050), 1), ((1, 1_000_000, 1_000_050), 0), ((1, 0, 10), 0), ((0, 500_000, 500_001), 0)])
    # the last interval of contig A reaches far; a query on contig B that sits before B's first start misses
    cases["last_of_A_reaches_far"] = ([(0, 10, 20), (0, 500, MAX_END), (1, 1000, 1010), (1, 2000, 2010)],
                                      [((1, 600, 700), 0), ((1, 0, 1000), 0), ((1, 1500, 1600), 0), ((1, 1005, 1006), 1), ((0, 600, 700), 1), ((2, 600, 700), 0)])
    return cases


def long_at_front(blocks=4):
    """one interval [0, 2^31 - 1) at the front of contig cB with `blocks` scan blocks of short intervals behind it, and a
    query that only it covers"""
    ivs = [(1, 0, MAX_END)] + [(1, 1000 + 10 * k, 1005 + 10 * k) for k in range(256 * blocks)] + [(0, 5, 6), (2, 5, 6)]
    far = 1000 + 10 * 256 * blocks + 12345
    return ivs, [((1, far, far + 1), 1), ((1, MAX_END - 1, MAX_END + 5), 1), ((1, MAX_END, MAX_END + 5), 0), ((0, far, far + 1), 0), ((2, far, far + 1), 0)]


def long_at_end_of_a(blocks=4):
    """the same interval as the LAST of contig cA (the largest start there), `blocks` scan blocks of short intervals on cB
    behind it, and queries on cB that no interval of cB covers"""
    ivs = [(0, 10 * k, 10 * k + 5) for k in range(300)] + [(0, 5000, MAX_END)] + [(1, 1000 + 10 * k, 1005 + 10 * k) for k in range(256 * blocks)]
    return ivs, [((1, 0, 1000), 0), ((1, 1005, 1010), 0), ((1, 1000 + 10 * 700 + 5, 1000 + 10 * 700 + 10), 0), ((1, 50_000, 60_000), 0), ((1, 1004, 1005), 1),
                 ((0, 50_000, 60_000), 1), ((2, 50_000, 60_000), 0)]
