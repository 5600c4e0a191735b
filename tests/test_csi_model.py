"""tests/csi_model.py against itself and against tests/bai_model.py: (14, 5) is BAI's bin tree, hand cases at (4, 2) where the
limit is 1024, the derived loffset, read_csi(build(...)) round trips, and query() — written from the layout alone — against
brute force under four geometries, positions beyond 2^29 included."""
import random
import struct

import pytest

import bai_model as bm
import csi_model as cm
from test_bai_model import laid_out, rec

GEOMETRIES = [(4, 2), (6, 3), (14, 5), (14, 6)]


def test_geometry_bounds():
    assert cm.check_geometry(4, 1) and cm.check_geometry(14, 6) and cm.check_geometry(8, 8) and cm.check_geometry(29, 1)
    for bad in [(3, 2), (14, 0), (14, 9), (14, 7), (30, 1), (4, 10)]:
        assert not cm.check_geometry(*bad), bad
    assert cm.limit_of(14, 5) == bm.MAX_END and cm.limit_of(14, 6) == 1 << 32 and cm.limit_of(4, 2) == 1024


def test_14_5_is_bais_bin_tree():
    spans = [(0, 1), (0, 1 << 14), (0, (1 << 14) + 1), ((1 << 14) - 1, (1 << 14) + 1), ((1 << 17) - 1, (1 << 17) + 1),
             ((1 << 20) - 1, (1 << 20) + 1), ((1 << 23) - 1, (1 << 23) + 1), ((1 << 26) - 1, (1 << 26) + 1), ((1 << 29) - 1, 1 << 29),
             (0, 1 << 29), ((1 << 29) - 10, 1 << 29)]
    rng = random.Random(3)
    for _ in range(4000):
        beg = rng.randrange(1 << 29)
        end = min(beg + rng.choice([1, 2, 100, 16384, 16385, 1 << 17, 1 << 20, 1 << 23, 1 << 26, rng.randrange(1, 1 << 29)]), 1 << 29)
        spans.append((beg, end))
    for beg, end in spans:
        assert cm.reg2bin(beg, end, 14, 5) == bm.reg2bin(beg, end), (beg, end)
        assert sorted(cm.reg2bins(beg, end, 14, 5)) == sorted(bm.reg2bins(beg, end)), (beg, end)
    assert cm.pseudo_bin(5) == bm.PSEUDO_BIN == 37450 and cm.pseudo_bin(6) == 299594
    assert [cm.first_bin(level) for level in range(7)] == [0, 1, 9, 73, 585, 4681, 37449]


def test_hand_cases_at_4_2():
    # inside one 16-base leaf (level 2 begins at bin 9); across a 16-base line inside a 128-base bin (level 1, from bin 1);
    # across a 128-base line: the root
    assert cm.reg2bin(33, 47, 4, 2) == 9 + 2
    assert cm.reg2bin(40, 50, 4, 2) == 1 + 0
    assert cm.reg2bin(130, 260, 4, 2) == 0 and cm.reg2bin(120, 130, 4, 2) == 0
    assert cm.reg2bin(1008, 1024, 4, 2) == 9 + 63
    r = [rec(0, 33, 14, 0, 10), rec(0, 40, 10, 10, 20), rec(0, 120, 10, 20, 30), rec(0, 1000, 24, 30, 40)]
    c = cm.per_call(r, 4, 2)  # (the last ends at 1024: accepted)
    assert c["chunks"] == [(0, 11, 0, 10), (0, 1, 10, 20), (0, 0, 20, 30), (0, 8, 30, 40)]
    assert c["linear"] == [(0, 2, 0), (0, 3, 10), (0, 7, 20), (0, 8, 20), (0, 62, 30), (0, 63, 30)]
    assert c["refs"] == [(0, 0, 40, 4, 0)]
    with pytest.raises(cm.IndexError_) as e:
        cm.per_call(r[:3] + [rec(0, 1000, 25, 30, 40)], 4, 2, first_index=5)
    assert (e.value.kind, e.value.record) == ("span", 8)
    cm.per_call([rec(-1, 1000, 500, 0, 1)], 4, 2)  # without a reference the span does not count
    with pytest.raises(cm.IndexError_) as e:
        cm.per_call([rec(0, 10, 5, 0, 1), rec(0, 9, 5, 1, 2)], 4, 2)
    assert (e.value.kind, e.value.record) == ("order", 1)


def test_14_5_per_call_is_bais():
    rng = random.Random(11)
    specs, pos = [], 0
    for tid in (0, 1):
        pos = 0
        for _ in range(300):
            pos += rng.choice([0, 3, 500, 20_000])
            specs.append((tid, pos, rng.choice([0, 1, 100, 30_000, 200_000]), 4 if rng.random() < 0.05 else 0))
    recs = laid_out(specs + [(-1, -1, 0, 4)] * 3)
    assert cm.per_call(recs, 14, 5) == bm.per_call(recs)


def test_loffset_is_the_back_filled_value_and_0_behind_the_last_window():
    # (4, 2): windows of 16.  Record 0 covers windows 2 .. 3; record 1 (unmapped, placed) lies in leaf 9 + 5 whose first
    # window 5 has no entry: it takes window 6's; record 2 covers window 6; record 3 (unmapped, placed) lies in leaf 9 + 60,
    # behind the last window that has a value
    r = [rec(0, 33, 20, 100, 200), rec(0, 85, 0, 200, 300, flag=4), rec(0, 100, 5, 300, 400), rec(0, 970, 0, 400, 500, flag=4)]
    csi = cm.read_csi(cm.build(1, r, 4, 2))
    bins = csi["refs"][0]["bins"]
    assert sorted(bins) == [1, 9 + 5, 9 + 6, 9 + 60]
    assert bins[1] == (100, [(100, 200)])           # level 1, index 0: first window 0 is empty -> window 2's value
    assert bins[9 + 5] == (300, [(200, 300)])       # window 5 is empty -> window 6's value
    assert bins[9 + 6] == (300, [(300, 400)])
    assert bins[9 + 60] == (0, [(400, 500)])        # behind the last window
    assert csi["refs"][0]["meta"] == (100, 500, 2, 2) and csi["n_no_coor"] == 0
    assert (csi["min_shift"], csi["depth"], csi["aux"]) == (4, 2, b"")
    # the cut-off is used: the level-1 bin's chunk ends in front of the leaf's loffset, the largest of the bins that hold 100
    assert cm.query(csi, 0, 100, 105) == [(300, 400)]
    assert cm.query(csi, 0, 40, 105) == [(100, 200), (200, 300), (300, 400)]
    assert cm.query(csi, 0, 975, 980) == [(400, 500)] and cm.query(csi, 0, 1024, 2000) == []


def test_payload_layout_and_file_bytes():
    recs = laid_out([(0, 100, 50), (0, 200, 50, 4), (2, 5, 70_000), (-1, -1, 0, 4)])
    data = cm.build(3, recs, 14, 6)
    assert data[:20] == b"CSI\1" + struct.pack("<iiii", 14, 6, 0, 3)
    # reference 0: one bin and the pseudo-bin
    leaf = cm.first_bin(6)
    assert data[20:24] == struct.pack("<i", 2)
    assert data[24:40] == struct.pack("<IQi", leaf, recs[0]["u"], 1)
    assert data[40:56] == struct.pack("<QQ", recs[0]["u"], recs[1]["v"])
    assert data[56:72] == struct.pack("<IQi", 299594, 0, 2)
    assert data[72:104] == struct.pack("<QQQQ", recs[0]["u"], recs[1]["v"], 1, 1)
    assert data[104:108] == struct.pack("<i", 0)  # reference 1 is empty
    assert data[-8:] == struct.pack("<Q", 1)
    csi = cm.read_csi(data)
    assert csi["refs"][1] == dict(bins={}, meta=None)
    assert csi["refs"][2]["bins"] == {cm.reg2bin(5, 70_005, 14, 6): (recs[2]["u"], [(recs[2]["u"], recs[2]["v"])])}
    f = cm.file_bytes(data)
    assert f.endswith(cm.BGZF_EOF) and cm.payload_of(f) == data
    big = bytes(range(256)) * 600  # more than one member
    fb = cm.file_bytes(big)
    assert cm.payload_of(fb) == big and fb.count(b"\x1f\x8b\x08\x04") >= 4


def test_calls_compose():
    rng = random.Random(5)
    specs = []
    for tid in (0, 2):
        pos = 0
        for _ in range(300):
            pos += rng.randrange(0, 3)
            specs.append((tid, pos, rng.choice([1, 5, 15, 300]), 4 if rng.random() < 0.05 else 0))
    specs += [(-1, -1, 0, 4)] * 7
    recs = laid_out(specs)
    whole = cm.build(3, recs, 4, 2)
    for _ in range(20):
        cuts = sorted(rng.sample(range(len(recs) + 1), 5)) + [len(recs)]
        b, at = cm.Builder(3, 4, 2), 0
        for c in cuts + [len(recs)]:  # (the last call is empty)
            b.add(0, cm.per_call(recs[at:c], 4, 2, first_index=at))
            at = c
        assert b.finish() == whole
    b = cm.Builder(1, 4, 2)
    b.add(0, cm.per_call([rec(0, 10, 5, 0, 1)], 4, 2))
    with pytest.raises(cm.IndexError_) as e:
        b.add(0, cm.per_call([rec(0, 9, 5, 1, 2)], 4, 2))
    assert (e.value.kind, e.value.record) == ("order", 1)


def seeded_records(min_shift, depth, seed, n=600):
    """n sorted records on three references, their spans scaled to the geometry's limit; under (14, 6) reference 0 ends in the
    large positions: 2^29 - 10 with 20 reference bases, 2^29, 2^30 + 77, and 2^31 - 2 with one base."""
    rng = random.Random(seed)
    limit = cm.limit_of(min_shift, depth)
    win = 1 << min_shift
    specs = []
    for tid in range(3):
        pos = rng.choice([0, win - 1, 8 * win + 3])
        unit = max(min(limit // (2 * (n // 3)), 2 * win), 1)  # (steps that keep a third of the records inside the limit)
        for _ in range(n // 3):
            pos += rng.choice([0, 1, unit // 2, unit, 2 * unit])
            if pos >= limit:
                break
            reflen = min(rng.choice([0, 1, win // 4, win // 4, 2 * win, 9 * win, 70 * win]), limit - pos)
            specs.append((tid, pos, reflen, 4 if rng.random() < 0.04 else 0))
        if tid == 0 and limit > 1 << 31:
            specs += [(0, (1 << 29) - 10, 20), (0, 1 << 29, 100), (0, (1 << 30) + 77, 150), (0, (1 << 31) - 2, 1)]
    specs += [(-1, -1, 0, 4)] * 3
    return laid_out(specs, size=rng.choice([40, 333]), block=rng.choice([0x400, 0x7f00]))


def brute(recs, tid, beg, end):
    return [i for i, r in enumerate(recs) if r["tid"] == tid and not r["flag"] & 4 and cm.span_of(r)[0] < end and cm.span_of(r)[1] > beg]


def found(csi, recs, tid, beg, end):
    """What a reader gets: it scans the chunks query() names and keeps the mapped records that overlap."""
    hit = set()
    for cb, ce in cm.query(csi, tid, beg, end):
        for i, r in enumerate(recs):
            if cb <= r["u"] < ce and r["tid"] == tid and not r["flag"] & 4 and cm.span_of(r)[0] < end and cm.span_of(r)[1] > beg:
                hit.add(i)
    return sorted(hit)


def regions(recs, min_shift, depth, rng, n_random=300):
    win = 1 << min_shift
    mapped = [r for r in recs if r["tid"] >= 0 and not r["flag"] & 4]
    top = max(cm.span_of(r)[1] for r in mapped) + 3 * win
    out = []
    for _ in range(n_random):
        if rng.random() < 0.5:  # around a record's ends
            r = rng.choice(mapped)
            beg = max(cm.span_of(r)[rng.randrange(2)] + rng.choice([-1, 0, 1]) - rng.choice([0, 0, win]), 0)
            tid = r["tid"]
        else:
            beg, tid = rng.randrange(top), rng.randrange(3)
        out.append((tid, beg, beg + rng.choice([1, 10, win, win + 1, 8 * win, 100 * win])))
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_query_finds_what_brute_force_finds(geometry):
    min_shift, depth = geometry
    rng = random.Random(min_shift * 10 + depth)
    recs = seeded_records(min_shift, depth, seed=depth)
    assert len(recs) >= 500
    csi = cm.read_csi(cm.build(3, recs, min_shift, depth))
    n_hits = 0
    for tid, beg, end in regions(recs, min_shift, depth, rng):
        want = brute(recs, tid, beg, end)
        assert found(csi, recs, tid, beg, end) == want, (tid, beg, end)
        n_hits += len(want)
    assert n_hits > 300
    if geometry == (14, 6):
        for pos, n in (((1 << 29) - 10, 20), (1 << 29, 100), ((1 << 30) + 77, 150), ((1 << 31) - 2, 1)):
            want = brute(recs, 0, pos, pos + n)
            assert want and found(csi, recs, 0, pos, pos + n) == want
            assert found(csi, recs, 0, pos + n - 1, pos + n) == brute(recs, 0, pos + n - 1, pos + n) != []
