"""tests/bai_model.py against itself: hand cases of the index rule, read_bai(build(...)) round trips, and query() — written from
the specification alone — against brute force over random sorted record sets."""
import random
import struct

import pytest

import bai_model as bm


def rec(tid, pos, reflen, u, v, flag=0):
    return dict(tid=tid, pos=pos, flag=flag, reflen=reflen, u=u, v=v)


def laid_out(specs, size=100, block=0x1000, member=0x300):
    """Records (tid, pos, reflen[, flag]) of `size` bytes each, back to back from file offset 0 in blocks of `block` bytes whose
    members take `member` bytes: the records with their u and v."""
    total = size * len(specs)
    nb = (total + block - 1) // block
    coff = [k * member for k in range(nb)]
    out = []
    for i, s in enumerate(specs):
        u = bm.virtual_offset(i * size, block, coff, total, nb * member)
        v = bm.virtual_offset((i + 1) * size, block, coff, total, nb * member)
        out.append(rec(s[0], s[1], s[2], u, v, s[3] if len(s) > 3 else 0))
    return out


def test_reg2bin_levels():
    assert bm.reg2bin(0, 1) == 4681
    assert bm.reg2bin(0, 1 << 14) == 4681
    assert bm.reg2bin(0, (1 << 14) + 1) == 585
    assert bm.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585
    assert bm.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73
    assert bm.reg2bin((1 << 20) - 1, (1 << 20) + 1) == 9
    assert bm.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    assert bm.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    assert bm.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767


def test_virtual_offsets_abut():
    coff = [0, 700, 1500]
    assert bm.virtual_offset(0, 1000, coff, 2500, 2100) == 0
    assert bm.virtual_offset(999, 1000, coff, 2500, 2100) == 999
    assert bm.virtual_offset(1000, 1000, coff, 2500, 2100) == 700 << 16
    assert bm.virtual_offset(2499, 1000, coff, 2500, 2100) == (1500 << 16) | 499
    assert bm.virtual_offset(2500, 1000, coff, 2500, 2100) == 2100 << 16
    # a total that is a whole number of blocks: the end is behind the last member, not at a member that does not exist
    assert bm.virtual_offset(2000, 1000, coff[:2], 2000, 1500) == 1500 << 16


def test_chunks_are_runs_of_one_bin():
    r = [rec(0, 10, 50, 0, 10), rec(0, 20, 50, 10, 20), rec(0, 16380, 10, 20, 30), rec(0, 16390, 5, 30, 40), rec(0, 16400, 5, 40, 50)]
    c = bm.per_call(r)
    assert c["chunks"] == [(0, 4681, 0, 20), (0, 585, 20, 30), (0, 4682, 30, 50)]
    assert c["refs"] == [(0, 0, 50, 5, 0)]
    assert c["linear"] == [(0, 0, 0), (0, 1, 20)]
    assert (c["first_key"], c["last_key"], c["n"]) == (11, 16401, 5)


def test_span_rules():
    # reflen 0 counts as 1; pos -1 with a tid begins at 0; flag 4 takes reflen 0, makes a chunk, stays out of the linear index
    r = [rec(1, -1, 0, 0, 5), rec(1, 16384, 0, 5, 9), rec(1, 16384, 40000, 9, 12, flag=4), rec(1, 16385, 3, 12, 20)]
    c = bm.per_call(r)
    assert c["chunks"] == [(1, 4681, 0, 5), (1, 4682, 5, 20)]
    assert c["linear"] == [(1, 0, 0), (1, 1, 5)]
    assert c["refs"] == [(1, 0, 20, 3, 1)]


def test_running_maximum():
    # a 100 kb skip, then short records inside its span: they add no window; the one behind its end adds its own
    r = [rec(0, 1000, 100_000, 0, 1), rec(0, 20_000, 50, 1, 2), rec(0, 90_000, 50, 2, 3), rec(0, 101_000, 20_000, 3, 4)]
    c = bm.per_call(r)
    assert c["linear"] == [(0, w, 0) for w in range(0, 7)] + [(0, 7, 3)]


def test_unmapped_tail_and_gap_references():
    r = [rec(0, 5, 10, 0, 1), rec(3, 5, 10, 1, 2), rec(-1, -1, 0, 2, 3, flag=4), rec(-1, -1, 0, 3, 4, flag=4)]
    c = bm.per_call(r)
    assert c["refs"] == [(0, 0, 1, 1, 0), (3, 1, 2, 1, 0), (-1, 2, 4, 0, 2)]
    bai = bm.read_bai(bm.build(5, r))
    assert bai["n_no_coor"] == 2
    assert [x["meta"] is None for x in bai["refs"]] == [False, True, True, False, True]
    assert bai["refs"][1] == dict(bins={}, meta=None, ioffset=[])
    assert bai["refs"][3]["meta"] == (1, 2, 1, 0)


def test_limit_of_bai():
    ok = [rec(0, (1 << 29) - 10, 10, 0, 1)]
    assert bm.per_call(ok)["chunks"][0][1] == 4681 + 32767
    with pytest.raises(bm.IndexError_) as e:
        bm.per_call(ok + [rec(0, (1 << 29) - 10, 11, 1, 2)], first_index=7)
    assert (e.value.kind, e.value.record) == ("span", 8)
    # without a reference the span does not count
    bm.per_call([rec(-1, (1 << 29), 100, 0, 1)])


def test_order():
    r = [rec(0, 10, 5, 0, 1), rec(0, 9, 5, 1, 2), rec(0, 8, 5, 2, 3)]
    with pytest.raises(bm.IndexError_) as e:
        bm.per_call(r)
    assert (e.value.kind, e.value.record) == ("order", 1)
    # refID -1 sorts last; equal keys are fine
    bm.per_call([rec(0, 10, 5, 0, 1), rec(0, 10, 5, 1, 2), rec(-1, -1, 0, 2, 3)])
    with pytest.raises(bm.IndexError_):
        bm.per_call([rec(-1, -1, 0, 0, 1), rec(0, 10, 5, 1, 2)])
    # between calls: the host's check
    b = bm.Builder(1)
    b.add(0, bm.per_call(r[:1]))
    with pytest.raises(bm.IndexError_) as e:
        b.add(0, bm.per_call(r[1:2]))
    assert (e.value.kind, e.value.record) == ("order", 1)


def test_same_block_merge_and_backfill():
    # records of 100 bytes in blocks of 0x1000: bins alternate, so every record is a chunk; chunks of one bin merge while the
    # next begins in the block the previous ends in
    specs = []
    for k in range(120):
        specs.append((0, 40_000 + k, 10) if k % 2 == 0 else (0, 40_000 + k, 20_000))
    recs = laid_out(specs)
    bai = bm.read_bai(bm.build(1, recs))
    ref = bai["refs"][0]
    small = ref["bins"][4681 + 2]
    # (byte 4096 lies inside record 40, of this bin: it ends in the block record 42 begins in, so nothing breaks there; byte
    # 8192 lies inside record 81, of the other bin: record 80 ends in block 1, record 82 begins in block 2)
    assert small == [(recs[0]["u"], recs[80]["v"]), (recs[82]["u"], recs[118]["v"])]
    assert small[0][1] >> 16 < small[1][0] >> 16
    # windows 0 and 1 hold no record: they take window 2's value
    assert ref["ioffset"][:3] == [recs[0]["u"]] * 3
    assert ref["ioffset"][3] == recs[1]["u"]
    assert ref["meta"] == (recs[0]["u"], recs[-1]["v"], 120, 0)


def test_calls_compose():
    rng = random.Random(5)
    specs, pos = [], 0
    for tid in (0, 2):
        pos = 0
        for _ in range(300):
            pos += rng.randrange(0, 400)
            specs.append((tid, pos, rng.choice([1, 50, 150, 30_000]), 4 if rng.random() < 0.05 else 0))
    specs += [(-1, -1, 0, 4)] * 7
    recs = laid_out(specs)
    whole = bm.build(3, recs)
    for _ in range(20):
        cuts = sorted(rng.sample(range(len(recs) + 1), 5)) + [len(recs)]
        b, at = bm.Builder(3), 0
        for c in cuts + [len(recs)]:  # (the last call is empty)
            b.add(0, bm.per_call(recs[at:c], first_index=at))
            at = c
        assert b.finish() == whole


def test_round_trip_layout():
    recs = laid_out([(0, 100, 50), (0, 200, 50, 4), (1, 5, 70_000), (-1, -1, 0, 4)])
    data = bm.build(2, recs)
    bai = bm.read_bai(data)
    assert data[:8] == b"BAI\1" + struct.pack("<i", 2)
    assert bai["refs"][0]["bins"] == {4681: [(recs[0]["u"], recs[1]["v"])]}
    assert bai["refs"][0]["meta"] == (recs[0]["u"], recs[1]["v"], 1, 1)
    assert bai["refs"][0]["ioffset"] == [recs[0]["u"]]
    assert bai["refs"][1]["bins"] == {bm.reg2bin(5, 70_005): [(recs[2]["u"], recs[2]["v"])]}
    assert bai["refs"][1]["ioffset"] == [recs[2]["u"]] * 5
    assert bai["n_no_coor"] == 1


def brute(recs, tid, beg, end):
    return [i for i, r in enumerate(recs) if r["tid"] == tid and not r["flag"] & 4 and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg]


def found(bai, recs, tid, beg, end):
    """What a reader gets: it scans the chunks query() names and keeps the mapped records that overlap."""
    hit = set()
    for cb, ce in bm.query(bai, tid, beg, end):
        for i, r in enumerate(recs):
            if cb <= r["u"] < ce and r["tid"] == tid and not r["flag"] & 4 and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg:
                hit.add(i)
    return sorted(hit)


@pytest.mark.parametrize("seed", range(6))
def test_query_finds_what_brute_force_finds(seed):
    rng = random.Random(seed)
    specs = []
    for tid in range(3):
        pos = rng.choice([0, 16_000, 130_000])
        for _ in range(rng.choice([0, 40, 400]) if tid else 400):
            pos += rng.choice([0, 1, 30, 700, 9_000])
            specs.append((tid, pos, rng.choice([0, 1, 100, 100, 5_000, 140_000]), 4 if rng.random() < 0.04 else 0))
    recs = laid_out(specs, size=rng.choice([40, 333]), block=rng.choice([0x400, 0x7f00]))
    bai = bm.read_bai(bm.build(3, recs))
    top = max(bm.span_of(r)[1] for r in recs) + 20_000
    for _ in range(150):
        tid = rng.randrange(3)
        beg = rng.randrange(top)
        end = beg + rng.choice([1, 10, 1000, 16384, 300_000])
        assert found(bai, recs, tid, beg, end) == brute(recs, tid, beg, end), (tid, beg, end)
