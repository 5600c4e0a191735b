"""fadehip_index_batch (Context.index_batch): the kernels of bam_index.hpp — the ones the file path runs under
FADEHIP_BAM_INDEX — held to tests/bai_model.py on one batch of designed records, at virtual offsets the test brings, with no
codec in between.  About 5,000 records, so the scans cross many tiles of 256."""
import numpy as np
import pytest

import fade_amd
import bai_model as bm
import clip_cases as cc

pytestmark = pytest.mark.gpu

TILE = 256
N_REF = 8
BLOCK = 0x7f00


def _rec(k, tid, pos, cigar, flag=0):
    return cc.build_rec("q%d" % k, tid, pos, 30 if tid >= 0 else 0, flag, -1, -1, 0, cigar, "*", "*", b"NMC\x01" if k % 3 == 0 else b"")


def _design():
    """[(tid, pos, cigar, flag)] in coordinate order, and the places the edges hang on."""
    rng = np.random.RandomState(11)
    s, marks = [], {}

    def add(tid, pos, cigar, flag=0):
        s.append((tid, pos, cigar, flag))
        return len(s) - 1

    # reference 0: the edges of the span rule
    marks["neg"] = add(0, -1, "10M")                 # pos -1 with a reference: begins at 0, key 0
    add(0, 0, "*")                                   # reflen 0 counts as 1
    add(0, 5, "20M", 4)                              # flag 4 with a reference: a chunk, no window
    add(0, 5, "10M5I10M")
    for shift in (14, 17, 20, 23, 26):               # both sides of every level boundary of reg2bin
        b = 1 << shift
        add(0, b - 10, "10M")                        # ends exactly on it
        add(0, b - 10, "11M")                        # crosses it by one base
        add(0, b - 1, "1M1D")                        # its last base and the first behind it
        add(0, b, "10M")                             # begins on it
        if shift == 17:
            # a 100 kb skip, then short records inside its span: the running maximum keeps their windows from counting again
            marks["skip"] = add(0, b + 100, "10M100000N10M")
            for d in (200, 16_000, 20_000, 50_000, 99_000):
                add(0, b + d, "30M")
            add(0, b + 100_100, "50M")               # begins in the skip's last window, reaches one more with 20 kb
            add(0, b + 100_200, "20000M")
    marks["limit"] = add(0, (1 << 29) - 100, "100M")  # end = 2^29 exactly: the last bin, the last window
    while len(s) < 2 * TILE:                         # (fill so that reference 1 begins on a tile's first record)
        add(0, (1 << 29) - 1, "1M")
    # reference 1 begins at a tile's first record and is one (refID, bin) run longer than two tiles ...
    marks["ref1"] = len(s)
    for k in range(3 * TILE - 1):
        add(1, 1000 + k // 2, "40M", 4 if k % 50 == 7 else 0)
    # ... so that reference 3 begins at a tile's last record; 2, 4 and 5 have none
    marks["ref3"] = len(s)
    pos = 0
    for k in range(700):
        pos += int(rng.choice([0, 1, 7, 300, 9000]))
        add(3, pos, str(rng.choice(["1M", "60M", "100M", "30M2000N30M", "*", "17000M"])), 4 if rng.rand() < 0.03 else 0)
    marks["ref6"] = len(s)
    pos = 100_000
    for k in range(3000):
        pos += int(rng.choice([0, 0, 2, 40, 5000, 40_000]))
        add(6, pos, str(rng.choice(["75M", "75M", "20S55M", "40M70000N35M", "10M1D10M"])), 4 if rng.rand() < 0.02 else 0)
    marks["tail"] = len(s)
    add(-1, -1, "*", 0)                              # no reference, flag 4 clear: counted as mapped of the -1 run, nothing else
    for k in range(40):
        add(-1, -1, "*", 4)
    return s, marks


SPECS, MARKS = _design()
assert MARKS["ref1"] % TILE == 0 and MARKS["ref3"] % TILE == TILE - 1


def _batch(specs):
    recs = [_rec(k, *sp) for k, sp in enumerate(specs)]
    off = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    total = int(off[-1])
    nb = (total + BLOCK - 1) // BLOCK
    coff = [1000 + 12_345 * k for k in range(nb)]
    voff = np.array([bm.virtual_offset(int(p), BLOCK, coff, total, 1000 + 12_345 * nb) for p in off], np.uint64)
    cat = np.frombuffer(b"".join(recs), np.uint8) if recs else np.zeros(0, np.uint8)
    return cat, off, voff


def _model(cat, voff):
    recs = bm.parse_records(cat.tobytes())
    for r, u, v in zip(recs, voff[:-1], voff[1:]):
        r["u"], r["v"] = int(u), int(v)
    return recs


@pytest.fixture(scope="module")
def designed(ctx):
    cat, off, voff = _batch(SPECS)
    return ctx.index_batch(cat, off, voff), bm.per_call(_model(cat, voff)), _model(cat, voff)


def test_counts_and_keys(designed):
    got, want, recs = designed
    assert len(recs) >= 5000
    assert (got["n"], got["first_key"], got["last_key"]) == (want["n"], want["first_key"], want["last_key"])
    assert got["first_key"] == 0 and got["last_key"] == (0xffffffff << 32)


def test_reference_runs(designed):
    got, want, recs = designed
    assert got["refs"] == want["refs"]
    assert [r[0] for r in got["refs"]] == [0, 1, 3, 6, -1]
    assert got["refs"][-1][3:] == (1, 40)
    assert got["refs"][1][1] == recs[MARKS["ref1"]]["u"] and got["refs"][1][2] == recs[MARKS["ref3"]]["u"]


def test_chunks(designed):
    got, want, recs = designed
    assert got["chunks"] == want["chunks"]
    # reference 1 is one run over three tiles; the record that ends on 2^29 sits in the last bin
    assert [c for c in got["chunks"] if c[0] == 1] == [(1, 4681, recs[MARKS["ref1"]]["u"], recs[MARKS["ref3"]]["u"])]
    assert (0, 4681 + 32767, recs[MARKS["limit"]]["u"], recs[MARKS["ref1"]]["u"]) in got["chunks"]


def test_linear_entries(designed):
    got, want, recs = designed
    assert got["linear"] == want["linear"]
    b = 1 << 17
    skip = recs[MARKS["skip"]]["u"]
    mine = [(w, o) for t, w, o in got["linear"] if t == 0 and (b + 100) >> 14 <= w <= (b + 100_119) >> 14]
    # the skip's windows carry the skip's offset: window 8 the record's in front, the short ones inside add none
    assert [o for w, o in mine if w > 8] == [skip] * 6
    assert (0, 32767, recs[MARKS["limit"]]["u"]) in got["linear"]


def test_assembled_file(designed):
    got, want, recs = designed
    b = fade_amd.BaiBuilder(N_REF)
    try:
        b.add(0, got)
        data = b.finish()
    finally:
        b.close()
    assert data == bm.build(N_REF, recs)
    bai = bm.read_bai(data)
    assert bai["n_no_coor"] == 41
    assert [r["meta"] is None for r in bai["refs"]] == [False, False, True, False, True, True, False, True]


def test_none_and_one(ctx):
    cat, off, voff = _batch([])
    got = ctx.index_batch(cat, off, voff)
    assert got == dict(chunks=[], linear=[], refs=[], n=0, first_key=0, last_key=0)
    cat, off, voff = _batch([(2, 40_000, "10M20000N10M")])
    got = ctx.index_batch(cat, off, voff)
    assert got == bm.per_call(_model(cat, voff))
    assert got["chunks"] == [(2, 585, int(voff[0]), int(voff[1]))] and [w for _, w, _ in got["linear"]] == [2, 3]


def test_beyond_the_limit_names_the_record(ctx):
    specs = list(SPECS)
    k = MARKS["limit"]
    specs[k] = (0, (1 << 29) - 100, "101M", 0)
    cat, off, voff = _batch(specs)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.index_batch(cat, off, voff)
    assert e.value.code == -5 and "record %d:" % k in str(e.value)
    with pytest.raises(bm.IndexError_) as m:
        bm.per_call(_model(cat, voff))
    assert (m.value.kind, m.value.record) == ("span", k)


def test_keys_that_step_back_name_the_record(ctx):
    specs = list(SPECS)
    k = MARKS["ref6"] + 1500
    assert specs[k][1] < specs[k + 400][1]
    specs[k] = specs[k + 400]           # one record too far ahead: the one behind it steps back
    cat, off, voff = _batch(specs)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.index_batch(cat, off, voff)
    assert e.value.code == -1
    assert "record %d: not in coordinate order (--write-index needs coordinate-sorted output)" % (k + 1) in str(e.value)
    with pytest.raises(bm.IndexError_) as m:
        bm.per_call(_model(cat, voff))
    assert (m.value.kind, m.value.record) == ("order", k + 1)


def test_null_arguments(ctx):
    import ctypes as C
    from fade_amd import _lib
    L = _lib.load()
    c = _lib.IndexCall()
    off = np.zeros(1, np.int64)
    assert L.fadehip_index_batch(ctx._h, 0, None, off.ctypes.data, None, C.byref(c)) == -1
    assert b"NULL" in L.fadehip_last_error(ctx._h)
    assert L.fadehip_index_batch(ctx._h, 0, None, None, off.ctypes.data, C.byref(c)) == -1
    assert L.fadehip_index_batch(ctx._h, 0, None, off.ctypes.data, off.ctypes.data, None) == -1
    assert L.fadehip_index_batch(None, 0, None, off.ctypes.data, off.ctypes.data, C.byref(c)) == -1
