"""A CSI geometry on the file path and on the record store (BamStream.index_geometry, RecStore.index_geometry,
fade_amd.CsiBuilder): the entries of the records a from-tags stream writes, or a store drains, under (14, 6) — positions beyond
2^29 among them — held call by call to tests/csi_model.py; the payload the host builder makes of them held to the model's
over the file's own records; and the written .csi bytes read back (tests/bai_reader.py walks the members) and queried against
brute force over the real output bytes."""
import random
import struct
import zlib

import pytest

import fade_amd
import bai_model as bm
import bai_reader as br
import csi_model as cm
import test_gpu_bam_index as bi
import test_gpu_keep_sorted as ks
from test_gpu_bgzf import EOF_MARK

pytestmark = pytest.mark.gpu

NAMES = ["big", "c1", "c2", "c3"]
GEO = (14, 6)


def _header(names):
    """One BGZF member with a BAM header of those references (what the driver writes in front of the first call)."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    p = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(names))
    for n in names:
        p += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", 0x7fffffff)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(p) + c.flush()
    return b"\x1f\x8b\x08\x04" + bytes(6) + b"\x06\x00BC\x02\x00" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(p), len(p))


def _records():
    """About 700 sorted records and the byte cuts of three calls: the first cut inside a (refID, bin) run, the second where
    reference 2 begins."""
    rng = random.Random(17)
    recs, at, cuts = [], 0, []

    def add(*a, **kw):
        nonlocal at
        recs.append(bi._rec(len(recs), *a, **kw))
        at += len(recs[-1])

    pos = 100
    for k in range(260):
        pos += 3
        add(0, pos)
        if k == 150:
            cuts.append(at)                               # (every record so far, and the next hundred, lie in leaf 0)
    for j in range(200):
        pos += rng.choice([0, 2, 90, 1500, 7000, 400_000])
        add(0, pos, cigar=rng.choice(["50M", "50M", "20M30000N30M", "25M1D25M", "10S40M", "*"]), flag=4 if j % 40 == 9 else 0)
    assert pos < (1 << 29) - 100_000
    add(0, (1 << 29) - 10, cigar="20M30S")                # 20 reference bases across 2^29
    add(0, 1 << 29)
    for j in range(40):
        add(0, (1 << 29) + 5 + 1000 * j, cigar=rng.choice(["50M", "25M70000N25M"]))
    add(0, (1 << 30) + 77)
    add(0, (1 << 30) + 77, cigar="25M%dN25M" % ((1 << 28) - 1))
    add(0, (1 << 31) - 2, cigar="1M49S")                  # one base, the last but one position a BAM record can name
    add(0, (1 << 31) - 2, flag=4)
    cuts.append(at)
    pos = (1 << 20) - 2000
    for j in range(200):
        pos += rng.choice([0, 5, 40, 400])
        add(2, pos, cigar=rng.choice(["50M", "50M", "50M", "20M100000N30M"]))
    for _ in range(7):
        add(-1, -1, cigar="*", flag=4)
    return recs, cuts


def _run(ctx, names, payload, cuts, geometry, index=True, **modes):
    """The payload through a FROM_TAGS stream cut at `cuts`: per call the members and, with index, the index entries."""
    st = ctx.bam_stream(names, floor_len=-3, window=-1, from_tags=True, index=index, **modes)
    try:
        if geometry:
            st.index_geometry(*geometry)
        edges = [0] + list(cuts) + ([len(payload)] if not cuts or cuts[-1] != len(payload) else [])
        pieces, calls = [], []
        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(payload[a:b], last=(j == len(edges) - 2))
            pieces.append(st.back())
            if index:
                calls.append(st.back_index())
        return pieces, calls
    finally:
        st.close()


def _check_queries(data, csi, recs, n_ref, seed=1):
    """Every region: what the index finds in the file's real bytes is exactly what brute force finds."""
    rng = random.Random(seed)
    mapped = [r for r in recs if r["tid"] >= 0 and not r["flag"] & 4]
    regions = set()
    for r in rng.sample(mapped, min(len(mapped), 80)):
        beg, end = bm.span_of(r)
        regions |= {(r["tid"], beg, beg + 1), (r["tid"], end - 1, end), (r["tid"], end, end + 1), (r["tid"], max(beg - 1, 0), beg)}
    for tid in range(n_ref):
        for shift in (14, 17, 20, 23, 26, 29):
            b = 1 << shift
            regions |= {(tid, b - 1, b), (tid, b, b + 1), (tid, b - 1, b + 1), (tid, 0, b)}
        regions |= {(tid, 0, 1 << 32), (tid, (1 << 29) - 10, (1 << 29) + 10), (tid, 1 << 29, (1 << 29) + 1), (tid, (1 << 30) + 77, (1 << 30) + 78),
                    (tid, (1 << 31) - 2, (1 << 31) - 1), (tid, (1 << 31) - 1, 1 << 31), (tid, (1 << 30) + (1 << 28), (1 << 30) + (1 << 28) + 5)}
    top = max(bm.span_of(r)[1] for r in mapped) + 40_000
    for _ in range(200):
        beg = rng.randrange(top) if rng.random() < 0.5 else rng.randrange(1 << 21)
        regions.add((rng.randrange(n_ref), beg, beg + rng.choice([1, 50, 3000, 16384, 200_000])))
    rd = br.Reader(data)
    n_hits = 0
    for tid, beg, end in sorted(regions):
        want = sorted(r["u"] for r in mapped if r["tid"] == tid and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg)
        got = set()
        for cb, ce in cm.query(csi, tid, beg, end):
            for u, t, pos, flag, reflen in rd.records(cb, ce):
                r = dict(tid=t, pos=pos, flag=flag, reflen=reflen)
                if t == tid and not flag & 4 and bm.span_of(r)[0] < end and bm.span_of(r)[1] > beg:
                    got.add(u)
        assert sorted(got) == want, (tid, beg, end, len(got), len(want))
        n_hits += len(want)
    assert n_hits > 0
    return n_hits


def _check_run(names, pieces, calls, geometry):
    """Per call the model's entries; the builder's payload the model's over the file's own records; the file's bytes read back."""
    header = _header(names)
    data = header + b"".join(pieces) + EOF_MARK
    b = fade_amd.CsiBuilder(len(names), *geometry)
    try:
        base = len(header)
        for k, (piece, got) in enumerate(zip(pieces, calls)):
            lay = br.Layout(br.walk_members(piece), len(piece))          # offsets relative to the call's first member
            assert got == cm.per_call(br.records_of(lay), *geometry), k
            b.add(base, got)
            base += len(piece)
        payload, written = b.finish(), b.file_bytes()
    finally:
        b.close()
    n_ref, recs = br.bam_records(data)
    assert n_ref == len(names) and payload == cm.build(n_ref, recs, *geometry)
    mem = br.walk_members(written)                                       # (inflates with zlib, checks ISIZE)
    assert written.endswith(EOF_MARK) and mem[-1][1] == b"" and all(0 < len(p) <= 0xff00 for _, p in mem[:-1])
    assert b"".join(p for _, p in mem) == payload
    csi = cm.read_csi(b"".join(p for _, p in mem))
    assert (csi["min_shift"], csi["depth"]) == geometry
    _check_queries(data, csi, recs, n_ref)
    return recs, csi


@pytest.mark.parametrize("stored", [True, False])
def test_csi_of_a_stream(ctx, stored):
    recs, cuts = _records()
    assert 650 <= len(recs) <= 760
    payload = b"".join(recs)
    pieces, calls = _run(ctx, NAMES, payload, cuts, GEO, stored=stored)
    assert b"".join(b"".join(p for _, p in br.walk_members(x)) for x in pieces) == payload
    assert [c["n"] for c in calls] == [len(f) for f in bi._calls_of(recs, cuts)] and len(calls) == 3
    # a (refID, bin) run lies across the first cut: both calls have a chunk of leaf 0 that abut; the third call begins reference 2
    leaf = cm.first_bin(6)
    assert calls[0]["chunks"][-1][:2] == (0, leaf) == calls[1]["chunks"][0][:2]
    assert calls[0]["chunks"][-1][3] == len(pieces[0]) << 16 and calls[1]["chunks"][0][2] == 0
    assert calls[2]["refs"][0][0] == 2 and calls[1]["refs"][-1][0] == 0
    allr, csi = _check_run(NAMES, pieces, calls, GEO)
    assert len(allr) == len(recs) and csi["n_no_coor"] == 7
    assert csi["refs"][1]["meta"] is None and csi["refs"][3]["meta"] is None
    bins = csi["refs"][0]["bins"]
    assert leaf + (1 << 15) in bins and leaf + (((1 << 31) - 2) >> 14) in bins and max(bins) < 299594
    assert len(bins[leaf][1]) == 1                                        # the run across the cut is one chunk of the file


def test_a_stream_without_the_geometry_call_gives_todays_entries(ctx):
    recs, cuts = _records()
    small = [r for r in recs if struct.unpack_from("<i", r, 8)[0] < (1 << 29) - 100]
    payload = b"".join(small)
    pieces, calls = _run(ctx, NAMES, payload, [len(payload) // 2], None, stored=True)
    with_14_5, calls_14_5 = _run(ctx, NAMES, payload, [len(payload) // 2], (14, 5), stored=True)
    assert pieces == with_14_5 and calls == calls_14_5                   # (14, 5) is BAI's tree
    for piece, got in zip(pieces, calls):
        assert got == bm.per_call(br.records_of(br.Layout(br.walk_members(piece), len(piece))))
    # the large positions: 2^29 is where it ends without the call, with today's message
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        st.front_raw(b"".join(recs), last=True)
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        k = next(i for i, r in enumerate(recs) if struct.unpack_from("<i", r, 8)[0] == (1 << 29) - 10)
        assert e.value.code == -5 and "record %d: ends beyond 2^29 on its reference (a BAI index cannot hold it)" % k in str(e.value)
    finally:
        st.close()


def test_clipped_records_in_their_final_order(ctx):
    recs = bi._clip_payload()
    payload = b"".join(recs)
    ends = ks._offsets(payload)[1:]
    cuts = [ends[250], ends[690], len(payload)]
    plain, _ = _run(ctx, ks.NAMES, payload, cuts, None, index=False, stored=True, clip=True, keep_sorted=True)
    pieces, calls = _run(ctx, ks.NAMES, payload, cuts, GEO, stored=True, clip=True, keep_sorted=True)
    assert pieces == plain
    allr, csi = _check_run(ks.NAMES, pieces, calls, GEO)
    assert len(allr) == len(recs) and csi["n_no_coor"] == 20
    assert sum(1 for r, src in zip(allr, recs) if r["pos"] != struct.unpack_from("<i", src, 8)[0]) > 50


def test_more_new_windows_in_a_call_than_its_first_room(ctx):
    """(4, 2): 1,100 references with one record over all 64 windows leave 70,400 linear entries in one call, more than the
    records + 65536 the call's arrays start with: the write kernel runs again into a block that holds them all."""
    names = ["r%d" % k for k in range(1100)]
    recs = [bi._rec(k, k, 0, cigar="25M974N25M") for k in range(1100)]
    pieces, calls = _run(ctx, names, b"".join(recs), [], (4, 2), stored=True)
    want = cm.per_call(br.records_of(br.Layout(br.walk_members(pieces[0]), len(pieces[0]))), 4, 2)
    assert len(want["linear"]) == 70_400 > len(recs) + 65536
    assert calls[0] == want
    # ... and one base more is beyond the limit, at the call's back
    recs[700] = bi._rec(700, 700, 1, cigar="25M974N25M")
    st = ctx.bam_stream(names, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        st.index_geometry(4, 2)
        st.front_raw(b"".join(recs), last=True)
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        assert e.value.code == -5 and "record 700:" in str(e.value) and "2^10" in str(e.value) and "CSI" in str(e.value)
    finally:
        st.close()


def test_when_and_where_the_geometry_call_is_taken(ctx):
    recs, _ = _records()
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        for geometry in [(3, 2), (14, 0), (14, 9), (14, 7), (30, 1)]:
            with pytest.raises(fade_amd.FadeHipError) as e:
                st.index_geometry(*geometry)
            assert e.value.code == -1 and "min_shift" in str(e.value)
        st.index_geometry(14, 5)
        st.index_geometry(14, 6)                       # (before the first front call it may be said again)
        st.front_raw(b"".join(recs[:10]), last=True)
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.index_geometry(14, 6)
        assert e.value.code == -6 and "before the first front call" in str(e.value)
        st.back()
        assert st.back_index()["chunks"][0][1] == cm.first_bin(6)
    finally:
        st.close()
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.index_geometry(14, 6)
        assert e.value.code == -1 and "FADEHIP_BAM_INDEX" in str(e.value)
    finally:
        st.close()


def test_drains_of_a_store_under_the_geometry(ctx):
    recs, _ = _records()
    shuffled = list(recs)
    random.Random(5).shuffle(shuffled)
    s = ctx.recstore()
    try:
        s.add_batch(shuffled[:300])
        s.add_batch(shuffled[300:])
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.index_geometry(14, 7)
        assert e.value.code == -1
        s.index_geometry(*GEO)
        s.sort()
        pieces, calls = [], []
        while True:
            out, n, idx = s.drain(5 * len(recs[0]), stored=len(pieces) % 2 == 0, index=True)   # a few records each
            if not n:
                break
            pieces.append(out)
            calls.append(idx)
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.index_geometry(14, 5)
        assert e.value.code == -6 and "before the first drain" in str(e.value)
    finally:
        s.close()
    assert len(pieces) > 100 and sum(c["n"] for c in calls) == len(recs)
    allr, csi = _check_run(NAMES, pieces, calls, GEO)
    assert len(allr) == len(recs) and csi["n_no_coor"] == 7
    # without the call the store's drains end at 2^29, with today's message
    s = ctx.recstore()
    try:
        s.add_batch(recs)
        s.sort()
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.drain(1 << 30, stored=True, index=True)
        assert e.value.code == -5 and "ends beyond 2^29 on its reference (a BAI index cannot hold it)" in str(e.value)
    finally:
        s.close()
