"""FADEHIP_BAM_INDEX on the file path (Context.bam_stream(..., index=True), BamStream.back_index(), fade_amd.BaiBuilder): the
.bai of the records a stream writes, made in the pass that writes them.  Streams run with from_tags=True and front_raw, so no
genome and no aligner run; stored and compressed members, both block geometries pinned.  The test derives every record's
virtual offsets itself (tests/bai_reader.py walks the output's members with zlib and the BC subfield), holds every call's
entries and the assembled file to tests/bai_model.py, and reads the real output bytes back through the written index."""
import struct
import zlib

import pytest

import fade_amd
import bai_model as bm
import bai_reader as br
import clip_cases as cc
import test_gpu_keep_sorted as ks
from test_gpu_bgzf import EOF_MARK

pytestmark = pytest.mark.gpu

NAMES = ["c0", "c1", "c2", "c3"]
BIG_BASES = 50_000   # a record of 36 + name + 25,000 + 50,000 bytes: longer than two blocks of 0x7f00 and than one of 0xff00


def _rec(k, tid, pos, cigar="50M", flag=0, rs=0, size=None, bases=50):
    """Record k with an integer rs; size: its bytes exactly (a padding tag takes up the difference)."""
    def make(pad):
        aux = b"rsC" + bytes([rs]) + (b"XPZ" + b"x" * pad + b"\0" if pad is not None else b"")
        seq = "ACGT" * (bases // 4) + "ACGT"[:bases % 4]
        return cc.build_rec("r%05d" % k, tid, pos, 30 if tid >= 0 else 0, flag, -1, -1, 0, cigar, seq, "5" * bases, aux)
    if size is None:
        return make(None)
    r = make(size - len(make(0)))
    assert len(r) == size
    return r


def _build(block, eject_some=False):
    """(records, cuts, marks) for blocks of `block` bytes: call 0 carries the records placed against the block grid."""
    recs, marks = [], {}
    at = 0

    def add(*a, **kw):
        nonlocal at
        if eject_some and len(recs) % 7 == 3:
            kw.setdefault("rs", 2)
        recs.append(_rec(len(recs), *a, **kw))
        at += len(recs[-1])
        return len(recs) - 1

    pos = 10
    while block - at > 500:
        pos += 3
        add(0, pos)
    marks["ends_on"] = add(0, pos + 1, size=block - at)          # ends exactly on the first block boundary
    assert at == block
    marks["starts_on"] = add(0, pos + 2)                          # starts exactly on it
    pos += 2
    while 2 * block - at > 4000:
        pos += 3
        add(0, pos)
    marks["big"] = add(0, pos + 1, cigar="%dM" % BIG_BASES, bases=BIG_BASES)   # from block 1 into block 3 or beyond
    marks["big_at"] = at - len(recs[-1])
    pos += 1
    for _ in range(200):
        pos += 3
        add(0, pos)
    cut0 = at                                                     # inside a (refID, bin) run: everything so far lies in bin 4681
    marks["call1"] = len(recs)
    for _ in range(200):
        pos += 3
        add(0, pos)
    assert pos + 50 < 16384
    import random
    rng = random.Random(3)
    for j in range(500):
        pos += rng.choice([0, 2, 90, 1500, 7000])
        add(0, pos, cigar=rng.choice(["50M", "50M", "20M30000N30M", "25M1D25M", "10S40M", "*"]), flag=4 if j % 40 == 9 else 0)
    cut1 = at
    marks["single"] = add(0, pos + 10)                            # a call of one record
    cut2 = at
    marks["call4"] = len(recs)
    pos = (1 << 20) - 2000                                        # reference 2 (1 has no record): across a level boundary
    for j in range(400):
        pos += rng.choice([0, 5, 40, 400])
        add(2, pos, cigar=rng.choice(["50M", "50M", "50M", "20M100000N30M"]))
    add(2, pos, flag=4)
    for _ in range(25):
        add(-1, -1, cigar="*", flag=4)
    cut3 = cut2 + len(recs[marks["call4"]]) // 2                  # call 3 brings half a record: its output is empty
    return recs, [cut0, cut1, cut2, cut3, at], marks


def _calls_of(recs, cuts):
    """Which records every call frames: a record belongs to the call that brings its last byte."""
    ends, at = [], 0
    for r in recs:
        at += len(r)
        ends.append(at)
    calls, k = [], 0
    for e in list(cuts) + ([] if cuts and cuts[-1] == at else [at]):
        n = 0
        while k + n < len(ends) and ends[k + n] <= e:
            n += 1
        calls.append(list(range(k, k + n)))
        k += n
    if cuts and cuts[-1] == at:
        calls.append([])   # (a cut at the payload's end: an empty last call)
    return calls


def _run(ctx, names, payload, cuts, depth=1, **modes):
    """The payload through a FROM_TAGS stream cut at `cuts` (the last may be len(payload): an empty last call), at most `depth`
    calls between front and back: per call the members and, with index=True, the index entries."""
    st = ctx.bam_stream(names, floor_len=-3, window=-1, from_tags=True, **modes)
    try:
        edges = [0] + sorted(cuts)
        if edges[-1] != len(payload):
            edges.append(len(payload))
        pieces, calls, done = [], [], 0

        def back():
            pieces.append(st.back())
            if modes.get("index"):
                calls.append(st.back_index())

        n_calls = len(edges) - 1 + (1 if cuts and sorted(cuts)[-1] == len(payload) else 0)
        spans = list(zip(edges, edges[1:])) + ([(len(payload), len(payload))] if n_calls > len(edges) - 1 else [])
        for j, (a, b) in enumerate(spans):
            st.front_raw(payload[a:b], last=(j == len(spans) - 1))
            if j + 1 - done >= depth:
                back()
                done += 1
        while done < len(spans):
            back()
            done += 1
        return pieces, calls
    finally:
        st.close()


def _header_member():
    p = b"BAM\1 a stand-in for the header members the driver writes in front of the first call" * 9
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(p) + c.flush()
    return b"\x1f\x8b\x08\x04" + bytes(6) + b"\x06\x00BC\x02\x00" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(p), len(p)), len(p)


def _check_run(pieces, calls, n_ref):
    """Steps 1 to 4 of the check for one run; returns (the file's records, the per-call records, the .bai)."""
    header, header_len = _header_member()
    data = header + b"".join(pieces) + EOF_MARK
    per_call = []
    b = fade_amd.BaiBuilder(n_ref)
    try:
        base = len(header)
        for piece, got in zip(pieces, calls):
            lay = br.Layout(br.walk_members(piece), len(piece))     # 1. offsets relative to the call's first member
            recs = br.records_of(lay)
            per_call.append(recs)
            assert got == bm.per_call(recs), len(per_call) - 1     # 2. the call's entries are the model's
            b.add(base, got)
            base += len(piece)
        bai = b.finish()
    finally:
        b.close()
    lay = br.Layout(br.walk_members(data), len(data))
    recs = br.records_of(lay, header_len)
    assert [r["u"] for r in recs] == [r["u"] + (bs << 16) for rc, bs in zip(per_call, _bases(len(header), pieces)) for r in rc]
    assert bai == bm.build(n_ref, recs)                              # 3. the assembled file is the model's, byte for byte
    br.check_queries(data, bai, recs, n_ref)                         # 4. the index finds what brute force finds
    return recs, per_call, bai


def _bases(first, pieces):
    out, at = [], first
    for p in pieces:
        out.append(at)
        at += len(p)
    return out


@pytest.fixture(scope="module", params=["stored", 64, 32])
def lane(request, ctx):
    """(context, stored?, block bytes): stored members on the shared context, each compressor geometry on one pinned to it"""
    if request.param == "stored":
        yield ctx, True, 0xff00
        return
    mp = pytest.MonkeyPatch()
    mp.setenv("FADEHIP_BGZF_GEOM", str(request.param))  # (read when a context compresses for the first time)
    c = fade_amd.Context(device=0)
    try:
        c.bgzf_deflate(bytes(16))
        yield c, False, {64: 0xff00, 32: 0x7f00}[request.param]
    finally:
        c.close()
        mp.undo()


def test_index_of_a_stream(lane):
    c, stored, block = lane
    recs, cuts, marks = _build(block)
    payload = b"".join(recs)
    plain, _ = _run(c, NAMES, payload, cuts, stored=stored)
    pieces, calls = _run(c, NAMES, payload, cuts, stored=stored, index=True)
    assert pieces == plain                                           # the flag changes no output byte
    assert b"".join(b"".join(p for _, p in br.walk_members(x)) for x in pieces) == payload
    frames = _calls_of(recs, cuts)
    assert [len(f) for f in frames][1:4] == [len(frames[1]), 1, 0] and len(frames[5]) == 0
    assert [c_["n"] for c_ in calls] == [len(f) for f in frames]
    assert calls[3] == dict(chunks=[], linear=[], refs=[], n=0, first_key=0, last_key=0) and pieces[3] == b""
    # the geometry is the one the placement was made for
    mem0 = br.walk_members(pieces[0])
    assert [len(p) for _, p in mem0[:-1]] == [block] * (len(mem0) - 1)
    allr, per_call, bai = _check_run(pieces, calls, len(NAMES))
    offs = [o for o, _ in mem0]
    r = per_call[0]
    assert r[marks["ends_on"]]["v"] == offs[1] << 16 == r[marks["starts_on"]]["u"]
    big = r[marks["big"]]
    assert marks["big_at"] // block == 1 and offs.index(big["v"] >> 16) - offs.index(big["u"] >> 16) >= 2
    # a (refID, bin) run lies across the first cut: both calls have a chunk of bin 4681 that abut, and the file has one
    assert calls[0]["chunks"][-1][:2] == (0, 4681) == calls[1]["chunks"][0][:2]
    assert calls[0]["chunks"][-1][3] == per_call[0][-1]["v"] == len(pieces[0]) << 16 and calls[1]["chunks"][0][2] == 0
    parsed = bm.read_bai(bai)
    assert parsed["refs"][0]["bins"][4681][0][0] == allr[0]["u"]
    assert any(cb < allr[marks["call1"]]["u"] < ce for cb, ce in parsed["refs"][0]["bins"][4681])
    assert parsed["refs"][1]["meta"] is None and parsed["refs"][3]["meta"] is None and parsed["n_no_coor"] == 25


def test_two_calls_in_flight(lane):
    c, stored, block = lane
    recs, cuts, _ = _build(block)
    payload = b"".join(recs)
    pieces, calls = _run(c, NAMES, payload, cuts, depth=2, stored=stored, index=True)
    _check_run(pieces, calls, len(NAMES))


def test_ejected_records_are_not_indexed(ctx):
    recs, cuts, marks = _build(0xff00, eject_some=True)
    payload = b"".join(recs)
    plain, _ = _run(ctx, NAMES, payload, cuts, stored=True, eject="records")
    pieces, calls = _run(ctx, NAMES, payload, cuts, stored=True, eject="records", index=True)
    assert pieces == plain
    kept = [r for r in recs if r[r.index(b"rsC") + 3] == 0]
    assert 0 < len(kept) < len(recs) and sum(c["n"] for c in calls) == len(kept)
    allr, _, _ = _check_run(pieces, calls, len(NAMES))
    assert len(allr) == len(kept)


def _clip_payload(resets=()):
    """Coordinate-sorted records with rs / am tags as test_gpu_keep_sorted builds them: a fifth is clipped on the left (and
    moves up), on the right or on both sides, none by as much as its aligned length — except those in `resets`."""
    import random
    rng = random.Random(8)
    recs = []
    for tid, n in ((0, 700), (1, 300)):
        pos = 100
        for _ in range(n):
            pos += rng.randrange(0, 4)
            r = rng.random()
            left, right = (0, 0) if r < 0.8 else (rng.randrange(1, 45), 0) if r < 0.9 else (0, rng.randrange(1, 45)) if r < 0.95 else (rng.randrange(1, 25), rng.randrange(1, 25))
            if len(recs) in resets:
                left, right = 55, 0
            recs.append(ks._rec(len(recs), tid, pos, left, right))
    recs += [ks._rec(len(recs) + j, -1, -1, tags=False) for j in range(20)]
    return recs


def test_clipped_records_in_their_final_order(ctx):
    """clip=True, keep_sorted=True: the index describes the records as they leave — clipped, at their new positions, in the
    order the stage gives them, a tail held from call to call."""
    recs = _clip_payload()
    payload = b"".join(recs)
    ends = ks._offsets(payload)[1:]
    cuts = [ends[250], ends[251], ends[690], ends[705], len(payload)]
    plain, _ = _run(ctx, ks.NAMES, payload, cuts, stored=True, clip=True, keep_sorted=True)
    pieces, calls = _run(ctx, ks.NAMES, payload, cuts, stored=True, clip=True, keep_sorted=True, index=True)
    assert pieces == plain
    allr, per_call, bai = _check_run(pieces, calls, len(ks.NAMES))
    assert len(allr) == len(recs) and [len(c) for c in per_call] != [len(f) for f in _calls_of(recs, cuts)]   # (records were held)
    moved = sum(1 for r, src in zip(allr, recs) if r["pos"] != struct.unpack_from("<i", src, 8)[0])
    assert moved > 50 and bm.read_bai(bai)["n_no_coor"] == 20


def test_a_reset_record_breaks_the_order_as_written(ctx):
    """A clip that takes the whole alignment resets the record: its bytes say refID 0, pos 0, and KEEP_SORTED places it with the
    unmapped tail.  By the bytes that leave, the stream is then not in coordinate order, and the rule fails the call there."""
    recs = _clip_payload(resets={5})
    st = ctx.bam_stream(ks.NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, clip=True, keep_sorted=True, index=True)
    try:
        st.front_raw(b"".join(recs), last=True)
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        assert e.value.code == -1 and "record %d: not in coordinate order (--write-index" % (len(recs) - 21) in str(e.value)
    finally:
        st.close()


def test_output_out_of_order_fails_the_call(ctx):
    recs, cuts, marks = _build(0xff00)
    k = marks["call1"] + 50                       # within call 1: record k + 1 steps back behind the one moved ahead of it
    recs[k], recs[k + 30] = recs[k + 30], recs[k]
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        payload = b"".join(recs)
        st.front_raw(payload[:cuts[0]])
        assert st.back() and st.back_index()["n"] == marks["call1"]
        st.front_raw(payload[cuts[0]:cuts[1]])
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        assert e.value.code == -1
        assert "bam stream: record %d: not in coordinate order (--write-index needs coordinate-sorted output)" % (k + 1) in str(e.value)
    finally:
        st.close()


def test_keys_that_step_back_between_calls_fail_the_later_call(ctx):
    recs, cuts, marks = _build(0xff00)
    k = marks["call1"]                            # the last record of call 0 and the first of call 1 change places
    assert len(recs[k - 1]) == len(recs[k])
    recs[k - 1], recs[k] = recs[k], recs[k - 1]
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        payload = b"".join(recs)
        st.front_raw(payload[:cuts[0]])
        st.back()
        st.front_raw(payload[cuts[0]:cuts[1]])
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        assert e.value.code == -1 and "record %d: not in coordinate order (--write-index" % k in str(e.value)
    finally:
        st.close()


@pytest.mark.parametrize("modes, flag", [(dict(no_output=True), "FADEHIP_BAM_NO_OUTPUT"),
                                         (dict(no_output=True, report="stats"), "FADEHIP_BAM_"),
                                         (dict(no_output=True, report="clip"), "FADEHIP_BAM_"),
                                         (dict(collect_names=True), "FADEHIP_BAM_COLLECT_NAMES")])
def test_refused_combinations_name_the_flag(ctx, modes, flag):
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.bam_stream(NAMES, from_tags=True, index=True, **modes)
    assert e.value.code == -1 and "FADEHIP_BAM_INDEX does not combine with " + flag in str(e.value)


def test_back_index_without_the_flag_is_a_state_error(ctx):
    recs, cuts, _ = _build(0xff00)
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True)
    try:
        st.front_raw(b"".join(recs[:10]), last=True)
        st.back()
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back_index()
        assert e.value.code == -6
    finally:
        st.close()
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, stored=True, index=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back_index()                          # before any back
        assert e.value.code == -6
    finally:
        st.close()
