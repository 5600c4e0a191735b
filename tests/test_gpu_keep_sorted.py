"""FADEHIP_BAM_KEEP_SORTED on the file path (Context.bam_stream(..., clip=True, keep_sorted=True)): the clipped output of
coordinate-sorted input stays in coordinate order, a tail held on the device between calls.  Streams run with
from_tags=True, so the records' own rs / am fix every trim and no genome is needed; front_raw + stored members.  The
expectation is the unflagged stream's records (held to filter.d elsewhere), byte for byte, in the order tests/resort_model.py
states — over the whole stream and call by call."""
import gzip
import random

import pytest

import fade_amd
import clip_cases as cc
import resort_model as rm
from test_gpu_bam_from_tags import _offsets, _records

pytestmark = pytest.mark.gpu

NAMES = ["c0", "c1"]
READ = 50


def _rec(k, tid, pos, left=0, right=0, tags=True):
    """Record k: 50M at (tid, pos) whose am sides take `left` / `right` reference bases (rs says which sides count)."""
    aux = b""
    if tags:
        rs = (2 if left else 0) | (4 if right else 0)
        am = (b"c0,1,%dM" % left if left else b"") + b";" + (b"c1,1,%dM" % right if right else b"")
        aux = b"rsC" + bytes([rs]) + b"amZ" + am + b"\0" + b"NMC\x01"
    seq = "".join("ACGT"[(k + j) % 4] for j in range(READ))
    if tid < 0:
        return cc.build_rec("u%05d" % k, -1, -1, 0, 4, -1, -1, 0, "*", seq, "I" * READ, aux)
    return cc.build_rec("r%05d" % k, tid, pos, 30, 0, -1, -1, 0, "%dM" % READ, seq, "5" * READ, aux)


def _build():
    """The file: (records, marks) — marks name the records the edges hang on."""
    rng = random.Random(20)
    recs, marks = [], {}

    def add(tid, pos, left=0, right=0, tags=True):
        recs.append(_rec(len(recs), tid, pos, left, right, tags))
        return len(recs) - 1

    def clip(p):
        r = rng.random()
        return (0, 0) if r < 0.8 else (rng.randrange(1, 45), 0) if r < 0.9 else (0, rng.randrange(1, 45)) if r < 0.94 \
            else (rng.randrange(1, 25), rng.randrange(1, 25)) if r < 0.98 else (rng.randrange(50, 60), 0) if r < 0.99 else (30, 30)

    pos = 100
    for _ in range(500):  # contig 0: a few per cent move, some are reset
        pos += rng.randrange(0, 4)
        add(0, pos, *clip(pos), tags=rng.random() < 0.9)
    # a left clip whose new pos passes the call's last record (a designed cut comes two records behind it)
    marks["far"] = add(0, pos, 45)
    add(0, pos + 1)
    marks["far_cut"] = add(0, pos + 2)
    pos += 3
    # two records clipped onto one new pos, which an unclipped record has too
    marks["same"] = add(0, pos, 10)
    add(0, pos + 5, 5)
    for d in range(6, 10):
        add(0, pos + d)
    add(0, pos + 10)
    add(0, pos + 10, 0, 7)
    pos += 12
    # a pile-up at one position, longer than a call: its left-clipped records are held while it lasts
    marks["pile"] = len(recs)
    add(0, pos, 30)
    for j in range(700):
        add(0, pos, *((rng.randrange(1, 40), 0) if j % 97 == 5 else (0, rng.randrange(1, 30)) if j % 89 == 7 else (0, 0)))
    marks["pile_end"] = len(recs)
    for _ in range(150):
        pos += rng.randrange(0, 3)
        add(0, pos, *clip(pos))
    # the last records of contig 0 move up and are held while the next call begins on contig 1
    add(0, pos + 1, 40)
    add(0, pos + 1, 20, 10)
    marks["contig1"] = len(recs)
    pos = 0
    for _ in range(450):
        pos += rng.randrange(0, 5)
        add(1, pos, *clip(pos))
    add(1, pos, 50)   # reset records right in front of the unmapped tail: they keep their place in front of it
    add(1, pos, 10, 45)
    marks["tail"] = len(recs)
    for _ in range(40):
        add(-1, -1, tags=False)
    return recs, marks


RECS, MARKS = _build()
PAYLOAD = b"".join(RECS)
ENDS = _offsets(PAYLOAD)[1:]  # where every record ends


def _run(ctx, payload, cuts, depth=1, **modes):
    """The payload through a FROM_TAGS clip stream, cut at the byte offsets `cuts` (one equal to len(payload): an empty last
    call), at most `depth` calls between front and back: per call the records written, held() behind it, the extract bytes."""
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True, **modes)
    try:
        edges = [0] + sorted(cuts) + [len(payload)]
        pieces, held, xs, done = [], [], [], 0

        def back():
            piece = st.back()
            pieces.append(gzip.decompress(piece) if piece else b"")
            held.append(st.held())
            if modes.get("extract"):
                xs.append(st.back_extract()[0])

        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(payload[a:b], last=(j == len(edges) - 2))
            if j + 1 - done >= depth:
                back()
                done += 1
        while done < len(edges) - 1:
            back()
            done += 1
        return dict(pieces=pieces, out=b"".join(pieces), held=held, x=b"".join(xs), totals=st.totals())
    finally:
        st.close()


def _calls_of(cuts, ends=ENDS, total=len(PAYLOAD)):
    """Which records every call frames: a record belongs to the call that brings its last byte."""
    edges = sorted(cuts) + [total]
    calls, at = [], 0
    for e in edges:
        n = 0
        while at + n < len(ends) and ends[at + n] <= e:
            n += 1
        calls.append(list(range(at, at + n)))
        at += n
    return calls


@pytest.fixture(scope="module")
def plain(ctx):
    """The unflagged stream: its records in input order, and their keys as they leave."""
    r = _run(ctx, PAYLOAD, [])
    out = _records(r["out"])
    assert len(out) == len(RECS)
    keys = [rm.key_out(a, b) for a, b in zip(RECS, out)]
    n_moved = sum(1 for a, b in zip(RECS, out) if rm.key_in(a) != rm.key_out(a, b))
    n_reset = sum(1 for a, b in zip(RECS, out) if rm.is_reset(a, b))
    assert n_moved > 100 and n_reset >= 4 and rm.stable_order(keys) != list(range(len(RECS)))  # (the file does what it is built for)
    assert [rm.key_in(a) for a in RECS] == sorted(rm.key_in(a) for a in RECS)
    return dict(out=out, keys=keys, x=_run(ctx, PAYLOAD, [], extract=True)["x"], totals=r["totals"])


def _model(plain, cuts):
    calls = _calls_of(cuts)
    return rm.run([[(rm.key_in(RECS[i]), plain["keys"][i], len(plain["out"][i])) for i in c] for c in calls])


def _designed_cuts():
    e = lambda i: ENDS[i]  # the cut behind record i
    p, q = MARKS["pile"], MARKS["pile_end"]
    return sorted({e(MARKS["far_cut"]), e(MARKS["same"]), e(MARKS["same"] + 1),   # ... a call of one record
                   e(p + 150), e(p + 350), e(p + 550), e(q + 5),                 # the pile-up over four calls
                   e(MARKS["contig1"] - 1),                                      # contig 0's held tail, the next call on contig 1
                   e(MARKS["contig1"] + 200) + 77,                               # in the middle of a record
                   e(MARKS["tail"] + 10), len(PAYLOAD)})                         # inside the unmapped tail; an empty last call


CUTS = {
    "designed": _designed_cuts(),
    "one_call": [],
    "record_per_call": ENDS[:-1],
    "random_bytes": sorted(random.Random(3).sample(range(1, len(PAYLOAD)), 12)),
    "stride": list(range(10007, len(PAYLOAD), 10007)),
}


@pytest.mark.parametrize("which", list(CUTS))
def test_the_stream_is_the_unflagged_records_in_stable_key_order(ctx, plain, which):
    cuts = CUTS[which]
    r = _run(ctx, PAYLOAD, cuts, depth=1 if which != "stride" else 2, keep_sorted=True)
    got = _records(r["out"])
    want = [plain["out"][i] for i in rm.stable_order(plain["keys"])]
    assert len(got) == len(want)
    assert got == want
    assert r["totals"] == plain["totals"]
    # call by call against the model: what is written, in which order, and how much is held behind
    model = _model(plain, cuts)
    assert len(model) == len(r["pieces"])
    for c, (m, piece) in enumerate(zip(model, r["pieces"])):
        assert _records(piece) == [plain["out"][i] for i in m["emitted"]], (which, c)
        if which != "stride":
            assert r["held"][c] == (len(m["held"]), m["held_bytes"]), (which, c)
    assert r["held"][-1] == (0, 0)
    keys = [rm.key_in(x) if not (x[4:12] == bytes(8) and x[16:20] == bytes(4)) else rm.KEY_UNMAPPED for x in got]
    assert keys == sorted(keys)


def test_the_designed_edges_are_there(plain):
    """The constructed file does hold what the cuts are aimed at (so that the test above walks those paths)."""
    cuts = CUTS["designed"]
    calls, model = _calls_of(cuts), _model(plain, cuts)
    call_of = {i: c for c, cs in enumerate(calls) for i in cs}
    far = MARKS["far"]
    assert far in model[call_of[far]]["held"] and plain["keys"][far] > rm.key_in(RECS[calls[call_of[far]][-1]])
    p = MARKS["pile"]
    assert sum(1 for m in model if p in m["held"]) >= 3 and len({call_of[i] for i in range(p, MARKS["pile_end"])}) >= 4
    cb = call_of[MARKS["contig1"] - 1]
    assert MARKS["contig1"] - 1 in model[cb]["held"] and calls[cb + 1][0] == MARKS["contig1"]
    assert any(len(c) == 1 for c in calls) and calls[-1] == [] and any(ENDS.count(x) == 0 for x in cuts if x < len(PAYLOAD))
    same = MARKS["same"]
    assert plain["keys"][same] == plain["keys"][same + 1] == rm.key_in(RECS[same + 6]) == plain["keys"][same + 6]
    assert sum(1 for i in range(MARKS["tail"]) if plain["keys"][i] == rm.KEY_UNMAPPED) >= 4
    both = [i for i, (a, b) in enumerate(zip(RECS, plain["out"])) if b"rsC\x06" in a and not rm.is_reset(a, b) and a != b]
    assert len(both) >= 5
    # held() is 0 behind a call whose last record lies beyond every clipped one, and not 0 somewhere in between
    assert any(not m["held"] for m in model[:-1]) and any(m["held"] for m in model)


@pytest.mark.parametrize("straddle", [False, True])
def test_unsorted_input_fails_back_with_the_record(ctx, straddle):
    k = 300
    assert rm.key_in(RECS[k]) < rm.key_in(RECS[k + 2])
    recs = list(RECS)
    recs[k], recs[k + 2] = recs[k + 2], recs[k]   # stream record k + 1 now comes behind a larger key
    first_bad = next(i for i in range(1, len(recs)) if rm.key_in(recs[i]) < rm.key_in(recs[i - 1]))
    payload = b"".join(recs)
    ends = _offsets(payload)[1:]
    cuts = [ends[100], ends[first_bad - 1] if straddle else ends[first_bad + 40]]
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True, keep_sorted=True)
    try:
        st.front_raw(payload[:cuts[0]])
        assert len(_records(gzip.decompress(st.back()))) > 0
        st.front_raw(payload[cuts[0]:cuts[1]])
        if straddle:
            st.back()
            st.front_raw(payload[cuts[1]:], last=True)
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.back()
        assert "bam stream: record %d: not in coordinate order (--keep-sorted needs coordinate-sorted input)" % first_bad in str(e.value)
        assert e.value.code == -1
    finally:
        st.close()


def test_extract_beside_the_flag(ctx, plain):
    cuts = CUTS["designed"]
    r = _run(ctx, PAYLOAD, cuts, extract=True, keep_sorted=True)
    assert len(plain["x"]) > 0 and r["x"] == plain["x"]
    assert _records(r["out"]) == [plain["out"][i] for i in rm.stable_order(plain["keys"])]


def test_close_with_records_held(ctx):
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True, keep_sorted=True)
    st.front_raw(PAYLOAD[:ENDS[MARKS["far_cut"]]])
    st.back()
    assert st.held()[0] >= 1
    st.close()  # (no last call: the held records are given back with the stream)
    plainly = ctx.bam_stream(NAMES, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True)
    try:
        assert plainly.held() == (0, 0)
    finally:
        plainly.close()


@pytest.mark.parametrize("modes", [dict(), dict(clip=True, no_output=True), dict(eject="records"), dict(clip=True, eject="groups"), dict(clip=True, collect_names=True),
                                   dict(clip=True, eject_named=True), dict(extract=True)])
def test_open_refuses_other_combinations(ctx, modes):
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, keep_sorted=True, **modes).close()
    assert e.value.code == -1 and "FADEHIP_BAM_KEEP_SORTED" in str(e.value)
