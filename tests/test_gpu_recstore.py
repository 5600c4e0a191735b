"""The record store (Context.recstore(), fadehip_recstore_*): records added in any order, sorted once on the
device, drained in coordinate order — raw, as BGZF members, as stored members, with the .bai entries of every drain — and the
streams that append their extract records to it (bam_stream(..., extract=True, recstore=store)).

The expected records are never computed by the code under test: they are the records the test builds (clip_cases.build_rec)
or the extract records the unflagged stream hands out (back_extract), put in order by tests/recstore_model.py.  Every
comparison is byte for byte.  Members are held to zlib and the index to tests/bai_model.py by the checks of
tests/test_gpu_bam_index.py, over offsets derived from the output's own members."""
import gzip
import random
import struct

import pytest

import fade_amd
import bai_model as bm
import bai_reader as br
import clip_cases as cc
import recstore_model as rm
import test_gpu_bam_index as bi
import test_gpu_bam_from_tags as ft

pytestmark = pytest.mark.gpu

RS_TILE = 2048       # bam_resort.hpp: items per block of the sort's histogram and scatter kernels
WHOLE = 1 << 40      # a max_payload no store here reaches


# ---------------------------------------------------------------------------------------------- records
_TEMPLATE = bytearray(cc.build_rec("r0000000", 0, 0, 30, 0, -1, -1, 0, "20M", "ACGTACGTACGTACGTACGT", "5" * 20, b"XAC\x07"))


def _quick(k, tid, pos):
    """A small record, number k in its name, at (tid, pos): the template with three fields patched."""
    r = bytearray(_TEMPLATE)
    struct.pack_into("<ii", r, 4, tid, pos)
    r[37:44] = b"%07d" % k
    return bytes(r)


def _numbered(keys):
    return [_quick(k, tid, pos) for k, (tid, pos) in enumerate(keys)]


def _random_keys(n, seed, n_tid=5, span=1 << 16):
    rng = random.Random(seed)
    return [(rng.randrange(n_tid), rng.randrange(span)) for _ in range(n)]


def _sized(k, tid, pos, size, name):
    """A record of exactly `size` bytes with the given name: a padding tag takes up the difference."""
    base = cc.build_rec(name, tid, pos, 30, 0, -1, -1, 0, "8M", "ACGTACGT", "5" * 8, b"")
    pad = size - len(base) - 4
    assert pad >= 0
    r = cc.build_rec(name, tid, pos, 30, 0, -1, -1, 0, "8M", "ACGTACGT", "5" * 8, b"XPZ" + b"p" * pad + b"\0")
    assert len(r) == size
    return r


def _case_records(case):
    if case == "none":
        return []
    if case == "one":
        return _numbered([(2, 77)])
    if isinstance(case, int):
        return _numbered(_random_keys(case, case))
    if case == "all_equal":
        return _numbered([(1, 500)] * 700)
    if case == "in_order":
        return _numbered(sorted(_random_keys(3000, 11)))
    if case == "reversed":
        return _numbered(sorted(set(_random_keys(3000, 12)), reverse=True))
    if case.startswith("byte"):
        # keys that differ in exactly one of the eight key bytes: pos + 1 holds bytes 0 .. 3, refID bytes 4 .. 7
        b = int(case[4:])
        rng = random.Random(b)
        vals = [rng.randrange(128 if b in (3, 7) else 256) for _ in range(600)]   # (refID and pos stay non-negative: bytes 3 and 7 below 128)
        keys = []
        for v in vals:
            key = 0x0102030405060708 & ~(0xff << (8 * b)) | (v << (8 * b))
            keys.append((key >> 32, (key & 0xffffffff) - 1))
        assert len({rm.key(_quick(0, t, p)) for t, p in keys}) == len(set(vals)) > 100 and keys[0][0] >= 65536
        return _numbered(keys)
    if case == "unmapped_among_mapped":
        rng = random.Random(5)
        keys = [(-1, -1) if k % 3 == 0 else (-1, rng.randrange(50)) if k % 7 == 0 else (rng.randrange(3), rng.randrange(-1, 900)) for k in range(900)]
        return _numbered(keys)
    if case == "sizes_and_names":
        # every residue of the size mod 4, names of 1 and 254 bytes (l_read_name 2 and 255), neighbours of unlike alignment
        rng = random.Random(6)
        out = []
        for k in range(240):
            name = "n" if k % 2 else "N" * 254
            out.append(_sized(k, rng.randrange(3), rng.randrange(400), 36 + len(name) + 1 + 4 + 4 + 8 + 4 + 40 + k % 13, name))
        assert {len(r) % 4 for r in out} == {0, 1, 2, 3}
        return out
    if case == "long_reads":
        rng = random.Random(7)
        out = _numbered(_random_keys(50, 8))
        for k in range(6):
            ops = [(1 + (j + k) % 3, "MID"[j % 3]) for j in range(300 + k)]
            cigar = "".join("%d%s" % o for o in ops) + "%dM" % (4096 - sum(n for n, o in ops if o in "MI"))
            seq = "".join(rng.choice("ACGT") for _ in range(4096))
            out.insert(7 * k, cc.build_rec("long%d" % k, k % 2, 1000 - 100 * k, 30, 0, -1, -1, 0, cigar, seq, "".join(chr(33 + (j * 7 + k) % 40) for j in range(4096)), b"NMi" + struct.pack("<i", k)))
        assert max(map(len, out)) > 6000 and struct.unpack_from("<H", out[0], 16)[0] > 300
        return out
    raise AssertionError(case)


CASES = ["none", "one", 255, 256, 257, RS_TILE - 1, RS_TILE, RS_TILE + 1, 70001, "all_equal", "in_order", "reversed"] + ["byte%d" % b for b in range(8)] + \
        ["unmapped_among_mapped", "sizes_and_names", "long_reads"]


def _drain_all(store, max_payload=WHOLE, **kw):
    out = []
    while True:
        got = store.drain(max_payload, **kw)
        if got[1] == 0:
            assert got[0] == b""
            return out
        out.append(got)


def _stored(ctx, batches, max_payload=WHOLE, **kw):
    """The batches added one after the other, the store sorted and drained: the drains."""
    s = ctx.recstore()
    try:
        for b in batches:
            s.add_batch(b)
        assert s.count() == (sum(len(b) for b in batches), sum(len(r) for b in batches for r in b))
        s.sort()
        return _drain_all(s, max_payload, **kw)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- the store and the raw drain
@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_raw_drain_is_the_models_order(ctx, case):
    recs = _case_records(case)
    want = rm.order(recs)
    cut = len(recs) // 3
    for batches in ([recs], [recs[:cut], [], recs[cut:]]):
        got = _stored(ctx, batches, raw=True)
        assert b"".join(d for d, _ in got) == b"".join(want)
        assert sum(n for _, n in got) == len(recs) and len(got) == (1 if recs else 0)
    if case in ("none", "one", 257, "sizes_and_names", "long_reads"):
        for mp in (1, 300, 7000):
            got = _stored(ctx, [recs], mp, raw=True)
            assert [rm.split(d) for d, _ in got] == rm.drains(recs, mp) and [n for _, n in got] == [len(x) for x in rm.drains(recs, mp)]


def test_pick_adds_only_the_picked_records(ctx):
    recs = _numbered(_random_keys(1500, 21))
    rng = random.Random(22)
    pick = [rng.randrange(3) for _ in recs]          # (any non-zero value picks)
    s = ctx.recstore()
    try:
        s.add_batch(recs, pick)
        s.add_batch(recs[:300], [0] * 300)
        s.add_batch(recs[:10])
        kept = [r for r, p in zip(recs, pick) if p] + recs[:10]
        assert s.count() == (len(kept), sum(map(len, kept)))
        s.sort()
        assert b"".join(d for d, _ in _drain_all(s, raw=True)) == b"".join(rm.order(kept))
    finally:
        s.close()


def test_an_empty_store_drains_nothing_in_every_form_and_its_index_serialises(ctx):
    s = ctx.recstore()
    try:
        assert s.count() == (0, 0)
        s.sort()
        assert s.drain(WHOLE, raw=True) == (b"", 0) and s.drain(1) == (b"", 0) and s.drain(WHOLE, stored=True) == (b"", 0)
        empty = dict(chunks=[], linear=[], refs=[], n=0, first_key=0, last_key=0)
        assert s.drain(WHOLE, index=True) == (b"", 0, empty) and s.drain(5, stored=True, index=True) == (b"", 0, empty)
    finally:
        s.close()
    b = fade_amd.BaiBuilder(3)
    try:
        assert b.finish() == bm.build(3, [])
    finally:
        b.close()


def test_growth_changes_nothing(ctx, monkeypatch):
    """FADEHIP_RECSTORE_BYTES at its smallest: the first arena holds two records, the arena doubles many times between the adds
    and jumps to what one large add needs; the item arrays (1024 at first) grow too."""
    recs = _case_records("sizes_and_names") + _numbered(_random_keys(5000, 31))
    batches = [recs[:1], recs[1:3], recs[3:8], recs[8:30], recs[30:200], recs[200:]] + [recs[k:k + 40] for k in range(0, 400, 40)]
    want = b"".join(d for d, _ in _stored(ctx, batches, raw=True))
    assert want == b"".join(rm.order([r for b in batches for r in b]))
    monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "1")
    assert b"".join(d for d, _ in _stored(ctx, batches, raw=True)) == want
    monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "100000")
    assert b"".join(d for d, _ in _stored(ctx, batches, raw=True)) == want


def test_a_failed_add_leaves_the_store_as_it_was(ctx):
    recs = _numbered(_random_keys(400, 41))
    bad = list(recs[:50])
    bad[17] = bad[17][:4] + bad[17][4:-3]            # block_size says three bytes more than there are
    worse = list(recs[:50])
    worse[31] = struct.pack("<I", 40) + bytes(40)    # l_read_name 0
    s = ctx.recstore()
    try:
        s.add_batch(recs[:200])
        before = s.count()
        for batch, k in ((bad, 17), (worse, 31)):
            with pytest.raises(fade_amd.FadeHipError) as e:
                s.add_batch(batch)
            assert e.value.code == -1 and "record %d " % k in str(e.value), str(e.value)
            assert s.count() == before
        s.add_batch(recs[200:])
        s.sort()
        assert b"".join(d for d, _ in _drain_all(s, raw=True)) == b"".join(rm.order(recs))
    finally:
        s.close()


def test_calls_out_of_order_are_state_errors(ctx, gold):
    names, x, _ = gold
    recs = _numbered(_random_keys(20, 51))
    s = ctx.recstore()
    try:
        s.add_batch(recs)
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.drain(WHOLE, raw=True)                 # drain before sort
        assert e.value.code == -6
        s.sort()
        for call in (lambda: s.add_batch(recs), lambda: s.add_batch([]), s.sort):      # add after sort, sort twice
            with pytest.raises(fade_amd.FadeHipError) as e:
                call()
            assert e.value.code == -6
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.drain(WHOLE, raw=True, index=True)
        assert e.value.code == -1 and "FADEHIP_RECSTORE_INDEX" in str(e.value)
        # a stream that appends to a sorted store fails where its call is finished
        st = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, extract=True, recstore=s)
        try:
            st.front_raw(x, last=True)
            with pytest.raises(fade_amd.FadeHipError) as e:
                st.back()
            assert e.value.code == -6 and "sorted" in str(e.value)
        finally:
            st.close()
        assert b"".join(d for d, _ in _drain_all(s, raw=True)) == b"".join(rm.order(recs))
    finally:
        s.close()


def test_the_stream_flag_and_its_store(ctx, gold):
    names, x, _ = gold
    from fade_amd import _lib
    assert _lib.BAM_STORE_EXTRACT == 32768
    with pytest.raises(fade_amd.FadeHipError) as e:   # the flag without EXTRACT
        ctx.bam_stream(names, from_tags=True, recstore=True)
    assert e.value.code == -1 and "FADEHIP_BAM_STORE_EXTRACT needs FADEHIP_BAM_EXTRACT" in str(e.value)
    with pytest.raises(fade_amd.FadeHipError) as e:   # what EXTRACT does not combine with stays refused, by its own message
        ctx.bam_stream(names, from_tags=True, extract=True, recstore=True, no_output=True, report="stats")
    assert e.value.code == -1 and "FADEHIP_BAM_REPORT_STATS" in str(e.value)
    st = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, extract=True, recstore=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:   # flagged, no store attached: the first front call
            st.front_raw(x, last=True)
        assert e.value.code == -6 and "fadehip_bam_use_recstore" in str(e.value)
    finally:
        st.close()
    s = ctx.recstore()
    st = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, extract=True, recstore=True)
    try:
        st._L.fadehip_bam_use_recstore(st._h, s._h)
        st.front_raw(x[:0])
        assert st._L.fadehip_bam_use_recstore(st._h, s._h) == -6    # attached after the first front call
        plain = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, extract=True)
        assert plain._L.fadehip_bam_use_recstore(plain._h, s._h) == -1   # a stream opened without the flag
        plain.close()
    finally:
        st.close()
        s.close()


# ---------------------------------------------------------------------------------------------- drains through the codec
def _shuffled(recs, seed):
    out = list(recs)
    random.Random(seed).shuffle(out)
    return out


def _indexed_drains(c, recs, mp, stored):
    s = c.recstore()
    try:
        s.add_batch(recs[:len(recs) // 2])
        s.add_batch(recs[len(recs) // 2:])
        s.sort()
        got = _drain_all(s, mp, stored=stored, index=True)
    finally:
        s.close()
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


lane = bi.lane   # (stored members on the shared context, each compressor geometry on a context pinned to it)


@pytest.mark.parametrize("where", ["below", "at", "above", "whole"])
def test_drains_are_members_with_an_index(lane, where):
    c, stored, block = lane
    built, _, marks = bi._build(block)
    recs = _shuffled(built, 61)
    want = rm.order(recs)
    # the placement against the block grid survives the shuffle: no key in front of the big record occurs twice
    at = [0]
    for r in want:
        at.append(at[-1] + len(r))
    assert at[marks["ends_on"] + 1] == block == at[marks["starts_on"]] and at[marks["big"]] // block == 1 and (at[marks["big"] + 1] - 1) // block >= 3
    mp = {"below": block - 1, "at": block, "above": block + 1, "whole": WHOLE}[where]
    pieces, counts, calls = _indexed_drains(c, recs, mp, stored)
    runs = rm.drains(recs, mp)
    assert counts == [len(x) for x in runs] and [k["n"] for k in calls] == counts
    payloads = [b"".join(p for _, p in br.walk_members(x)) for x in pieces]          # (walk_members inflates with zlib and checks CRC32 and ISIZE)
    assert payloads == [b"".join(x) for x in runs]
    if where != "whole":
        assert len(runs) > 5 and any(len(x) == 1 and len(x[0]) > mp for x in runs)   # the big record leaves alone
    mem0 = br.walk_members(pieces[0])
    assert [len(p) for _, p in mem0[:-1]] == [block] * (len(mem0) - 1)               # the geometry the placement was made for
    if stored:
        assert all(x[o + 18] == 1 for x in pieces for o, _ in br.walk_members(x))   # BFINAL, BTYPE 00: a stored block
    allr, per_call, bai = bi._check_run(pieces, calls, len(bi.NAMES))
    assert len(allr) == len(recs)
    if where == "whole":
        offs = [o for o, _ in mem0]
        r = per_call[0]
        assert r[marks["ends_on"]]["v"] == offs[1] << 16 == r[marks["starts_on"]]["u"]
        big = r[marks["big"]]
        assert offs.index(big["v"] >> 16) - offs.index(big["u"] >> 16) >= 2
    else:
        # a (refID, bin) run lies across the first two drains: both have a chunk of bin 4681 that abut, and the file has one
        assert calls[0]["chunks"][-1][:2] == (0, 4681) == calls[1]["chunks"][0][:2]
        assert calls[0]["chunks"][-1][3] == len(pieces[0]) << 16 and calls[1]["chunks"][0][2] == 0
    assert bm.read_bai(bai)["n_no_coor"] == 25


def test_one_record_per_drain(ctx):
    recs = _shuffled(_case_records("sizes_and_names")[:60] + [bi._rec(k, -1, -1, cigar="*", flag=4) for k in range(3)], 62)
    for stored in (True, False):
        pieces, counts, calls = _indexed_drains(ctx, recs, 1, stored)
        assert counts == [1] * len(recs)
        assert [b"".join(p for _, p in br.walk_members(x)) for x in pieces] == rm.order(recs)
        bi._check_run(pieces, calls, 3)


def test_a_record_beyond_2_29_fails_the_indexed_drain_and_names_it(ctx):
    recs = _numbered([(0, 500), (1, 10), (0, 100), (0, (1 << 29) - 10), (0, 7)])
    s = ctx.recstore()
    try:
        s.add_batch(recs)
        s.sort()
        assert s.drain(2 * len(recs[0]), stored=True, index=True)[1] == 2
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.drain(WHOLE, stored=True, index=True)
        assert e.value.code == -5 and "record 3: ends beyond 2^29" in str(e.value), str(e.value)   # (its number in final order)
        rest = _drain_all(s, raw=True)                                                             # the store stayed where it was
        assert b"".join(d for d, _ in rest) == b"".join(rm.order(recs)[2:])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- streams that append
def _from_tags_run(ctx, names, payload, cuts, depth, store=None):
    """The payload through a FROM_TAGS | EXTRACT stream cut at `cuts`, at most `depth` calls between front and back:
    (main output pieces, [(extract bytes, records)] per call)."""
    st = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, extract=True, recstore=store)
    try:
        edges = [0] + sorted(cuts) + [len(payload)]
        spans = list(zip(edges, edges[1:]))
        main, xs, done = [], [], 0

        def back():
            main.append(st.back())
            xs.append(st.back_extract())

        for j, (a, b) in enumerate(spans):
            st.front_raw(payload[a:b], last=(j == len(spans) - 1))
            if j + 1 - done >= depth:
                back()
                done += 1
        while done < len(spans):
            back()
            done += 1
        return main, xs
    finally:
        st.close()


def _gold(tmp_path_factory):
    import samutil
    from test_cli_extract import _annotated_sam
    from test_gpu_annotate_clip import _bam_of, _split
    d = tmp_path_factory.mktemp("recstore_gold")
    sam, bam = d / "anno.sam", d / "anno.bam"
    sam.write_text(_annotated_sam("anno_c5"))
    _bam_of(sam, bam)
    header, recs = samutil.parse_sam(sam.read_text())
    names = [dict(x.split(":", 1) for x in h.split("\t")[1:])["SN"] for h in header if h.startswith("@SQ")]
    bams = ft._records(ft._records_of_bam_body(_split(bam.read_bytes())[1]))
    rs = [int(r["tags"]["rs"][1]) for r in recs]
    assert len(bams) == len(rs) and sum(1 for v in rs if v & 6) > 10 and not any(v & 6 == 6 for v in rs)
    # the golden set calls no read on both sides: constructed ones among its records, their two sides far apart
    for j, k in enumerate(range(20, len(bams), 37)):
        am = b"%s,%d,7M2D3M;%s,%d,4M1I6M" % (names[j % len(names)].encode(), 90000 - 1000 * j, names[(j + 1) % len(names)].encode(), 10 + 3 * j)
        seq = "ACGTTGCAACGT"[:10 + j % 3]
        bams.insert(k, cc.build_rec("both%d" % j, j % len(names), 500 + j, 30, 16 * (j % 2), -1, -1, 0, "%dM" % len(seq), seq, "I" * len(seq), b"rsC\x06" + ft._z(b"am", am)))
        rs.insert(k, 6)
    return names, b"".join(bams), rs


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    return _gold(tmp_path_factory)


@pytest.mark.parametrize("cutting", ["one_call", "record_per_call", "inside_a_two_sided_read", "calls_without_artifacts", "two_in_flight"])
def test_a_from_tags_stream_appends_what_the_plain_stream_hands_out(ctx, gold, cutting, monkeypatch):
    names, payload, rs = gold
    off = ft._offsets(payload)
    both = [k for k, v in enumerate(rs) if v & 6 == 6]
    arts = [k for k, v in enumerate(rs) if v & 6]
    assert len(both) > 5 and len(arts) > 40
    depth = 1
    if cutting == "one_call":
        cuts = []
    elif cutting == "record_per_call":
        cuts = off[1:-1]
    elif cutting == "inside_a_two_sided_read":
        cuts = [off[k] + 40 for k in both] + [off[k + 1] for k in both[:3]]     # the read's record comes in two calls
    elif cutting == "calls_without_artifacts":
        clean = [k for k in range(len(rs) - 1) if not rs[k] & 6]
        cuts = sorted({off[k] for k in clean} | {off[k + 1] for k in clean})    # every clean record is a call of its own
    else:
        cuts, depth = off[3:-1:5], 2
        monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "1")                        # the arena grows while two calls are in flight
    main0, xs0 = _from_tags_run(ctx, names, payload, cuts, depth)
    want = rm.order(rm.split(b"".join(x for x, _ in xs0)))
    assert len(want) == sum(n for _, n in xs0) == sum(bin(v & 6).count("1") for v in rs)
    s = ctx.recstore()
    try:
        main1, xs1 = _from_tags_run(ctx, names, payload, cuts, depth, store=s)
        assert main1 == main0                                                    # the main output does not know about the store
        assert xs1 == [(b"", n) for _, n in xs0]                                 # no bytes cross; the counts are the plain stream's
        assert s.count() == (len(want), sum(map(len, want)))
        s.sort()
        got = _drain_all(s, 1, raw=True)                                         # every drain one record: the two sides of a read apart
        assert [d for d, _ in got] == want
    finally:
        s.close()


def test_streams_and_add_batch_share_a_store_in_call_order(ctx, gold):
    names, payload, _ = gold
    _, xs0 = _from_tags_run(ctx, names, payload, [], 1)
    x = rm.split(xs0[0][0])
    extra = _numbered([struct.unpack_from("<ii", x[0], 4)] * 3)                  # ties with the stream's first record
    s = ctx.recstore()
    try:
        s.add_batch(extra[:1])
        _from_tags_run(ctx, names, payload, [], 1, store=s)
        s.add_batch(extra[1:])
        _from_tags_run(ctx, names, payload, [ft._offsets(payload)[7]], 2, store=s)
        s.sort()
        assert b"".join(d for d, _ in _drain_all(s, raw=True)) == b"".join(rm.order(extra[:1] + x + extra[1:] + x))
    finally:
        s.close()


@pytest.fixture(scope="module")
def synth4k(tmp_path_factory):
    """4,000 reads of C5 as a BAM of a few dozen BGZF members (tests/test_gpu_annotate_extract.py's fixture, smaller)."""
    import samutil
    from fade_amd import synth
    from test_gpu_annotate_clip import _ok, _run
    d = tmp_path_factory.mktemp("recstore4k")
    cfg, g, b = synth.make_config("C5", 4000, contig_len=200_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    return dict(bam=bam, g=g)


def _annotate_run(s, pieces, depth, store_of=None):
    """tests/test_gpu_annotate_extract.py's _stream with at most `depth` calls in flight and, with store_of, a store attached:
    (main output pieces, [(extract bytes, records)], the raw drains of the sorted store)."""
    raw = s["bam"].read_bytes()
    payload = gzip.decompress(raw)
    at = 8 + struct.unpack_from("<i", payload, 4)[0]
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", payload, at)[0]
        names.append(payload[at + 4:at + 4 + ln - 1].decode())
        at += 8 + ln
    ms = ft._members(raw)
    cum, k = 0, 0
    while cum + struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0] <= at:
        cum += struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0]
        k += 1
    body = ms[k:]
    calls = [body[j:j + pieces] for j in range(0, len(body), pieces)] if pieces else [body]
    ctx = fade_amd.Context(device=0)
    store = None
    try:
        ctx.genome_upload(s["g"].names, s["g"].ascii_contigs())
        store = ctx.recstore() if store_of else None
        st = ctx.bam_stream(names, floor_len=5, window=100, first_record=at - cum, extract=True, recstore=store)
        main, xs, done = [], [], 0
        try:
            for j, c in enumerate(calls):
                st.front(b"".join(c), last=(j == len(calls) - 1))
                if j + 1 - done >= depth:
                    main.append(st.back())
                    xs.append(st.back_extract())
                    done += 1
            while done < len(calls):
                main.append(st.back())
                xs.append(st.back_extract())
                done += 1
        finally:
            st.close()
        drained = None
        if store:
            store.sort()
            drained = _drain_all(store, raw=True)
        return main, xs, drained
    finally:
        if store:
            store.close()
        ctx.close()


@pytest.mark.parametrize("pieces, depth", [(0, 1), (1, 1), (2, 2)], ids=["one_call", "member_per_call", "two_in_flight"])
def test_annotates_own_stream_appends_what_the_plain_stream_hands_out(synth4k, pieces, depth, monkeypatch):
    main0, xs0, _ = _annotate_run(synth4k, pieces, depth)
    want = rm.order(rm.split(b"".join(x for x, _ in xs0)))
    assert len(want) > 100
    monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "4096")
    main1, xs1, drained = _annotate_run(synth4k, pieces, depth, store_of=True)
    assert main1 == main0
    assert xs1 == [(b"", n) for _, n in xs0]
    assert b"".join(d for d, _ in drained) == b"".join(want)
