"""FADEHIP_BAM_STORE_OUTPUT (Context.bam_stream(..., store_output=store)): a stream's output records stay on the
device, in a record store, and leave it in coordinate order as they leave — whatever the input's order — in one window or,
when a budget says the store cannot hold them at once, in windows of the key space cut from a table measured on the device.

The expected records are never computed by the code under test: they are what the UNFLAGGED stream of the same modes hands
out, put in order and into buckets and windows by tests/sorted_out_model.py.  Every comparison is byte for byte, and the
bucket table is held to the model exactly (integer sums)."""
import gzip
import random
import struct

import pytest

import fade_amd
import bai_model as bm
import clip_cases as cc
import mates_cases as mc
import sorted_out_model as sm
import test_gpu_bam_from_tags as ft
import test_gpu_bam_index as bi
import test_gpu_recstore as gr
from test_gpu_recstore import synth4k  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NAMES = ["ctgA", "ctgB", "ctgC"]
LEN = [1100 * 65536, 10, 70000]     # ctgA: 1,101 buckets, ctgB: one, ctgC: two; then the last bucket


# ---------------------------------------------------------------------------------------------- records
def _tagged(aux):
    return bytearray(cc.build_rec("r0000000", 0, 0, 30, 0, -1, -1, 0, "20M", "ACGTACGTACGTACGTACGT", "5" * 20, aux))


_CLEAN = _tagged(b"rsC\x00")
_ART = _tagged(b"rsC\x02" + ft._z(b"am", b"ctgA,5,3M;"))


def _rec(k, tid, pos, art=False):
    """A small annotated record, number k in its name, at (tid, pos): clean, or an artifact call on its left side."""
    r = bytearray(_ART if art else _CLEAN)
    struct.pack_into("<ii", r, 4, tid, pos)
    r[37:44] = b"%07d" % k
    return bytes(r)


def _keys_of(pattern, n):
    """(tid, pos) of n records, input order: the bucket pattern across a wavefront's lanes is the point."""
    if pattern == "one_bucket":
        return [(0, 3 * 65536 + 5 + (n - k) % 900) for k in range(n)]
    if pattern == "alternating":
        return [(0, 65536 * 2 + 100 - k % 50) if k % 2 else (2, 66000 + k % 7) for k in range(n)]
    if pattern == "ref_change_mid_wave":
        return [(0, 40 + k) if k % 64 < 29 else (2, 10 + k) if k % 64 < 50 else (-1, -1) for k in range(n)]
    raise AssertionError(pattern)


def _own_bucket_keys(n):
    """n records, each in a bucket of its own (n <= 1,101), out of order."""
    order = list(range(n))
    random.Random(n).shuffle(order)
    return [(0, b * 65536 + 9) for b in order]


# ---------------------------------------------------------------------------------------------- runs
def _plain(ctx, names, payload, cuts=(), **modes):
    """What the unflagged stream of the same modes writes: (records, ejected)."""
    r = ft._stream(ctx, names, payload, cuts, **modes)
    return sm.split(r["out"]), r["ejected"]


def _feed(st, payload, cuts, depth):
    """front_raw / back with at most `depth` calls in flight; every back hands out nothing."""
    edges = [0] + sorted(cuts) + [len(payload)]
    spans = list(zip(edges, edges[1:]))
    done = 0
    for j, (a, b) in enumerate(spans):
        st.front_raw(payload[a:b], last=(j == len(spans) - 1))
        if j + 1 - done >= depth:
            assert st.back() == b""
            done += 1
    while done < len(spans):
        assert st.back() == b""
        done += 1


def _pass(ctx, store, names, payload, cuts=(), depth=1, **modes):
    st = ctx.bam_stream(names, floor_len=-3, window=-1, from_tags=True, store_output=store, **modes)
    try:
        _feed(st, payload, cuts, depth)
        return st.ejected()
    finally:
        st.close()


def _drain(store):
    store.sort()
    return b"".join(d for d, _ in gr._drain_all(store, raw=True))


def _one_window(ctx, names, payload, cuts=(), depth=1, ref_len=None, **modes):
    """(the raw drain, ejected, the table or None, (records, bytes) stored)"""
    s = ctx.recstore()
    try:
        if ref_len is not None:
            s.measure(ref_len)
        ej = _pass(ctx, s, names, payload, cuts, depth, **modes)
        count = s.count()
        hist = s.histogram() if ref_len is not None else None
        assert not s.over()
        return _drain(s), ej, hist, count
    finally:
        s.close()


def _window_loop(ctx, names, payload, ref_len, budget, cuts=(), depth=1, **modes):
    """The protocol of a file that may not fit: a measured first pass under the budget; if the store went over, one more pass
    per window of the model's cut of the DEVICE's table.  (the drains per window, went over, the table)"""
    s = ctx.recstore()
    try:
        s.set_budget(budget)
        s.measure(ref_len)
        _pass(ctx, s, names, payload, cuts, depth, **modes)
        hist = s.histogram()
        if not s.over():
            return [_drain(s)], False, hist
        assert s.count() == (0, 0)
        out = []
        for w in sm.windows(hist[0], hist[1], budget):
            nbytes, nrec = sum(hist[0][w[0]:w[1]]), sum(hist[1][w[0]:w[1]])
            s.reset(nbytes, nrec)
            s.set_window(*sm.window_keys(ref_len, w))
            _pass(ctx, s, names, payload, cuts, depth, **modes)
            assert s.count() == (nrec, nbytes) and not s.over()
            out.append(_drain(s))
        return out, True, hist
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- kernel shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_the_table_and_the_drain_are_the_models_at_every_shape(ctx, n):
    for pattern in ("one_bucket", "own_bucket", "alternating", "ref_change_mid_wave"):
        keys = _own_bucket_keys(n) if pattern == "own_bucket" else _keys_of(pattern, n)
        for ejecting in (False, True):
            recs = [_rec(k, t, p, art=ejecting and k % 3 == 1) for k, (t, p) in enumerate(keys)]
            modes = dict(eject="records") if ejecting else {}
            payload = b"".join(recs)
            want, want_ej = _plain(ctx, NAMES, payload, **modes)
            assert len(want) == n - (len([k for k in range(n) if k % 3 == 1]) if ejecting else 0) and want_ej == n - len(want)
            got, ej, hist, count = _one_window(ctx, NAMES, payload, ref_len=LEN, **modes)
            assert ej == want_ej and count == (len(want), sum(map(len, want))), (pattern, ejecting)
            assert hist == sm.histogram(LEN, want), (pattern, ejecting)
            assert got == b"".join(sm.order(want)), (pattern, ejecting)
            if pattern == "own_bucket" and not ejecting:
                assert sum(1 for x in hist[1] if x) == n and max(hist[1]) == 1


def test_more_distinct_buckets_in_a_wavefront_than_it_adds_up_by_ballot(ctx):
    """Five, eight and sixty-four buckets among the lanes of one wavefront (bam_sortwin.hpp's SW_WAVE_BUCKETS is 4): the lanes
    left over add their own."""
    for distinct in (4, 5, 8, 64):
        keys = [(0, (k % distinct) * 65536 + k) for k in range(640)]
        recs = [_rec(k, t, p) for k, (t, p) in enumerate(keys)]
        got, _, hist, _ = _one_window(ctx, NAMES, b"".join(recs), ref_len=LEN)
        assert hist == sm.histogram(LEN, recs) and sum(1 for x in hist[1] if x) == distinct
        assert got == b"".join(sm.order(recs))


# ---------------------------------------------------------------------------------------------- window edges
def test_records_at_the_windows_edges(ctx):
    lo_t, lo_p, hi_t, hi_p = 0, 70000, 2, 300          # (edges that are no bucket's: any pair of keys is a window)
    lo, hi = (lo_t << 32) | (lo_p + 1), (hi_t << 32) | (hi_p + 1)
    edge = [(0, lo_p - 1), (0, lo_p), (0, lo_p + 1), (2, hi_p - 1), (2, hi_p), (2, hi_p + 1), (0, -1), (-1, -1), (1, 5), (0, 65536 * 1000)]
    rng = random.Random(4)
    keys = edge * 3 + [(rng.choice([0, 0, 1, 2, -1]), rng.randrange(-1, 140000)) for _ in range(700)]
    rng.shuffle(keys)
    recs = [_rec(k, t, p) for k, (t, p) in enumerate(keys)]
    inside = [r for r in recs if lo <= sm.key(r) <= hi]
    assert {sm.key(r) for r in inside} >= {lo, hi, lo + 1, hi - 1} and not {sm.key(r) for r in inside} & {lo - 1, hi + 1}
    s = ctx.recstore()
    try:
        s.set_window(lo, hi)
        for cuts in ((), ft._offsets(b"".join(recs))[1:-1:97]):
            _pass(ctx, s, NAMES, b"".join(recs), cuts)
            assert s.count() == (len(inside), sum(map(len, inside)))
            assert _drain(s) == b"".join(sm.order(inside))
            s.reset()                                   # (the window stays)
        s.set_window(hi + 1, hi + 1)                    # a window of one key
        _pass(ctx, s, NAMES, b"".join(recs))
        assert _drain(s) == b"".join(r for r in recs if sm.key(r) == hi + 1) != b""
        s.reset()
        s.set_window(5, 5)                              # a window that holds nothing
        _pass(ctx, s, NAMES, b"".join(recs))
        assert s.count() == (0, 0) and _drain(s) == b""
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- streams
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """test_gpu_recstore's annotated golden set (name-collated, two-sided reads among it), its records shuffled as well."""
    names, payload, rs = gr._gold(tmp_path_factory)
    recs = ft._records(payload)
    shuffled = list(recs)
    random.Random(77).shuffle(shuffled)
    return names, payload, b"".join(shuffled), rs


def _cuts(payload, cutting):
    off = ft._offsets(payload)
    return {"one_call": ([], 1), "record_per_call": (off[1:-1], 1), "many_calls": (off[5:-1:11], 1), "two_in_flight": (off[3:-1:5], 2)}[cutting]


@pytest.mark.parametrize("cutting", ["one_call", "record_per_call", "many_calls", "two_in_flight"])
@pytest.mark.parametrize("mode", ["plain", "clip", "eject_records", "eject_groups"])
def test_a_from_tags_stream_stores_what_the_plain_stream_writes(ctx, gold, mode, cutting, monkeypatch):
    names, collated, shuffled, rs = gold
    modes = {"plain": {}, "clip": dict(clip=True), "eject_records": dict(eject="records"), "eject_groups": dict(eject="groups")}[mode]
    payload = collated if mode == "eject_groups" else shuffled       # (groups are neighbours in name-collated input)
    cuts, depth = _cuts(payload, cutting)
    if mode == "eject_groups":                                        # a group never lies across two calls
        recs = ft._records(payload)
        keep = {sum(map(len, recs[:k])) for k in range(1, len(recs)) if recs[k][36:36 + recs[k][12]] != recs[k - 1][36:36 + recs[k - 1][12]]}
        cuts = [c for c in cuts if c in keep]
    if cutting == "two_in_flight":
        monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "256")          # the arena grows while two calls are in flight
    want, want_ej = _plain(ctx, names, payload, cuts, **modes)
    reset = None
    if mode == "clip":
        src = ft._records(payload)
        reset = [_is_reset(a, b) for a, b in zip(src, want)]
        assert len(src) == len(want) and any(sm.key(a) != sm.key(b) for a, b in zip(src, want))   # a clip moved a pos
    ref_len = [150000] * len(names)
    got, ej, hist, count = _one_window(ctx, names, payload, cuts, depth, ref_len=ref_len, **modes)
    assert ej == want_ej and count == (len(want), sum(map(len, want)))
    assert hist == sm.histogram(ref_len, want, reset)
    assert got == b"".join(sm.order(want, reset))
    if mode != "plain":
        assert got != b"".join(sm.order(ft._records(payload)))       # (the mode did something)


def _is_reset(src, out):
    """A record that went in mapped with a CIGAR and came out zero-filled: refID 0, pos 0, flag 0, no op."""
    return struct.unpack_from("<H", src, 16)[0] > 0 and struct.unpack_from("<iiBBHHH", out, 4)[:2] == (0, 0) and struct.unpack_from("<HH", out, 16) == (0, 0)


def test_clipped_records_are_keyed_where_they_leave_and_reset_records_come_last(ctx):
    """Left clips that carry a record past later ones, right clips that move nothing, clips that reset the record — among
    records on the contigs behind ctgA, which a reset record's zero-filled bytes (refID 0, pos 0) would sort in front of."""
    def art(k, tid, pos, rs, left, right):
        am = b"ctgB,7,%dM;ctgB,9,%dM" % (left, right)
        return cc.build_rec("c%06d" % k, tid, pos, 30, 0, -1, -1, 0, "20M", "ACGTACGTACGTACGTACGT", "5" * 20, bytes([114, 115, 67, rs]) + ft._z(b"am", am))
    recs, k = [], 0
    rng = random.Random(9)
    for _ in range(300):
        tid, pos = rng.choice([0, 2]), rng.randrange(0, 60)
        kind = rng.randrange(5)
        if kind == 0:
            recs.append(art(k, tid, pos, 2, rng.randrange(1, 19), 3))      # left clip: pos moves up
        elif kind == 1:
            recs.append(art(k, tid, pos, 4, 3, rng.randrange(1, 19)))      # right clip: pos stays
        elif kind == 2:
            recs.append(art(k, tid, pos, 6, 25, 2))                        # the left side takes the whole alignment: reset
        else:
            recs.append(_rec(k, tid, pos))
        k += 1
    payload = b"".join(recs)
    want, _ = _plain(ctx, NAMES, payload, clip=True)
    reset = [_is_reset(a, b) for a, b in zip(recs, want)]
    moved = [sm.key(a) != sm.key(b) for a, b, r in zip(recs, want, reset) if not r]
    assert len(want) == len(recs) and sum(reset) > 20 and sum(moved) > 20
    final = sm.order(want, reset)
    n_reset = sum(reset)
    assert all(struct.unpack_from("<i", r, 4)[0] == 0 and len(r) < len(recs[0]) for r in final[-n_reset:])   # the reset ones, at the end
    for cuts in ((), ft._offsets(payload)[1:-1:7]):
        got, _, hist, _ = _one_window(ctx, NAMES, payload, cuts, ref_len=LEN, clip=True)
        assert hist == sm.histogram(LEN, want, reset) and hist[1][-1] == n_reset
        assert got == b"".join(final)
    s = ctx.recstore()                                                     # the store counts them, whatever its window
    try:
        s.set_window(0, 5)
        _pass(ctx, s, NAMES, payload, ft._offsets(payload)[1:-1:7], 2, clip=True)
        assert s.resets() == n_reset and s.count()[0] < len(recs)
        s.reset()
        assert s.resets() == 0
        _pass(ctx, s, NAMES, payload)                                      # (no clip: nothing resets)
        assert s.resets() == 0
    finally:
        s.close()
    # and through windows, one per bucket that holds something: the reset records are the last window's
    nbytes, nrec = sm.histogram(LEN, want, reset)
    most = max(sm.cost(b, n) for b, n in zip(nbytes, nrec))
    per, over, _ = _window_loop(ctx, NAMES, payload, LEN, most, clip=True)
    assert over and len(per) >= 3 and b"".join(per) == b"".join(final)


def test_eject_named_and_fix_mates_streams(ctx):
    # eject_named: the two passes of `fade out --fragments` over shuffled records
    rng = random.Random(12)
    keys = [(rng.choice([0, 2, -1]), rng.randrange(-1, 140000)) for _ in range(900)]
    recs = []
    for k, (t, p) in enumerate(keys):
        r = bytearray(_rec(k // 2, t, p, art=(k % 14 == 3)))               # two records per name: an artifact call takes its mate along
        recs.append(bytes(r))
    payload = b"".join(recs)
    ns = ctx.nameset()
    try:
        assert ft._stream(ctx, NAMES, payload, no_output=True, collect_names=ns)["out"] == b""
        want, want_ej = _plain(ctx, NAMES, payload, eject_named=ns)
        assert 0 < want_ej < len(recs) and want_ej > sum(1 for k in range(len(recs)) if k % 14 == 3)
        got, ej, hist, _ = _one_window(ctx, NAMES, payload, ft._offsets(payload)[1:-1:101], 2, ref_len=LEN, eject_named=ns)
        assert ej == want_ej and hist == sm.histogram(LEN, want) and got == b"".join(sm.order(want))
    finally:
        ns.close()
    # fix_mates: the third of its three passes stores; mate fields and MC follow the clip as they do without the store
    records, rs, _, _ = mc.flat_tagged([name for name in mc.CASES if name != "aux_not_whole_in_front_of_mc"])
    payload = b"".join(records)
    names = ["ctgA", "ctgB"]
    ns, ms = ctx.nameset(), ctx.mateset()
    try:
        assert ft._stream(ctx, names, payload, no_output=True, collect_names=ns)["out"] == b""
        assert ft._stream(ctx, names, payload, no_output=True, clip=True, collect_mates=ns, mateset=ms)["out"] == b""
        want, _ = _plain(ctx, names, payload, clip=True, fix_mates=True, mateset=ms)
        clipped, _ = _plain(ctx, names, payload, clip=True)
        assert len(want) == len(records) and want != clipped                # (a mate field changed)
        reset = [_is_reset(a, b) for a, b in zip(records, want)]
        for cuts in ((), ft._offsets(payload)[1:-1:3]):
            got, _, hist, _ = _one_window(ctx, names, payload, cuts, 2, ref_len=[100000, 100000], clip=True, fix_mates=True, mateset=ms)
            assert hist == sm.histogram([100000, 100000], want, reset) and got == b"".join(sm.order(want, reset))
    finally:
        ms.close()
        ns.close()


def _annotate(s, pieces, depth, clip, store_of=None):
    """annotate's own stream over the synthetic BAM (test_gpu_recstore._annotate_run's framing): the main output's records, or
    with store_of (a function of the context: the store) whatever the stream left in it."""
    raw = s["bam"].read_bytes()
    payload = gzip.decompress(raw)
    at = 8 + struct.unpack_from("<i", payload, 4)[0]
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    names, lens = [], []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", payload, at)[0]
        names.append(payload[at + 4:at + 4 + ln - 1].decode())
        lens.append(struct.unpack_from("<i", payload, at + 4 + ln)[0])
        at += 8 + ln
    ms = ft._members(raw)
    cum, k = 0, 0
    while cum + struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0] <= at:
        cum += struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0]
        k += 1
    body = ms[k:]
    calls = [body[j:j + pieces] for j in range(0, len(body), pieces)] if pieces else [body]
    c = fade_amd.Context(device=0)
    store = None
    try:
        c.genome_upload(s["g"].names, s["g"].ascii_contigs())
        if store_of:
            store = c.recstore()
            store.measure(lens)
        st = c.bam_stream(names, floor_len=5, window=100, first_record=at - cum, clip=clip, store_output=store)
        out, done = [], 0
        try:
            for j, piece in enumerate(calls):
                st.front(b"".join(piece), last=(j == len(calls) - 1))
                if j + 1 - done >= depth:
                    out.append(st.back())
                    done += 1
            while done < len(calls):
                out.append(st.back())
                done += 1
        finally:
            st.close()
        if not store:
            return sm.split(b"".join(gzip.decompress(x) for x in out if x)), lens
        assert out == [b""] * len(calls)
        return _drain(store), store.histogram()
    finally:
        if store:
            store.close()
        c.close()


@pytest.mark.parametrize("clip", [False, True], ids=["annotate", "annotate_clip"])
def test_annotates_own_stream_stores_what_it_writes(synth4k, clip, monkeypatch):  # noqa: F811
    want, lens = _annotate(synth4k, 0, 1, clip)
    src = sm.split(_plain_input(synth4k))
    assert len(want) == len(src) > 3000
    reset = [clip and _is_reset(a, b) for a, b in zip(src, want)]
    if clip:
        assert sum(1 for a, b in zip(src, want) if struct.unpack_from("<i", a, 8) != struct.unpack_from("<i", b, 8)) > 10
    final = b"".join(sm.order(want, reset))
    assert final != b"".join(want)                                          # (the set is not in coordinate order as it is)
    monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "4096")
    for pieces, depth in ((0, 1), (1, 1), (2, 2)):
        got, hist = _annotate(synth4k, pieces, depth, clip, store_of=True)
        assert hist == sm.histogram(lens, want, reset)
        assert got == final


def _plain_input(s):
    payload = gzip.decompress(s["bam"].read_bytes())
    at = 8 + struct.unpack_from("<i", payload, 4)[0]
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", payload, at)[0]
    return payload[at:]


# ---------------------------------------------------------------------------------------------- budget and windows
@pytest.fixture(scope="module")
def spread():
    """3,000 shuffled records over the three contigs and the unmapped tail, some beyond their contig's end."""
    rng = random.Random(21)
    keys = [(0, rng.randrange(-1, 40 * 65536)) for _ in range(1800)] + [(1, rng.randrange(0, 300)) for _ in range(300)] + \
           [(2, rng.randrange(0, 90000)) for _ in range(500)] + [(-1, -1)] * 250 + [(-1, 5), (7, 3)] * 75
    rng.shuffle(keys)
    return [_rec(k, t, p, art=(k % 11 == 0)) for k, (t, p) in enumerate(keys)]


def test_a_tiny_budget_sends_the_first_pass_over_and_the_window_loop_yields_the_same_bytes(ctx, spread):
    payload = b"".join(spread)
    cuts = ft._offsets(payload)[1:-1:211]
    want, _ = _plain(ctx, NAMES, payload, cuts, eject="records")
    final = b"".join(sm.order(want))
    nbytes, nrec = sm.histogram(LEN, want)
    total, most = sm.cost(sum(nbytes), sum(nrec)), max(sm.cost(b, n) for b, n in zip(nbytes, nrec))
    seen = []
    for budget in (total, total - 1, total // 3, most):                    # fits exactly; over by one byte; a few windows; a window per bucket, nearly
        per, over, hist = _window_loop(ctx, NAMES, payload, LEN, budget, cuts, 2, eject="records")
        assert hist == (nbytes, nrec)
        assert over == (budget < total)
        assert len(per) == len(sm.windows(nbytes, nrec, budget)) if over else len(per) == 1
        assert per == [b"".join(w) for w in sm.in_windows(LEN, want, budget)] if over else per == [final]
        assert b"".join(per) == final
        seen.append(len(per))
    assert seen[0] == 1 and seen[1] == 2 and 2 < seen[2] < seen[3]


def test_a_budget_of_one_buckets_cost_makes_every_bucket_that_holds_something_a_window(ctx):
    buckets = [0, 1, 2, 5, 9, 10, 400, 1100, 1101, 1102, 1103, 1104]       # (1100: ctgA's last; ctgB's; ctgC's two; the last bucket)
    keys = []
    for b in buckets:
        lo, _, ref = sm.bucket_range(LEN, b)
        keys += [(ref, (lo & 0xffffffff) - 1 + j) if ref >= 0 else (-1, -1) for j in range(1, 13)]
    random.Random(5).shuffle(keys)
    recs = [_rec(k, t, p) for k, (t, p) in enumerate(keys)]
    nbytes, nrec = sm.histogram(LEN, recs)
    assert [b for b, n in enumerate(nrec) if n] == buckets and set(nrec) == {0, 12}
    budget = sm.cost(nbytes[0], nrec[0])
    per, over, hist = _window_loop(ctx, NAMES, b"".join(recs), LEN, budget, ft._offsets(b"".join(recs))[1:-1:29])
    assert over and hist == (nbytes, nrec) and len(per) == len(buckets)
    assert [sm.split(w) for w in per] == sm.in_windows(LEN, recs, budget)
    assert b"".join(per) == b"".join(sm.order(recs))


def test_the_environment_overrides_the_budget(ctx, spread, monkeypatch):
    payload = b"".join(spread[:400])
    monkeypatch.setenv("FADEHIP_RECSTORE_BUDGET", "5000")
    s = ctx.recstore()
    try:
        s.set_budget(0)                                                     # (0 would derive one from the device's free memory)
        s.measure(LEN)
        _pass(ctx, s, NAMES, payload)
        assert s.over() and s.count() == (0, 0)
        assert s.histogram() == sm.histogram(LEN, spread[:400])             # measuring went on to the end of the pass
    finally:
        s.close()
    monkeypatch.setenv("FADEHIP_RECSTORE_BUDGET", "five")
    s = ctx.recstore()
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.set_budget(1 << 30)
        assert e.value.code == -1 and "FADEHIP_RECSTORE_BUDGET" in str(e.value)
    finally:
        s.close()
    monkeypatch.delenv("FADEHIP_RECSTORE_BUDGET")
    s = ctx.recstore()
    try:
        s.set_budget(0)                                                     # derived: a device with memory to spare holds 400 records
        s.measure(LEN)
        _pass(ctx, s, NAMES, payload)
        assert not s.over() and s.count()[0] == 400
    finally:
        s.close()


def test_a_bucket_alone_over_the_budget_is_named_by_the_model_from_the_devices_table(ctx):
    recs = [_rec(k, 0, 65536 * 3 + k) for k in range(500)] + [_rec(900 + k, 2, k) for k in range(10)]
    s = ctx.recstore()
    try:
        s.set_budget(20000)
        s.measure(LEN)
        _pass(ctx, s, NAMES, b"".join(recs))
        assert s.over()
        hist = s.histogram()
        with pytest.raises(sm.BucketOverBudget) as e:
            sm.windows(hist[0], hist[1], 20000)
        assert e.value.bucket == 3 and sm.bucket_range(LEN, 3)[:3] == (3 * 65536, 4 * 65536 - 1, 0)
        with pytest.raises(fade_amd.FadeHipError) as e:                     # and the store refuses to be sized for it
            s.reset(hist[0][3], hist[1][3])
        assert e.value.code == -4 and "budget of 20000 bytes" in str(e.value)
    finally:
        s.close()


def test_going_over_without_measuring_fails_with_nomem(ctx, spread):
    payload = b"".join(spread[:600])
    cuts = ft._offsets(payload)[1:-1:50]
    s = ctx.recstore()
    try:
        s.set_budget(30000)
        with pytest.raises(fade_amd.FadeHipError) as e:
            _pass(ctx, s, NAMES, payload, cuts)
        assert e.value.code == -4 and "budget of 30000 bytes" in str(e.value) and "holds every output record on the device" in str(e.value)
        n, b = s.count()
        assert 0 < n < 600 and sm.cost(b, n) <= 30000                       # the calls that fitted stay
        with pytest.raises(fade_amd.FadeHipError) as e:                     # add_batch answers to the same budget
            s.add_batch(spread[:600])
        assert e.value.code == -4
    finally:
        s.close()


def test_growth_from_256_bytes_under_a_budget_changes_nothing_and_stays_below_it(ctx, spread, monkeypatch):
    payload = b"".join(spread)
    cuts = ft._offsets(payload)[1:-1:37]
    want = b"".join(sm.order(spread))
    total = sm.cost(len(payload), len(spread))
    monkeypatch.setenv("FADEHIP_RECSTORE_BYTES", "256")
    s = ctx.recstore()
    try:
        s.set_budget(total)                                                 # the tightest budget the records fit
        _pass(ctx, s, NAMES, payload, cuts, 2)
        assert s.count() == (len(spread), len(payload)) and _drain(s) == want
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- state and flags
def test_calls_out_of_order_are_state_errors(ctx, spread):
    recs = spread[:50]
    s = ctx.recstore()
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.histogram()                                                   # before measure
        assert e.value.code == -6 and "fadehip_recstore_measure" in str(e.value)
        assert s.over() is False
        s.measure(LEN)
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.measure(LEN)                                                  # twice
        assert e.value.code == -6
        s.add_batch(recs)
        for call in (lambda: s.set_budget(1 << 20), lambda: s.set_window(0, 5)):   # on a store that holds records
            with pytest.raises(fade_amd.FadeHipError) as e:
                call()
            assert e.value.code == -6
        s.sort()
        for call in (lambda: s.set_budget(1 << 20), lambda: s.set_window(0, 5), lambda: _pass(ctx, s, NAMES, b"".join(recs))):   # sorted
            with pytest.raises(fade_amd.FadeHipError) as e:
                call()
            assert e.value.code == -6
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.set_window(9, 8)
        assert e.value.code == -1
        table = s.histogram()                                               # (what the refused pass measured before it was refused)
        s.reset()                                                           # a sorted store is emptied, and takes records again
        assert s.count() == (0, 0)
        s.set_budget(1 << 20)
        s.set_window(0, sm.ALL)
        _pass(ctx, s, NAMES, b"".join(recs))
        assert s.histogram() == table == sm.histogram(LEN, recs)            # reset ended measuring: the table stays as it was
        assert _drain(s) == b"".join(sm.order(recs))
        with pytest.raises(fade_amd.FadeHipError) as e:
            s.measure([-1])
        assert e.value.code == -1
    finally:
        s.close()
    other = fade_amd.Context(device=0)
    s = other.recstore()
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:                     # a store of another context
            ctx.bam_stream(NAMES, from_tags=True, store_output=s)
        assert e.value.code == -1
    finally:
        s.close()
        other.close()


def test_the_flag_its_refusals_and_its_store(ctx):
    from fade_amd import _lib
    assert _lib.BAM_STORE_OUTPUT == 131072
    refused = [("FADEHIP_BAM_NO_OUTPUT", dict(no_output=True)), ("FADEHIP_BAM_STORED", dict(stored=True)), ("FADEHIP_BAM_KEEP_SORTED", dict(clip=True, keep_sorted=True)),
               ("FADEHIP_BAM_INDEX", dict(index=True)), ("FADEHIP_BAM_EXTRACT", dict(extract=True)), ("FADEHIP_BAM_STORE_EXTRACT", dict(extract=True, recstore=True)),
               ("FADEHIP_BAM_COLLECT_NAMES", dict(collect_names=True)), ("FADEHIP_BAM_COLLECT_MATES", dict(clip=True, no_output=False, collect_mates=True)),
               ("FADEHIP_BAM_REPORT_STATS", dict(report="stats")), ("FADEHIP_BAM_REPORT_CLIP", dict(report="clip")), ("FADEHIP_BAM_REPORT_REPEATS", dict(repeats=True))]
    for name, modes in refused:
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.bam_stream(NAMES, from_tags=True, store_output=True, **modes)
        assert e.value.code == -1 and "FADEHIP_BAM_STORE_OUTPUT does not combine with" in str(e.value) and name in str(e.value).split("(")[0], (name, str(e.value))
    with pytest.raises(fade_amd.FadeHipError) as e:                         # what excludes each other without the flag still does
        ctx.bam_stream(NAMES, from_tags=True, store_output=True, clip=True, eject="records")
    assert e.value.code == -1 and "FADEHIP_BAM_CLIP and FADEHIP_BAM_EJECT" in str(e.value)
    st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, store_output=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:                     # flagged, no store attached: the first front call
            st.front_raw(_rec(0, 0, 5), last=True)
        assert e.value.code == -6 and "FADEHIP_BAM_STORE_OUTPUT" in str(e.value) and "fadehip_bam_use_recstore" in str(e.value)
    finally:
        st.close()
    s = ctx.recstore()
    try:
        st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, from_tags=True, store_output=True)
        try:
            assert st._L.fadehip_bam_use_recstore(st._h, s._h) == 0
            st.front_raw(b"")
            assert st._L.fadehip_bam_use_recstore(st._h, s._h) == -6       # attached after the first front call
        finally:
            st.close()
        # an empty stream, and a stream and add_batch sharing a store in call order
        _pass(ctx, s, NAMES, b"")
        a, b, c = _rec(1, 0, 7), _rec(2, 0, 7), _rec(3, 0, 7)
        s.add_batch([a])
        _pass(ctx, s, NAMES, b)
        s.add_batch([c])
        assert _drain(s) == a + b + c
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- drains
def test_indexed_drains_across_two_windows_serialise_to_one_bai(ctx):
    import bai_reader as br
    rng = random.Random(31)
    keys = [(0, rng.randrange(0, 300000)) for _ in range(700)] + [(2, rng.randrange(0, 60000)) for _ in range(300)] + [(-1, -1)] * 40
    rng.shuffle(keys)
    recs = [bi._rec(k, t, p, cigar="*", flag=4) if t < 0 else _rec(k, t, p) for k, (t, p) in enumerate(keys)]
    payload = b"".join(recs)
    nbytes, nrec = sm.histogram(LEN, recs)
    ws = sm.windows(nbytes, nrec, sm.cost(sum(nbytes), sum(nrec)) * 2 // 3)
    assert len(ws) == 2
    s = ctx.recstore()
    pieces, calls = [], []
    try:
        for w in ws:
            s.reset(sum(nbytes[w[0]:w[1]]), sum(nrec[w[0]:w[1]]))
            s.set_window(*sm.window_keys(LEN, w))
            _pass(ctx, s, NAMES, payload, ft._offsets(payload)[1:-1:97], 2)
            s.sort()
            for members, _, call in gr._drain_all(s, 20000, stored=True, index=True):
                pieces.append(members)
                calls.append(call)
    finally:
        s.close()
    assert len(pieces) > 4
    body = b"".join(p for x in pieces for _, p in br.walk_members(x))
    assert body == b"".join(sm.order(recs))
    # (one BaiBuilder over the drains of both windows, its file held to bai_model and read back by bai_reader's queries)
    allr, _, bai = bi._check_run(pieces, calls, len(NAMES))
    assert len(allr) == len(recs) and bm.read_bai(bai)["n_no_coor"] == 40
