"""`fade out -c --fix-mates` and the file path under FADEHIP_BAM_COLLECT_MATES / FADEHIP_BAM_FIX_MATES (Context.bam_stream)
against tests/mates_model.py: three passes over the same records — the names of the artifact calls, the placements of every primary paired-end record of
those names, then the clip with the mate fields following it — on the hand-built records of tests/mates_cases.py and on the
annotated golden sets given mate information by mates_model.pair_up, in one call and in many, with the tables starting small."""
import functools
import gzip
import random
import struct

import pytest

import bai_model as bm
import bai_reader as br
import fade_amd
import mates_cases as mc
import mates_model as mm
import nameset_model as nm
import resort_model as rm
import tags_model as tm
from fade_amd import _lib
from test_cli_fix_mates import W_FIX_MATES, W_PICARD, W_SORT
from test_gpu_annotate_clip import _ok, _run, _split
from test_gpu_bam_from_tags import SETS, _clip_trims, _records, _stream
from test_gpu_cli_out_device import EOF_MEMBER, _said, big  # noqa: F401  (big: the fixture)
from test_gpu_out_fragments import _bgzf, _recs_of

pytestmark = pytest.mark.gpu

NAMES = ["ctgA", "ctgB"]


def _model(records, rs, tl, tr):
    """(the records as they leave, fixed[], class counts, (entries, ambiguous) of the map, names in the set)."""
    names = nm.name_set(records, [1 if v & 6 else 0 for v in rs])
    mates = mm.insert({}, records, rs, tl, tr, pick=nm.contains(names, records))
    out, fixed, classes = mm.fix_batch(mates, records, rs, tl, tr)
    return out, fixed, classes, mm.count(mates), len(names)


def _three_passes(ctx, ref_names, records, cuts=(), **modes):
    """The three passes over the records through streams of one context: (records out, fixed, ambiguous, map count, names)."""
    payload = b"".join(records)
    ns, ms = ctx.nameset(), ctx.mateset()
    try:
        assert _stream(ctx, ref_names, payload, cuts, no_output=True, collect_names=ns)["out"] == b""
        assert _stream(ctx, ref_names, payload, cuts, no_output=True, clip=True, collect_mates=ns, mateset=ms)["out"] == b""
        st = ctx.bam_stream(ref_names, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True, fix_mates=True, mateset=ms, **modes)
        try:
            edges = [0] + sorted(cuts) + [len(payload)]
            out = []
            for j, (a, b) in enumerate(zip(edges, edges[1:])):
                st.front_raw(payload[a:b], last=(j == len(edges) - 2))
                piece = st.back()
                out.append(gzip.decompress(piece) if piece else b"")
            n_fixed, n_amb = st.mates()
        finally:
            st.close()
        return _records(b"".join(out)), n_fixed, n_amb, ms.count, ns.count
    finally:
        ms.close()
        ns.close()


def _hold(got, want):
    recs, n_fixed, n_amb, count, n_names = got
    out, fixed, _, want_count, want_names = want
    assert n_names == want_names and count == want_count
    assert len(recs) == len(out)
    for k, (g, w) in enumerate(zip(recs, out)):
        assert g == w, (k, g.hex(), w.hex())
    assert (n_fixed, n_amb) == (fixed.count(1), fixed.count(2))


# (the file path refuses a record whose aux area is not whole fields before any of this runs: that case is the batch call's)
FILE_CASES = [name for name in mc.CASES if name != "aux_not_whole_in_front_of_mc"]


@functools.lru_cache(maxsize=None)
def _hand():
    records, rs, tl, tr = mc.flat_tagged(FILE_CASES)
    return records, _model(records, rs, tl, tr)


@functools.lru_cache(maxsize=None)
def _gold(tag):
    """A golden set with mate information from unclipped geometry, MC on every second fragment, the hand-built cases behind it."""
    ref_names, _, bams = tm.annotated(tag)
    ref_names = ref_names + ["ctgB"][:max(0, 2 - len(ref_names))]  # (the hand-built records lie on two contigs)
    records = mm.pair_up(bams, mc=lambda rec: sum(rec[36:36 + rec[12]]) % 2 == 0)
    rs, tl, tr = [], [], []
    for rec in records:
        v, (a, b) = _clip_trims(rec, ref_names)
        rs.append(v or 0)
        tl.append(a)
        tr.append(b)
    hand = mc.flat_tagged(FILE_CASES)
    records, rs, tl, tr = records + hand[0], rs + hand[1], tl + hand[2], tr + hand[3]
    return ref_names, records, _model(records, rs, tl, tr), (rs, tl, tr)


def test_the_hand_built_cases_in_one_call_reach_every_class(ctx):
    records, want = _hand()
    assert all(want[2][c] >= 1 for c in mm.CLASSES), want[2]
    _hold(_three_passes(ctx, NAMES, records), want)


def test_the_hand_built_cases_cut_into_many_calls_with_small_tables(ctx, monkeypatch):
    monkeypatch.setenv("FADEHIP_MATESET_SLOTS", "16")
    monkeypatch.setenv("FADEHIP_MATESET_HASH_BITS", "0")
    monkeypatch.setenv("FADEHIP_NAMESET_SLOTS", "16")
    records, want = _hand()
    n = len(b"".join(records))
    _hold(_three_passes(ctx, NAMES, records, cuts=[n // 7 * k + k for k in range(1, 7)]), want)


@pytest.mark.parametrize("tag", SETS)
def test_golden_sets_with_mate_information_in_one_call_and_in_many(ctx, tag):
    ref_names, records, want, _ = _gold(tag)
    assert want[2]["fixed"] >= 10 and all(want[2][c] >= 1 for c in mm.CLASSES), want[2]
    _hold(_three_passes(ctx, ref_names, records), want)
    n = len(b"".join(records))
    _hold(_three_passes(ctx, ref_names, records, cuts=[n // 5 * k + 3 * k for k in range(1, 5)]), want)


def test_forbidden_combinations_are_refused_at_open_and_a_stream_without_its_sets_at_the_first_front(ctx):
    assert (_lib.BAM_COLLECT_MATES, _lib.BAM_FIX_MATES) == (8192, 16384)
    ms, ns = ctx.mateset(), ctx.nameset()
    try:
        for modes in (dict(fix_mates=True), dict(fix_mates=True, from_tags=True), dict(fix_mates=True, clip=True),
                      dict(fix_mates=True, from_tags=True, clip=True, extract=True), dict(fix_mates=True, from_tags=True, clip=True, no_output=True),
                      dict(fix_mates=True, from_tags=True, clip=True, collect_mates=True, no_output=True),
                      dict(collect_mates=True, from_tags=True, clip=True), dict(collect_mates=True, from_tags=True, no_output=True),
                      dict(collect_mates=True, from_tags=True, clip=True, no_output=True, keep_sorted=True),
                      dict(collect_mates=True, from_tags=True, clip=True, no_output=True, collect_names=True)):
            with pytest.raises(fade_amd.FadeHipError) as e:
                ctx.bam_stream(NAMES, mateset=ms, **modes)
            assert e.value.code == -1 and "FADEHIP_BAM_" in str(e.value), (modes, str(e.value))
        records = mc.flat_tagged(["example_mate_behind"])[0]
        for modes in (dict(fix_mates=True), dict(collect_mates=True, no_output=True, mateset=ms), dict(collect_mates=ns, no_output=True),
                      dict(collect_mates=True, no_output=True)):
            st = ctx.bam_stream(NAMES, floor_len=-3, window=-1, stored=True, from_tags=True, clip=True, **modes)
            try:
                with pytest.raises(fade_amd.FadeHipError) as e:
                    st.front_raw(b"".join(records), last=True)
                assert e.value.code == -6 and "attached" in str(e.value), (modes, e.value.code, str(e.value))
            finally:
                st.close()
        # the flags stand beside STORED, KEEP_SORTED and INDEX
        for modes in (dict(stored=True), dict(keep_sorted=True), dict(index=True), dict(stored=True, keep_sorted=True, index=True)):
            ctx.bam_stream(NAMES, from_tags=True, clip=True, fix_mates=True, mateset=ms, **modes).close()
    finally:
        ms.close()
        ns.close()


# ---------------------------------------------------------------------------------------------- `fade out -c --fix-mates`
SMALL = {"FADEHIP_MATESET_SLOTS": "16", "FADEHIP_MATESET_HASH_BITS": "0", "FADE_BAM_CHUNK_MB": "1"}


def _bam_bytes(ref_names, records):
    text = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:2147483647\n" % n for n in ref_names)
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(ref_names))
    for n in ref_names:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", 2147483647)
    return _bgzf(head + b"".join(records))


def _stats_lines(err):
    return [l for l in _said(err) if not l.startswith("[W::")]


def _fix(bam, fmt, extra=(), env=None):
    p = _ok(_run(["out", "-c", "--fix-mates", "--timing"] + list(extra) + [fmt, str(bam)], env))
    assert p.stderr.count(W_FIX_MATES) == 1 and W_PICARD not in p.stderr, p.stderr.decode()
    assert all(p.stderr.count(b"[timing] pass %d" % k) == 1 for k in (1, 2, 3)), p.stderr.decode()
    assert b"names collected" in p.stderr and b"placements stored" in p.stderr and b"records fixed" in p.stderr
    assert p.stdout.endswith(EOF_MEMBER)
    return p


@pytest.fixture(scope="module", params=SETS)
def files(request, tmp_path_factory):
    """A golden set with mate information and the hand-built cases, coordinate-sorted and shuffled, as BAM files; the model's
    records for both orders; the runs of `fade out -c --gpus 1` over them."""
    d = tmp_path_factory.mktemp("fix_mates_%s" % request.param)
    ref_names, records, want, trims = _gold(request.param)
    orders = {"sorted": sorted(range(len(records)), key=lambda i: (rm.key_in(records[i]), i)), "shuffled": list(range(len(records)))}
    random.Random(20261020).shuffle(orders["shuffled"])
    out = dict(ref_names=ref_names, want=want, records=records, trims=trims)
    for name, order in orders.items():
        bam = d / (name + ".bam")
        bam.write_bytes(_bam_bytes(ref_names, [records[i] for i in order]))
        out[name] = dict(bam=bam, recs_in=[records[i] for i in order], recs_out=[want[0][i] for i in order],
                         plain={fmt: _ok(_run(["out", "-c", "--gpus", "1", fmt, str(bam)])) for fmt in ("-b", "-u")})
    return out


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_the_output_is_the_models_in_input_order_with_the_header_and_the_stats_of_fade_out_c(files, order):
    f = files[order]
    for fmt in ("-b", "-u"):
        plain = f["plain"][fmt]
        assert plain.stderr.count(W_SORT) == 1 and plain.stderr.count(W_PICARD) == 1 and W_FIX_MATES not in plain.stderr
        for inflate in ("device", "host"):
            p = _fix(f["bam"], fmt, env={"FADE_BAM_INFLATE": inflate})
            assert ("inflate on the %s" % inflate).encode() in p.stderr and p.stderr.count(W_SORT) == 1
            assert _recs_of(p.stdout) == f["recs_out"]
            assert _split(p.stdout)[0] == _split(plain.stdout)[0] and _stats_lines(p.stderr) == _stats_lines(plain.stderr)
            assert (b"%d names collected" % files["want"][4]) in p.stderr and (b"%d placements stored" % files["want"][3][0]) in p.stderr
            assert (b"%d records fixed" % files["want"][1].count(1)) in p.stderr


def test_small_tables_and_small_calls_give_identical_bytes(files):
    f = files["shuffled"]
    assert _split(_fix(f["bam"], "-b", env=SMALL).stdout) == _split(_fix(f["bam"], "-b").stdout)


def test_keep_sorted_gives_the_same_records_in_the_resort_models_order(files):
    f = files["sorted"]
    keys = [rm.key_out(a, b) for a, b in zip(f["recs_in"], f["recs_out"])]
    order = rm.stable_order(keys)
    assert sum(1 for k, i in enumerate(order) if k != i) >= 1, "the clip moves records of this input"
    for fmt in ("-b", "-u"):
        assert _recs_of(_fix(f["bam"], fmt, ["--keep-sorted"]).stdout) == [f["recs_out"][i] for i in order]


def test_write_index_is_the_bai_models_over_the_output(files, tmp_path):
    """Without the records the clip resets: under --keep-sorted those leave at the end with refID 0 in their bytes, which no
    index of a coordinate-sorted file takes — with or without --fix-mates."""
    records, (rs, tl, tr) = files["records"], files["trims"]
    keep = [i for i in range(len(records)) if not rm.is_reset(records[i], files["want"][0][i])]
    keep.sort(key=lambda i: (rm.key_in(records[i]), i))
    assert len(keep) < len(records)
    sel = lambda a: [a[i] for i in keep]
    want = _model(sel(records), sel(rs), sel(tl), sel(tr))
    assert want[1].count(1) >= 10
    bam = tmp_path / "no_resets.bam"
    bam.write_bytes(_bam_bytes(files["ref_names"], sel(records)))
    order = rm.stable_order([rm.key_in(r) for r in want[0]])
    path = str(tmp_path / "out.bai")
    indexed = _fix(bam, "-b", ["--keep-sorted", "--write-index", path])
    assert _recs_of(indexed.stdout) == [want[0][i] for i in order]
    assert _split(indexed.stdout) == _split(_fix(bam, "-b", ["--keep-sorted"]).stdout)
    n_ref, recs = br.bam_records(indexed.stdout)
    bai = open(path, "rb").read()
    assert len(bm.read_bai(bai)["refs"]) == n_ref and bai == bm.build(n_ref, recs)
    br.check_queries(indexed.stdout, bai, recs, n_ref)


def test_30000_reads_shuffled_in_many_calls_with_mates_in_different_calls(big, tmp_path):  # noqa: F811
    raw = gzip.decompress(big.read_bytes())
    recs = _recs_of(big.read_bytes())
    head = raw[:len(raw) - sum(len(r) for r in recs)]
    # the fixture's reads come in name-sorted pairs: the first of a pair becomes segment 1, the second segment 2
    recs = [r[:18] + struct.pack("<H", (struct.unpack_from("<H", r, 18)[0] & ~0xC1) | 1 | (0x40 if k % 2 == 0 else 0x80)) + r[20:] for k, r in enumerate(recs)]
    recs = mm.pair_up(recs, mc=lambda rec: rec[40] % 2 == 0)
    random.Random(7).shuffle(recs)
    ref_names = [l.split("\t")[1][3:] for l in _split(big.read_bytes())[0] if l.startswith("@SQ")]
    rs, tl, tr = [], [], []
    for rec in recs:
        v, (a, b) = _clip_trims(rec, ref_names)
        rs.append(v or 0)
        tl.append(a)
        tr.append(b)
    want = _model(recs, rs, tl, tr)
    assert want[1].count(1) >= 1000 and want[2]["mc_replaced"] >= 100
    bam = tmp_path / "shuffled.bam"
    bam.write_bytes(_bgzf(head + b"".join(recs)))
    p = _fix(bam, "-b", env=SMALL)
    got = _recs_of(p.stdout)
    assert len(got) == len(want[0]) and all(g == w for g, w in zip(got, want[0]))
    assert (b"%d records fixed" % want[1].count(1)) in p.stderr


def test_a_bam_of_a_header_alone(tmp_path):
    bam = tmp_path / "empty.bam"
    bam.write_bytes(_bam_bytes(NAMES, []))
    p = _fix(bam, "-b")
    assert _recs_of(p.stdout) == [] and b"read count:\t0" in p.stderr and b"0 names collected" in p.stderr and b"0 records fixed" in p.stderr
