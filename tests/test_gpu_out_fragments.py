"""`fade out --fragments` and the file path under FADEHIP_BAM_COLLECT_NAMES / FADEHIP_BAM_EJECT_NAMED against
tests/nameset_model.py and the host loop of the same binary: the annotated golden sets name-sorted and shuffled, with -b and
-u, the device and the host inflating; 30,000 annotated reads shuffled and taken in many calls; the set growing from sixteen
slots with every name colliding while two calls are in flight; a BAM that holds a header alone; and the two flags through
Context.bam_stream."""
import struct
import zlib

import pytest

import fade_amd
import nameset_model as nm
import samutil
from test_cli_extract import _annotated_sam
from test_cli_out_fragments import W_FRAGMENTS
from test_gpu_annotate_clip import _bam_of, _ok, _run, _split
from test_gpu_annotate_eject import W_GROUPS, W_RECORDS
from test_gpu_bam_from_tags import SETS, _records, _records_of_bam_body, _shuffled, _stream
from test_gpu_cli_out_device import EOF_MEMBER, _said, big  # noqa: F401  (big: the fixture)

pytestmark = pytest.mark.gpu


def _recs_of(bam_bytes):
    return _records(_records_of_bam_body(_split(bam_bytes)[1]))


def _stats(err, warning):
    """What a run said beside its --timing lines and its warning (which must be there once): the stats block."""
    said = _said(err)
    assert said.count(warning.decode()) == 1, err.decode()
    return [l for l in said if l != warning.decode()]


def _fragments(bam, fmt, env=None):
    p = _ok(_run(["out", "--fragments", "--timing", fmt, str(bam)], env))
    assert p.stderr.count(W_FRAGMENTS) == 1 and W_GROUPS not in p.stderr and W_RECORDS not in p.stderr, p.stderr.decode()
    assert p.stderr.count(b"[timing] pass 1") == 1 and p.stderr.count(b"[timing] pass 2") == 1 and b"names collected" in p.stderr
    assert p.stdout.endswith(EOF_MEMBER)
    pg = [l for l in samutil.bam_to_sam_records(p.stdout)[0].splitlines() if l.startswith("@PG")]
    assert pg[-1].startswith("@PG\tID:fade-extract\tPN:fade") and " --fragments " in pg[-1]
    return p


def _hold(p, in_recs, host, in_order):
    """One --fragments run against the model over the input's records and against the host loop's run on the name-sorted file."""
    got = _recs_of(p.stdout)
    names = nm.artifact_names(in_recs)
    assert got == [r for r, k in zip(in_recs, nm.keep(names, in_recs)) if k]  # byte for byte, in input order
    host_recs = _recs_of(host.stdout)
    assert sorted(got) == sorted(host_recs) and 0 < len(got) < len(in_recs)
    if in_order:
        assert got == host_recs
    assert _split(p.stdout)[0] == _split(host.stdout)[0]  # the header without @PG
    assert _stats(p.stderr, W_FRAGMENTS) == _stats(host.stderr, W_GROUPS)
    assert p.stderr.count(b"read count:\t%d\n" % len(in_recs)) == 1
    return names


@pytest.fixture(scope="module", params=SETS)
def gold(request, tmp_path_factory):
    """An annotated golden set as a BAM, name-sorted and shuffled, and the host loop's runs on the name-sorted one."""
    d = tmp_path_factory.mktemp("fragments_%s" % request.param)
    lines = _annotated_sam(request.param).splitlines()
    out = {}
    for order, ls in (("sorted", lines), ("shuffled", _shuffled(lines))):
        sam, bam = d / (order + ".sam"), d / (order + ".bam")
        sam.write_text("\n".join(ls) + "\n")
        _bam_of(sam, bam)
        out[order] = bam
    out["host"] = {fmt: _ok(_run(["out", fmt, str(out["sorted"])])) for fmt in ("-b", "-u")}
    return out


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_golden_sets_whole_fragments_leave_whatever_the_order(gold, order):
    bam = gold[order]
    in_recs = _recs_of(bam.read_bytes())
    for fmt in ("-b", "-u"):
        for inflate in ("device", "host"):
            p = _fragments(bam, fmt, {"FADE_BAM_INFLATE": inflate})
            assert ("inflate on the %s" % inflate).encode() in p.stderr
            names = _hold(p, in_recs, gold["host"][fmt], order == "sorted")
            assert (b"%d names collected" % len(names)) in p.stderr


def test_the_set_grows_from_sixteen_slots_with_every_name_colliding_and_the_output_is_the_same(gold):
    bam = gold["shuffled"]
    plain = _fragments(bam, "-b")
    small = _fragments(bam, "-b", {"FADEHIP_NAMESET_SLOTS": "16", "FADEHIP_NAMESET_HASH_BITS": "0", "FADE_BAM_CHUNK_MB": "1"})
    assert _split(small.stdout) == _split(plain.stdout)
    _hold(small, _recs_of(bam.read_bytes()), gold["host"]["-b"], False)


def _bgzf(data):
    out = []
    for at in range(0, len(data), 0xff00):
        chunk = data[at:at + 0xff00]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + EOF_MEMBER


def test_30000_annotated_reads_shuffled_in_many_calls(big, tmp_path):  # noqa: F811
    import gzip
    raw = gzip.decompress(big.read_bytes())
    body = _split(big.read_bytes())[1]
    recs = _records(_records_of_bam_body(body))
    head = raw[:len(raw) - sum(len(r) for r in recs)]
    # shuffled by _shuffled, as lines of the name and the record's index
    order = [int(l.split("\t")[1]) for l in _shuffled(["%s\t%d" % (r[36:36 + r[12] - 1].decode(), k) for k, r in enumerate(recs)])]
    in_recs = [recs[k] for k in order]
    bam = tmp_path / "shuffled.bam"
    bam.write_bytes(_bgzf(head + b"".join(in_recs)))
    host = _ok(_run(["out", "-b", str(big)]))
    assert host.stderr.count(W_GROUPS) == 1
    names = None
    for env in ({"FADE_BAM_INFLATE": "device"}, {"FADE_BAM_INFLATE": "host"},
                # the set grows from sixteen slots, every name colliding with every other, while two calls are in flight
                {"FADE_BAM_INFLATE": "device", "FADEHIP_NAMESET_SLOTS": "16", "FADEHIP_NAMESET_HASH_BITS": "0"}):
        p = _fragments(bam, "-b", dict(env, FADE_BAM_CHUNK_MB="1"))
        names = _hold(p, in_recs, host, False)
    # what plain FADEHIP_BAM_EJECT would not do: records that leave without being artifact calls themselves
    mates = sum(1 for r in in_recs if nm.key(r) in names and not (nm.rs_of(r) or 0) & 6)
    print("records ejected that are not artifact calls themselves: %d of %d ejected" % (mates, sum(1 for r in in_recs if nm.key(r) in names)))
    assert mates >= 100


def test_a_bam_of_a_header_alone_gives_the_header_the_eof_member_and_a_read_count_of_zero(tmp_path):
    sam, bam = tmp_path / "empty.sam", tmp_path / "empty.bam"
    sam.write_text("\n".join(l for l in _annotated_sam("anno_c1").splitlines() if l.startswith("@")) + "\n")
    _bam_of(sam, bam)
    p = _fragments(bam, "-b")
    head, _ = _split(p.stdout)
    assert len(head) >= 2 and samutil.bam_to_sam_records(p.stdout)[2] == []
    assert b"read count:\t0" in p.stderr and b"0 names collected" in p.stderr


def _payload(gold, order):
    sam = gold[order].with_suffix(".sam").read_text()
    header, _ = samutil.parse_sam(sam)
    names = [dict(x.split(":", 1) for x in h.split("\t")[1:])["SN"] for h in header if h.startswith("@SQ")]
    return names, _records_of_bam_body(_split(gold[order].read_bytes())[1])


def test_through_context_bam_stream_collect_fills_the_set_and_eject_named_writes_the_rest(ctx, gold):
    ref, payload = _payload(gold, "shuffled")
    recs = _records(payload)
    model = nm.artifact_names(recs)
    assert 0 < len(model) < len(recs)
    cuts = [sum(len(r) for r in recs[:k]) for k in (len(recs) // 3, 2 * len(recs) // 3)]
    s = ctx.nameset()
    try:
        r = _stream(ctx, ref, payload, cuts, collect_names=s, no_output=True)
        assert r["out"] == b"" and r["ejected"] == 0 and r["totals"][1] == len(recs)
        assert s.count == len(model) and s.contains(recs).tolist() == nm.contains(model, recs)
        r = _stream(ctx, ref, payload, collect_names=s)  # the records pass as under FROM_TAGS alone; nothing new is added
        assert r["out"] == payload and s.count == len(model)
        want = [x for x, k in zip(recs, nm.keep(model, recs)) if k]
        r = _stream(ctx, ref, payload, cuts, eject_named=s)
        assert r["out"] == b"".join(want) and r["ejected"] == len(recs) - len(want) and r["totals"][1] == len(recs)
        # a record without rs is written unless its name is in the set
        loose = [nm.rec(b"no_rs_and_no_name_of_the_set"), nm.rec(b"nor_this_one"), nm.rec(sorted(model)[0][1][:-1])]
        assert nm.keep(model, loose) == [True, True, False] and all(nm.rs_of(x) is None for x in loose)
        r = _stream(ctx, ref, b"".join(loose), eject_named=s)
        assert r["out"] == b"".join(loose[:2]) and r["ejected"] == 1
    finally:
        s.close()


def test_through_context_bam_stream_the_flags_need_a_set_and_exclude_the_other_modes(ctx):
    s = ctx.nameset()
    try:
        st = ctx.bam_stream(["c"], from_tags=True, eject_named=True)  # the flag, and no set attached
        try:
            with pytest.raises(fade_amd.FadeHipError) as e:
                st.front_raw(nm.rec(b"r"), last=True)
            assert e.value.code == -6 and "name set" in str(e.value)
        finally:
            st.close()
        st = ctx.bam_stream(["c"], from_tags=True, collect_names=True)
        try:
            with pytest.raises(fade_amd.FadeHipError) as e:
                st.front_raw(nm.rec(b"r"), last=True)
            assert e.value.code == -6
        finally:
            st.close()
        for modes in (dict(from_tags=True, collect_names=s, eject_named=s), dict(collect_names=s), dict(eject_named=s),
                      dict(from_tags=True, collect_names=s, clip=True), dict(from_tags=True, eject_named=s, clip=True),
                      dict(from_tags=True, collect_names=s, extract=True), dict(from_tags=True, eject_named=s, extract=True),
                      dict(from_tags=True, collect_names=s, eject="records"), dict(from_tags=True, eject_named=s, eject="groups")):
            with pytest.raises(fade_amd.FadeHipError) as e:
                ctx.bam_stream(["c"], **modes)
            assert e.value.code == -1, modes
        for modes in (dict(collect_names=s, stored=True, no_output=True), dict(eject_named=s, stored=True), dict(eject_named=s, no_output=True)):
            ctx.bam_stream(["c"], from_tags=True, **modes).close()
        # attached after the first front call: FADEHIP_E_STATE
        st = ctx.bam_stream(["c"], from_tags=True, eject_named=s)
        try:
            st.front_raw(nm.rec(b"r"), last=False)
            assert ctx._L.fadehip_bam_use_nameset(st._h, s._h) == -6
            st.back()
        finally:
            st.close()
    finally:
        s.close()
