"""FADEHIP_BAM_FROM_TAGS on the file path (Context.bam_stream(..., from_tags=True)): `fade out -c`, plain `fade out` and
`fade extract` over records that were annotated earlier, rs and am read back on the device.  front_raw + stored members
unless said.  The expectations use no GPU: oracle/pyfilter.fade_out and oracle/pyremap.extract_records on the annotated golden
sets, the host loops of the `fade` binary for the bytes, and tests/tags_model.py with its restatements (clip_by_trims,
eject_keep) on constructed records."""
import gzip
import random
import struct

import pytest

import fade_amd
import clip_cases as cc
import samutil
import tags_model as tm
from oracle import pyfilter, pyremap
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import _bam_of, _ok, _run, _split
from test_gpu_bam_stream import _members
from test_gpu_tags_batch import CASES, NAMES, SEQ, _z

pytestmark = pytest.mark.gpu

SETS = ["anno_c1", "anno_c2", "anno_c5", "anno_floor0"]


# ---------------------------------------------------------------------------------------------- helpers
def _offsets(payload):
    off, at = [], 0
    while at < len(payload):
        off.append(at)
        at += 4 + struct.unpack_from("<I", payload, at)[0]
    assert at == len(payload)
    return off + [at]


def _records(payload):
    off = _offsets(payload)
    return [bytes(payload[a:b]) for a, b in zip(off, off[1:])]


def _records_of_bam_body(body):
    """_split's body (the reference list, then the records) -> the records' bytes."""
    at = 4
    for _ in range(struct.unpack_from("<i", body, 0)[0]):
        at += 8 + struct.unpack_from("<i", body, at)[0]
    return bytes(body[at:])


def _stream(ctx, names, payload, cuts=(), **modes):
    """The payload through a FROM_TAGS stream, cut at the given offsets: dict(out, x, n_x, ejected, per_call, totals)."""
    st = ctx.bam_stream(names, floor_len=-3, window=-1, stored=True, from_tags=True, **modes)
    try:
        edges = [0] + sorted(cuts) + [len(payload)]
        out, xs, per_call, n_x = [], [], [], 0
        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(payload[a:b], last=(j == len(edges) - 2))
            piece = st.back()
            piece = gzip.decompress(piece) if piece else b""
            out.append(piece)
            per_call.append(len(_offsets(piece)) - 1)
            if modes.get("extract"):
                x, n = st.back_extract()
                xs.append(x)
                n_x += n
        return dict(out=b"".join(out), x=b"".join(xs), n_x=n_x, ejected=st.ejected(), per_call=per_call, totals=st.totals())
    finally:
        st.close()


def _stats_of(rs, have):
    """stats.d:45-54 as fadehip_bam_totals sums it: read_count over every record, the rest over records with an integer rs."""
    st = [len(rs)] + [0] * 7
    for v, h in zip(rs, have):
        if not h & 1:
            continue
        v = int(v)
        sc, al, ar, ml, mr, su = v & 1, (v >> 1) & 1, (v >> 2) & 1, (v >> 3) & 1, (v >> 4) & 1, (v >> 5) & 1
        for k, add in enumerate((sc, su, (al | ar) & su, al | ar, (al & ml) | (ar & mr), al, ar)):
            st[k + 1] += add
    return st


def _third_field_ref(text):
    """filter.d:24-25: the reference bases of the CIGAR behind a side's second comma, None when there is none or it does not parse."""
    f = text.split(b",", 2)
    if len(f) < 3:
        return None
    n, at = 0, 0
    for m in tm._PAIR.finditer(f[2]):
        if m.start() != at or int(m.group(1)) >= 1 << 28:
            return None
        if tm.OPS.index(m.group(2).decode()) in tm.REF_OPS:
            n += int(m.group(1))
        at = m.end()
    return None if at != len(f[2]) else min(n, tm.INT32_MAX)


def _clip_trims(rec, names):
    """(rs or None without an integer rs, [left, right] trims with None where a side whose bit is set does not give one)"""
    t = tm.read_tags(rec, names)
    if not t["have"] & 1:
        return None, [0, 0]
    fields = {}
    for tag, ty, val in tm.aux_fields(bytes(rec[tm.aux_offset(rec):])):
        fields.setdefault(tag, (ty, val))
    am = fields[b"am"][1][:-1] if b"am" in fields and fields[b"am"][0] == "Z" else None
    cut = (am.split(b";", 1) + [b""])[:2] if am is not None else [None, None]
    trims = [0, 0]
    for side in range(2):
        if t["rs"] & (2 << side):
            trims[side] = None if cut[side] is None else _third_field_ref(cut[side])
    return t["rs"], trims


def _clip_expect(rec, rs, tl, tr, names):
    """filter.d:15-91 on the bytes of one record by tags_model.clip_by_trims: the aux bytes stay, a reset record has none."""
    d = cc.decode_rec(rec)
    src = dict(qname=d["qname"], cigar=d["cigar"], pos=d["pos"], seq=d["seq"], qual=d["qual"], whole=True)
    new = tm.clip_by_trims(src, rs, tl, tr, names[0])
    if "whole" not in new:  # reset
        return cc.build_rec(d["qname"], 0, 0, 0, 0, 0, 0, 0, "*", new["seq"], new["qual"], b"")
    return cc.build_rec(d["qname"], d["tid"], new["pos"], d["mapq"], d["flag"], d["mtid"], d["mpos"], d["tlen"], new["cigar"], new["seq"], new["qual"], d["aux"])


def _extract_expect(rec, t, k):
    """remap.d:29-85 on the bytes of one record from the model's arrays: its extract records, left before right."""
    d = cc.decode_rec(rec)
    out = []
    for side in range(2):
        if t["have"][k] & 1 and t["have"][k] & 2 and t["rs"][k] & (2 << side):
            s = 2 * k + side
            cigar = "".join("%d%s" % (x >> 4, tm.OPS[x & 15]) for x in t["cig"][t["cig_off"][s]:t["cig_off"][s + 1]]) or "*"
            out.append(cc.build_rec(d["qname"], int(t["art_tid"][s]), int(t["art_pos"][s]), 0, 0 if d["flag"] & 0x10 else 0x10, 0, 0, 0, cigar,
                                    pyremap.reverse_complement(d["seq"]), d["qual"][::-1], b""))
    return out


def _refused(ctx, names, payload, index, **modes):
    with pytest.raises(fade_amd.FadeHipError) as e:
        _stream(ctx, names, payload, **modes)
    assert e.value.code == -1 and ("record %d:" % index) in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------- the flag
def test_the_stream_opens_with_the_flag_and_clip_with_eject_stays_refused(ctx):
    from fade_amd import _lib
    assert _lib.BAM_FROM_TAGS == 64
    st = ctx.bam_stream(["c"], from_tags=True)
    st.close()
    for eject in ("records", "groups"):
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.bam_stream(["c"], clip=True, eject=eject, from_tags=True)
        assert e.value.code == -1
    # an empty stream: one last call without a byte
    r = _stream(ctx, ["c"], b"", clip=True)
    assert r["out"] == b"" and r["totals"][0] == [0] * 8 and r["totals"][1] == 0


# ---------------------------------------------------------------------------------------------- golden sets
def _shuffled(lines):
    head = [l for l in lines if l.startswith("@")]
    body = [l for l in lines if not l.startswith("@")]
    rng = random.Random(20261019)
    while True:
        rng.shuffle(body)
        first = [l.split("\t")[0] for l in body[:10]]
        if any(pyfilter.numerically_aware_cmp(first[k], first[k - 1]) < 0 for k in range(1, 10)):
            return head + body


@pytest.fixture(scope="module", params=[(t, o) for t in SETS for o in ("sorted", "shuffled")], ids=lambda p: "%s-%s" % p)
def gold(request, tmp_path_factory):
    """An annotated golden set as SAM text, as the record bytes a BAM of it holds, and what the host loops make of it."""
    tag, order = request.param
    d = tmp_path_factory.mktemp("fromtags_%s_%s" % (tag, order))
    lines = _annotated_sam(tag).splitlines()
    if order == "shuffled":
        lines = _shuffled(lines)
    sam, bam = d / "anno.sam", d / "anno.bam"
    sam.write_text("\n".join(lines) + "\n")
    _bam_of(sam, bam)
    header, recs = samutil.parse_sam(sam.read_text())
    names = [dict(x.split(":", 1) for x in h.split("\t")[1:])["SN"] for h in header if h.startswith("@SQ")]
    payload = _records_of_bam_body(_split(bam.read_bytes())[1])
    host = {k: _records_of_bam_body(_split(_ok(_run(a + ["-u", str(sam)])).stdout)[1]) for k, a in (("clip", ["out", "-c"]), ("out", ["out"]), ("extract", ["extract"]))}
    return dict(tag=tag, order=order, names=names, recs=recs, payload=payload, host=host, bam=bam)


def test_golden_sets_every_mode_equals_the_oracle_and_the_host_loops(ctx, gold):
    names, recs, payload = gold["names"], gold["recs"], gold["payload"]
    bams = _records(payload)
    assert [tm.bam_to_line(b, names) for b in bams] == [pyfilter._fmt(r) for r in recs]
    rs = [int(r["tags"]["rs"][1]) for r in recs]
    assert sum(1 for v in rs if v & 6) >= 6 and any(v & 2 for v in rs) and any(v & 4 for v in rs)
    want_stats = _stats_of(rs, [1] * len(rs))
    lines = lambda b: [tm.bam_to_line(x, names) for x in _records(b)]
    # the flag alone: every record passes byte for byte
    r = _stream(ctx, names, payload)
    assert r["out"] == payload and r["ejected"] == 0 and r["totals"][:2] == (want_stats, len(recs))
    # fade out -c
    r = _stream(ctx, names, payload, clip=True)
    assert lines(r["out"]) == pyfilter.fade_out(recs, names[0], clip=True)[0]
    assert r["out"] == gold["host"]["clip"] and r["totals"][:2] == (want_stats, len(recs))
    # fade out: the mode the first ten names give
    grouped = gold["order"] == "sorted"
    want = pyfilter.fade_out(recs, names[0], clip=False)[0]
    r = _stream(ctx, names, payload, eject="groups" if grouped else "records")
    assert lines(r["out"]) == want and 0 < len(want) < len(recs)
    assert r["out"] == gold["host"]["out"] and r["ejected"] == len(recs) - len(want) and r["totals"][:2] == (want_stats, len(recs))
    # fade extract
    want = pyremap.extract_records(recs, names)
    r = _stream(ctx, names, payload, extract=True, no_output=True)
    assert lines(r["x"]) == want and r["n_x"] == len(want) >= 6 and r["out"] == b""
    assert r["x"] == gold["host"]["extract"] and r["totals"][:2] == (want_stats, len(recs))


def test_one_run_through_front_inflates_the_members_on_the_device(ctx, gold):
    names = gold["names"]
    members = _members(gold["bam"].read_bytes())
    hdr = len(gzip.decompress(gold["bam"].read_bytes())) - len(gold["payload"])
    cum = 0
    while cum + len(gzip.decompress(members[0])) <= hdr:  # whole members of the header
        cum += len(gzip.decompress(members.pop(0)))
    st = ctx.bam_stream(names, first_record=hdr - cum, stored=True, clip=True, extract=True, from_tags=True)
    try:
        half = max(1, len(members) // 2)
        out, xs = [], []
        for j, part in enumerate((members[:half], members[half:])):
            st.front(b"".join(part), last=j == 1)
            piece = st.back()
            out.append(gzip.decompress(piece) if piece else b"")
            xs.append(st.back_extract()[0])
        assert b"".join(out) == gold["host"]["clip"] and b"".join(xs) == gold["host"]["extract"]
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------- constructed records
# tests/test_gpu_tags_batch.py's aux areas, and behind them the ones that read rs or am alone (sides, names, positions, CIGARs)
# once more with rs 6 in front: both sides are asked for
ALL = CASES + [(lab + "+rs6", tid, b"rsC\x06" + aux) for lab, tid, aux in CASES if lab.startswith(("cig_", "pos_", "name_"))]


def _grec(k, tid, aux):
    """tests/test_gpu_tags_batch.py's record with names in groups of three (g0 g0 g0 g1 ...)."""
    lq = k % len(SEQ) + 1
    return cc.build_rec("g%d" % (k // 3), tid, 100 + k, 30, 16 * (k % 2), -1, -1, 0, "%dM" % lq, SEQ[:lq], "I" * lq, aux)


def _clip_case_records():
    """tests/clip_cases.py's records with the case's rs and its trims written as am CIGARs behind the case's aux bytes."""
    out = []
    for c in cc.cases():
        am = c["rec"]["tags"]["am"][1].encode()
        out.append(cc.to_bam(c["rec"], c["aux"] + b"rsC" + bytes([c["rs"]]) + _z(b"am", am)))
    return out


def test_clip_cases_with_the_trims_written_as_am_cigars(ctx):
    recs = _clip_case_records()
    names = cc.CONTIGS
    by = {c["name"]: k for k, c in enumerate(cc.cases())}
    want = []
    for k, (b, c) in enumerate(zip(recs, cc.cases())):
        rs, trims = _clip_trims(b, names)
        assert rs == c["rs"] and trims == [c["tl"] if rs & 2 else 0, c["tr"] if rs & 4 else 0]
        want.append(_clip_expect(b, rs, trims[0], trims[1], names) if rs & 6 else b)
    # a reset on the left, a reset on the right after a left clip, aux areas of several KB: they are there, and they differ
    for lab in ("reset_left_equal", "reset_right_after_left", "long_reset_big_aux"):
        assert struct.unpack_from("<H", want[by[lab]], 16)[0] == 0 and len(want[by[lab]]) < len(recs[by[lab]])
    assert len(recs[by["long_both_big_aux"]]) > 3000 and want[by["long_both_big_aux"]][-3000:] == recs[by["long_both_big_aux"]][-3000:]
    r = _stream(ctx, names, b"".join(recs), clip=True)
    got = _records(r["out"])
    bad = [(cc.cases()[k]["name"], k) for k in range(len(recs)) if got[k] != want[k]]
    assert not bad and len(got) == len(recs), bad[:5]
    assert r["totals"][0] == _stats_of([c["rs"] for c in cc.cases()], [1] * len(recs))


def _model(recs):
    return tm.tags_batch(recs, NAMES)


def test_constructed_aux_areas_clip_passes_what_it_can_and_names_what_it_cannot(ctx):
    recs = [_grec(k, tid, aux) for k, (_, tid, aux) in enumerate(ALL)]
    by = {lab: k for k, (lab, _, _) in enumerate(ALL)}
    plan = [_clip_trims(b, NAMES) for b in recs]
    fails = [k for k, (rs, tr) in enumerate(plan) if None in tr]
    good = [k for k in range(len(recs)) if k not in fails]
    # what the issue names: no rs and rs:Z pass, a junk position passes, a missing side CIGAR / no am / am:i on a set bit fail
    assert all(plan[by[x]][0] is None for x in ("rs_Z", "rs_none", "no_aux", "rs_A", "rs_f"))
    assert by["pos_12a+rs6"] in good and by["pos_empty+rs6"] in good and plan[by["pos_12a+rs6"]][1] == [3, 0]
    assert all(by[x] in fails for x in ("am_absent", "am_i", "am_empty", "am_left_only", "am_right_only", "am_no_semicolon", "rs_last", "cig_lower+rs6",
                                        "cig_left_bad_right_good+rs6", "cig_third_comma+rs6", "name_own+rs6"))
    assert by["cig_lower"] in good and len(fails) >= 20 and len(good) >= 60
    want = [_clip_expect(recs[k], plan[k][0], plan[k][1][0], plan[k][1][1], NAMES) if plan[k][0] is not None and plan[k][0] & 6 else recs[k] for k in good]
    r = _stream(ctx, NAMES, b"".join(recs[k] for k in good), clip=True)
    got = _records(r["out"])
    bad = [ALL[k][0] for j, k in enumerate(good) if got[j] != want[j]]
    assert not bad and len(got) == len(good), bad[:5]
    assert sum(1 for a, k in zip(want, good) if a != recs[k]) >= 15
    # every failing record, each at another index among good ones; two in one call: the first is named
    for j, k in enumerate(fails):
        at = j % 7
        _refused(ctx, NAMES, b"".join([recs[g] for g in good[:at]] + [recs[k]] + [recs[g] for g in good[at:at + 3]]), at, clip=True)
    _refused(ctx, NAMES, b"".join([recs[good[0]], recs[good[1]], recs[fails[0]], recs[good[2]], recs[fails[1]]]), 2, clip=True)
    # a record index counts over the calls of the stream
    payload = b"".join([recs[good[0]], recs[good[1]], recs[fails[0]]])
    with pytest.raises(fade_amd.FadeHipError) as e:
        _stream(ctx, NAMES, payload, cuts=[len(recs[good[0]])], clip=True)
    assert "record 2:" in str(e.value)


def test_constructed_aux_areas_eject_records_groups_and_the_flag_alone(ctx):
    recs = [_grec(k, tid, aux) for k, (_, tid, aux) in enumerate(ALL)]
    by = {lab: k for k, (lab, _, _) in enumerate(ALL)}
    t = _model(recs)
    payload = b"".join(recs)
    qn = ["g%d" % (k // 3) for k in range(len(recs))]
    stats = _stats_of(t["rs"], t["have"])
    assert stats[0] == len(recs) and 0 < stats[4] < len(recs) and stats[6] > 0 and stats[7] > 0
    r = _stream(ctx, NAMES, payload)
    assert r["out"] == payload and r["totals"][:2] == (stats, len(recs)) and r["ejected"] == 0
    for grouped in (False, True):
        keep = tm.eject_keep(qn, t["rs"], t["have"], grouped)
        r = _stream(ctx, NAMES, payload, eject="groups" if grouped else "records")
        assert r["out"] == b"".join(b for b, k in zip(recs, keep) if k), grouped
        assert r["ejected"] == len(recs) - sum(keep) > 0 and r["totals"][:2] == (stats, len(recs))
        if not grouped:  # a record without rs is dropped record by record
            assert not t["have"][by["rs_none"]] & 1 and not keep[by["rs_none"]] and not keep[by["no_aux"]] and not keep[by["rs_Z"]]
    # am is never looked at: records whose am is junk leave or stay by rs alone (the calls above did not fail)
    assert t["rs"][by["cig_lower"]] == 0 and t["rs"][by["am_i"]] == 6
    # a group whose only artifact-looking member has no integer rs stays whole
    trio = [_grec(0, 1, b"NMC\x01"), _grec(1, 1, _z(b"rs", b"6")), _grec(2, 1, b"rsC\x01")]
    r = _stream(ctx, NAMES, b"".join(trio), eject="groups")
    assert r["out"] == b"".join(trio) and r["ejected"] == 0
    r = _stream(ctx, NAMES, b"".join(trio), eject="records")
    assert r["out"] == trio[2] and r["ejected"] == 2 and r["totals"][0] == [3, 1, 0, 0, 0, 0, 0, 0]


def _fits_int32(rec):
    t = tm.read_tags(rec, NAMES)
    return all(s is None or -(1 << 31) <= s[1] < (1 << 31) for s in t["sides"])


def test_constructed_aux_areas_extract_builds_the_sides_and_names_a_junk_one(ctx):
    # (a BAM record's pos field holds 32 bits: the sides whose position needs more are fadehip_extract_batch's own cases)
    recs = [_grec(k, tid, aux) for k, (_, tid, aux) in enumerate(ALL) if _fits_int32(_grec(k, tid, aux))]
    labs = [lab for k, (lab, tid, aux) in enumerate(ALL) if _fits_int32(_grec(k, tid, aux))]
    assert len(recs) >= len(ALL) - 12
    by = {lab: k for k, lab in enumerate(labs)}
    t = _model(recs)
    takes = [bool(t["have"][k] & 1 and t["rs"][k] & 6 and t["have"][k] & 2) for k in range(len(recs))]
    fails = [k for k in range(len(recs)) if takes[k] and any(t["rs"][k] & (2 << s) and not t["have"][k] & (4 << s) for s in range(2))]
    good = [k for k in range(len(recs)) if k not in fails]
    assert all(not takes[by[x]] for x in ("rs_Z", "rs_none", "am_absent", "am_i", "am_without_rs")) and takes[by["rs_c"]] and takes[by["am_both"]]
    assert all(by[x] in fails for x in ("am_empty", "am_left_only", "am_right_only", "am_no_semicolon", "pos_12a+rs6", "pos_empty+rs6", "cig_lower+rs6",
                                        "cig_third_comma+rs6", "name_own+rs6")) and len(fails) >= 20
    assert all(by[x] in good and takes[by[x]] for x in ("cig_300+rs6", "cig_empty+rs6", "pos_minus+rs6", "name_other+rs6", "cig_max_count+rs6"))
    sub = [recs[k] for k in good]
    ts = _model(sub)
    want = [x for j in range(len(sub)) for x in _extract_expect(sub[j], ts, j)]
    assert len(want) >= 12 and any(struct.unpack_from("<i", x, 4)[0] == -1 for x in want)
    r = _stream(ctx, NAMES, b"".join(sub), extract=True)
    got = _records(r["x"])
    assert r["out"] == b"".join(sub) and r["n_x"] == len(want) == len(got)
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, (bad[:5], cc.decode_rec(got[bad[0]]), cc.decode_rec(want[bad[0]]))
    for j, k in enumerate(fails):
        at = j % 5
        _refused(ctx, NAMES, b"".join([recs[g] for g in good[:at]] + [recs[k]] + [recs[good[0]]]), at, extract=True, no_output=True)
    # a junk position on a set bit: CLIP passes it (its third field parses), EXTRACT names the record
    junk = [_grec(0, 1, b"rsC\x01"), _grec(1, 1, b"rsC\x02" + _z(b"am", b"chr1,12a,3M;")), _grec(2, 1, b"rsC\x04" + _z(b"am", b";chr1,7,2M"))]
    r = _stream(ctx, NAMES, b"".join(junk), clip=True)
    assert _records(r["out"])[1] == _clip_expect(junk[1], 2, 3, 0, NAMES) and _records(r["out"])[2] == _clip_expect(junk[2], 4, 0, 2, NAMES)
    _refused(ctx, NAMES, b"".join(junk), 1, extract=True)
    # 65,535 ops on a side are built, one more is refused
    many = lambda n: _grec(1, 1, b"rsC\x02" + _z(b"am", b"chr2,9," + b"1M1I" * (n // 2) + b"1M" * (n % 2) + b";"))
    r = _stream(ctx, NAMES, junk[0] + many(65535), extract=True, no_output=True)
    d = cc.decode_rec(_records(r["x"])[0])
    assert r["n_x"] == 1 and d["tid"] == 2 and d["pos"] == 9 and struct.unpack_from("<H", r["x"], 16)[0] == 65535
    _refused(ctx, NAMES, junk[0] + many(65536), 1, extract=True, no_output=True)


# ---------------------------------------------------------------------------------------------- cuts
@pytest.fixture(scope="module")
def cut(ctx):
    """anno_c5's annotated records (a few hundred, name-sorted) in one payload, and the single-call run of every mode."""
    names, recs, bams = tm.annotated("anno_c5")
    payload = b"".join(bams)
    modes = dict(groups=dict(eject="groups"), records=dict(eject="records"), clip=dict(clip=True), extract=dict(extract=True, no_output=True),
                 clip_extract=dict(clip=True, extract=True))
    one = {k: _stream(ctx, names, payload, **m) for k, m in modes.items()}
    assert 200 <= len(bams) and one["groups"]["ejected"] > one["records"]["ejected"] > 0 and one["extract"]["n_x"] >= 10
    return dict(names=names, bams=bams, payload=payload, off=_offsets(payload), modes=modes, one=one, qn=[r["qname"] for r in recs])


def _cuttings(s):
    off, bams, qn = s["off"], s["bams"], s["qn"]
    n = len(bams)
    same = [k for k in range(1, n) if qn[k] == qn[k - 1]]
    with_am = [k for k in range(n) if b"amZ" in bams[k]]
    pair = next(k for k in same if k >= 2 and qn[k - 2] != qn[k] and k + 1 < n and qn[k + 1] != qn[k])  # a group of exactly two
    assert len(same) >= 20 and len(with_am) >= 6
    return {
        "inside_a_record": [off[k] + 17 for k in range(5, n, 37)] + [off[k + 1] - 1 for k in range(11, n, 53)],
        "inside_an_aux_area": [off[k] + tm.aux_offset(bams[k]) + 5 for k in with_am[::2]],
        "inside_the_am_text": [off[k] + bams[k].index(b"amZ") + 9 for k in with_am],
        "between_two_records_of_a_group": [off[k] for k in same[3::5]],
        "a_call_that_is_one_group": [off[pair - 1], off[pair], off[pair + 1]],
        "a_byte_per_call_for_200_bytes": list(range(1, 201)),
    }


@pytest.mark.parametrize("which", ["inside_a_record", "inside_an_aux_area", "inside_the_am_text", "between_two_records_of_a_group",
                                   "a_call_that_is_one_group", "a_byte_per_call_for_200_bytes"])
def test_cuts_change_nothing(ctx, cut, which):
    s = cut
    cuts = sorted(set(_cuttings(s)[which]))
    assert len(cuts) >= 3 and 0 < min(cuts) and max(cuts) < len(s["payload"])
    for mode, kw in s["modes"].items():
        r, one = _stream(ctx, s["names"], s["payload"], cuts=cuts, **kw), s["one"][mode]
        assert (r["out"], r["x"], r["n_x"], r["ejected"], r["totals"]) == (one["out"], one["x"], one["n_x"], one["ejected"], one["totals"]), mode
        assert sum(r["per_call"]) == sum(one["per_call"])
        if mode == "groups" and which == "a_call_that_is_one_group":
            assert r["per_call"][2] == 0  # the call that holds nothing but the carried group's second record yields nothing
        if which == "a_byte_per_call_for_200_bytes":
            assert r["per_call"][:200] == [0] * 200
