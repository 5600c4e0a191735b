"""The two repeat-overlap columns of `fade stats` on the device — fadehip_report_batch_repeats / Context.report_batch(...,
repeats=set), FADEHIP_BAM_REPORT_REPEATS on the file path, `fade stats --gpus 1 --repeats BED` — against
tests/report_file_model.py's rows with tests/intervals_model.py's two columns appended, byte for byte.  The BED is built from
the model's own rows: for every row an interval that touches, overlaps by one base, or misses each of its two regions."""
import os
import random
import subprocess

import pytest

import fade_amd
import intervals_model as im
import report_cases as rc
import report_file_model as M
import stats_report_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")
ABSENT = "chrUn_KI270742v1"  # a contig the header of report_cases does not carry, and the BED does


def _near(rng, a, b):
    """an interval (start, end) that touches [a, b) on either side, shares exactly one base with it on either side, or
    misses it — whichever of those 0 <= start < end allows (a region that starts below 0 cannot be met from the left)"""
    w = rng.choice([1, 3, 40])
    ways = [(b + 1000, b + 1000 + w)] if b + 1000 >= 0 else []
    if a > 0:
        ways.append((max(0, a - w), a))  # touches on the left
    if b >= 0:
        ways.append((b, b + w))  # touches on the right
    if a >= 0 and a < b:
        ways.append((max(0, a - w), a + 1))  # one base on the left
    if b >= 1 and a < b:
        ways.append((b - 1, b + w))  # one base on the right
    return rng.choice(ways) if ways else (0, 1)


def bed_of_rows(rows, seed, extra=()):
    """[(name, start, end)] drawn by seed from stats rows (bytes): one interval per region of every row"""
    rng = random.Random(seed)
    out = list(extra)
    for row in rows:
        c = row.split(b"\t")
        for name, a, b in ((c[1], int(c[4]), int(c[5])), (c[6], int(c[7]), int(c[8]))):
            out.append((name,) + _near(rng, a, b))
    rng.shuffle(out)
    return out


def model_of(bed):
    m = im.IntervalModel()
    for name, _, _ in bed:
        if im._b(name) not in m.by_name:
            m.name(name)
    m.add(bed)
    return m


def device_set(ctx, bed):
    names = []
    for name, _, _ in bed:
        if im._b(name) not in names:
            names.append(im._b(name))
    s = ctx.intervalset(names)
    s.add([names.index(im._b(n)) for n, _, _ in bed], [a for _, a, _ in bed], [b for _, _, b in bed])
    s.seal()
    return s


def extra_record():
    """an artifact whose am side names a contig that the header does not carry"""
    sl = rc._bases(14)
    return rc.rec("absent", "8S50M", rc.aux(b"rsC\x03", ABSENT.encode() + b",40,14M;", sl + b";", rc._like(sl) + b";", b"G" * 14), tid=0, pos=700)


@pytest.fixture(scope="module")
def case(ctx):
    """the 600 hand-built records and one more; the model's rows; the BED drawn from them; both as a set on the device"""
    recs = rc.good_records() + [extra_record()]
    rows = M.stats_rows(recs, rc.NAMES)
    # (the BED also holds an interval right on the absent contig's region)
    bed = bed_of_rows([r for _, _, r in rows], 20261021, extra=[(ABSENT, 45, 50)])
    model = model_of(bed)
    want = [(k, side, row + im.rpm_columns(model, row)) for k, side, row in rows]
    s = device_set(ctx, bed)
    yield dict(recs=recs, rows=rows, bed=bed, model=model, want=want, set=s)
    s.close()


def _text(rows):
    return b"".join(r + b"\n" for _, _, r in rows)


def test_the_hand_built_records_in_one_call(ctx, case):
    got = ctx.report_batch(case["recs"], rc.NAMES, "stats", repeats=case["set"])
    lines = got.split(b"\n")[:-1]
    assert len(lines) == len(case["want"])
    for (k, side, row), line in zip(case["want"], lines):
        assert line == row, ((rc.LABELS + ["absent"])[k], side, line, row)
    assert got == _text(case["want"])
    # the first 21 columns are the call without a set, byte for byte
    plain = ctx.report_batch(case["recs"], rc.NAMES, "stats")
    assert plain == _text(case["rows"]) and [l.rsplit(b"\t", 2)[0] for l in lines] == plain.split(b"\n")[:-1]
    # both columns take both values, and the cases the rule names are among the rows
    cols = [tuple(l.split(b"\t")[21:]) for l in lines]
    assert {c[0] for c in cols} == {b"0", b"1"} and {c[1] for c in cols} == {b"0", b"1"} and all(len(c) == 2 for c in cols)
    by_label = {(rc.LABELS + ["absent"])[k]: l.split(b"\t") for (k, _, _), l in zip(case["want"], lines)}
    assert int(by_label["pos_0_left_clip"][4]) == -8 and by_label["name_1"][1] == b"c" and by_label["name_40"][1] == b"n" * 40
    assert by_label["cigar_inner_S"][6] == b"c" and int(by_label["cigar_inner_S"][7]) == -3 and by_label["right_only"][6] == b"chr10"
    # art_rpm follows the NAME in am: the absent contig's interval is hit, through the set's own names
    assert by_label["absent"][6] == ABSENT.encode() and by_label["absent"][22] == b"1" and case["model"].hit(ABSENT, 40, 54)
    # the clip report never changes, and "both" is the two alone
    both = ctx.report_batch(case["recs"][:120], rc.NAMES, "both", repeats=case["set"])
    assert both[1] == ctx.report_batch(case["recs"][:120], rc.NAMES, "clip") and both[0] == _text([w for w in case["want"] if w[0] < 120])


def test_every_artifact_record_alone_against_a_bed_drawn_from_its_own_rows(ctx, case):
    """The hand-built records share their regions (most lie at chr1:92-100 with an am side at chr1:40), so in one BED for all of
    them the hits of one row's interval cover the others.  Here every record meets a set drawn from its own rows alone: each
    touch, each single base of overlap and each miss decides a column by itself."""
    seen = {0: [], 1: []}
    for k in sorted({k for k, _, _ in case["rows"]}):
        rows = [r for j, _, r in case["rows"] if j == k]
        bed = bed_of_rows(rows, 1000 + k)
        model = model_of(bed)
        s = device_set(ctx, bed)
        try:
            got = ctx.report_batch([case["recs"][k]], rc.NAMES, "stats", repeats=s)
        finally:
            s.close()
        assert got == b"".join(r + im.rpm_columns(model, r) + b"\n" for r in rows), (rc.LABELS + ["absent"])[k]
        for line in got.split(b"\n")[:-1]:
            c = line.split(b"\t")
            seen[0].append(c[21])
            seen[1].append(c[22])
    for col in (0, 1):
        assert min(seen[col].count(b"0"), seen[col].count(b"1")) >= 10, seen


def test_an_empty_set_and_a_set_without_the_headers_names_give_zeros(ctx, case):
    for names in ([], ["elsewhere"]):
        s = ctx.intervalset(names)
        if names:
            s.add([0], [0], [im.MAX_END])
        s.seal()
        try:
            got = ctx.report_batch(case["recs"][:200], rc.NAMES, "stats", repeats=s)
            assert got == b"".join(r + b"\t0\t0\n" for k, _, r in case["rows"] if k < 200) and got
        finally:
            s.close()
    s = ctx.intervalset(["chr1"])
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:  # not sealed
            ctx.report_batch(case["recs"][:5], rc.NAMES, "stats", repeats=s)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ctx.report_batch(case["recs"][:5], rc.NAMES, "clip", repeats=s)
    finally:
        s.close()


def _stream(ctx, payload, cut, **kw):
    st = ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, **kw)
    try:
        text, rows = {"stats": [], "clip": []}, 0
        edges = list(range(0, len(payload), cut)) + [len(payload)]
        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(payload[a:b], last=(j == len(edges) - 2))
            assert st.back() == b""
            for w in ("stats", "clip") if kw["report"] == "both" else (kw["report"],):
                t, n = st.report(w)
                assert t.count(b"\n") == n
                text[w].append(t)
                rows += n
        return {w: b"".join(t) for w, t in text.items()}
    finally:
        st.close()


@pytest.mark.parametrize("cut,report", [(1000, "stats"), (7919, "both"), (1 << 30, "stats")])
def test_the_stream_in_cuts_equals_the_batch(ctx, case, cut, report):
    """(the artifact rows at records 255, 256, 257 and 511, 512 lie at the edges of a block of records, as they do today)"""
    payload = b"".join(case["recs"])
    got = _stream(ctx, payload, cut, report=report, repeats=case["set"])
    assert got["stats"] == _text(case["want"])
    assert {255, 256, 257, 511, 512} <= {k for k, _, _ in case["want"]}
    if report == "both":
        assert got["clip"] == ctx.report_batch(case["recs"], rc.NAMES, "clip") and got["clip"]


def test_the_flag_without_a_set_fails_the_first_front_and_without_report_stats_the_open(ctx, case):
    st = ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, report="stats", repeats=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.front_raw(b"".join(case["recs"][:10]), last=True)
        assert e.value.code == -6 and "fadehip_bam_use_intervals" in str(e.value)
    finally:
        st.close()
    for kw in (dict(report="clip"), dict()):
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, repeats=True, **kw)
        assert e.value.code == -1 and "FADEHIP_BAM_REPORT_REPEATS" in str(e.value)
    s = ctx.intervalset(["chr1"])  # a set that has not been sealed is not attached
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, report="stats", repeats=s)
        assert e.value.code == -1 and "sealed" in str(e.value)
    finally:
        s.close()
    # without the flag the stream is what it was
    assert _stream(ctx, b"".join(case["recs"]), 7919, report="stats")["stats"] == _text(case["rows"])


def test_the_command_line_on_a_golden_bam_annotated_by_the_same_build(tmp_path):
    tag = "anno_c5"
    prm = dict(kv.split("=") for line in open(os.path.join(GOLD, tag + ".expected.tsv")) if line.startswith("#floor_len") for kv in line[1:].split())
    bam, anno = tmp_path / "in.bam", tmp_path / "anno.bam"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "sam2bam"])
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), os.path.join(GOLD, tag + ".sam")], stdout=fo)
    with open(anno, "wb") as fo:
        subprocess.check_call([FADE, "annotate", "--min-length", prm["floor_len"], "-w", prm["window"], "-b", str(bam), os.path.join(GOLD, tag + ".fa")], stdout=fo,
                              stderr=subprocess.DEVNULL, timeout=300)
    plain = subprocess.run([FADE, "stats", "--gpus", "1", str(anno)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    lines = plain.stdout.split(b"\n")
    assert lines[0] == R.STATS_HEADER.encode() and lines[-1] == b"" and len(lines) > 22
    rows = lines[1:-1]
    bed = bed_of_rows(rows, 7)
    model = model_of(bed)
    f = tmp_path / "rmsk.bed"
    f.write_bytes(b"#chrom\tstart\tend\n" + im.bed_text(bed))
    want = [lines[0] + b"\tread_rpm\tart_rpm"] + [r + im.rpm_columns(model, r) for r in rows] + [b""]
    p = subprocess.run([FADE, "stats", "--gpus", "1", "--repeats", str(f), str(anno)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    got = p.stdout.split(b"\n")
    assert len(got[0].split(b"\t")) == 23 and got == want
    assert {g.split(b"\t")[21] for g in got[1:-1]} == {b"0", b"1"} and {g.split(b"\t")[22] for g in got[1:-1]} == {b"0", b"1"}
    named = tmp_path / "out.tsv"
    p2 = subprocess.run([FADE, "stats", "--gpus", "1", "--timing", "--repeats=" + str(f), str(anno), str(named)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p2.returncode == 0 and p2.stdout == b"" and named.read_bytes() == p.stdout, p2.stderr.decode()
    assert b"[timing] --repeats: %d intervals" % len(bed) in p2.stderr
    # a BED that does not parse is refused with its line, and leaves no report behind
    f.write_bytes(b"chr1\t1\t2\nchr1\t2\t2\n")
    never = tmp_path / "never.tsv"
    p3 = subprocess.run([FADE, "stats", "--gpus", "1", "--repeats", str(f), str(anno), str(never)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p3.returncode == 1 and p3.stdout == b"" and b"line 2: start is not below end" in p3.stderr, p3.stderr.decode()
