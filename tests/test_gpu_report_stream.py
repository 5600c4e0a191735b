"""FADEHIP_BAM_REPORT_STATS / _CLIP on the file path (Context.bam_stream(..., from_tags=True, no_output=True, report=...)) and
`fade stats --gpus 1` / `fade stats-clip --gpus 1`: the reports of a stream, one piece per call, against report_batch of the
whole and tests/report_file_model.py — records and rows that span calls, a failure named by its index in the stream, the
golden BAM files through the command line."""
import gzip
import os
import struct
import subprocess

import pytest

import fade_amd
import report_cases as rc
import report_file_model as M
import stats_report_ref as R
import tags_model as tm
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import _bam_of
from test_gpu_cli_out_device import big  # noqa: F401  (the fixture: 30,000 reads annotated by the same build)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
HEADER = {"stats": R.STATS_HEADER.encode() + b"\n", "clip": R.CLIP_HEADER.encode() + b"\n"}


def _stream(ctx, names, payload, cut, report):
    """The payload through a report stream in calls of `cut` bytes: ({which: text}, {which: rows}, calls)."""
    which = ("stats", "clip") if report == "both" else (report,)
    st = ctx.bam_stream(names, from_tags=True, no_output=True, report=report)
    try:
        text, rows, calls = {w: [] for w in which}, {w: 0 for w in which}, 0
        edges = list(range(0, len(payload), cut)) + [len(payload)]
        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(payload[a:b], last=(j == len(edges) - 2))
            assert st.back() == b""
            calls += 1
            for w in which:
                t, n = st.report(w)
                assert t.count(b"\n") == n
                text[w].append(t)
                rows[w] += n
        return {w: b"".join(text[w]) for w in which}, rows, calls
    finally:
        st.close()


@pytest.fixture(scope="module")
def whole(ctx):
    """report_batch of the 600 hand-built records, held to the model"""
    recs = rc.good_records()
    got = dict(zip(("stats", "clip"), ctx.report_batch(recs, rc.NAMES, "both")))
    for w in got:
        assert got[w] == M.report_text(recs, rc.NAMES, w)
    return got


@pytest.mark.parametrize("cut,report", [(1000, "both"), (7919, "both"), (7919, "stats"), (1000, "clip"), (1 << 30, "both")])
def test_records_and_rows_that_span_calls(ctx, whole, cut, report):
    payload = b"".join(rc.good_records())
    text, rows, calls = _stream(ctx, rc.NAMES, payload, cut, report)
    assert calls == (len(payload) + cut - 1) // cut
    for w in text:
        assert text[w] == whole[w] and rows[w] == whole[w].count(b"\n")


def test_a_failure_is_named_by_its_index_in_the_stream_and_the_flags_are_held_to_their_rules(ctx):
    recs = rc.good_records()[:400]
    recs.insert(300, rc.FAILURES["ab_short"][2])
    payload = b"".join(recs)
    st = ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, report="stats")
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            for a in range(0, len(payload), 7919):
                st.front_raw(payload[a:a + 7919], last=a + 7919 >= len(payload))
                st.back()
        assert e.value.code == -1 and "record 300:" in str(e.value), str(e.value)
    finally:
        st.close()
    for kw in (dict(from_tags=True), dict(no_output=True), dict(from_tags=True, no_output=True, clip=True), dict(from_tags=True, no_output=True, extract=True)):
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.bam_stream(rc.NAMES, report="stats", **kw)
        assert e.value.code == -1
    st = ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True, stored=True, report="clip")
    try:
        for w in ("clip", "stats"):  # before any back; and the report the stream was not opened for
            with pytest.raises(fade_amd.FadeHipError) as e:
                st.report(w)
            assert e.value.code == -6
        st.front_raw(b"", last=True)
        assert st.back() == b"" and st.report("clip") == (b"", 0)
    finally:
        st.close()
    st = ctx.bam_stream(rc.NAMES, from_tags=True, no_output=True)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            st.report("stats")
        assert e.value.code == -6
    finally:
        st.close()


def _bam_records(data):
    """A BAM file's bytes -> (contig names, the records' bytes, block_size first)"""
    raw = gzip.decompress(data)
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    # (the reference list, entry by entry)
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, at)[0]
        names.append(raw[at + 4:at + 4 + ln - 1].decode())
        at += 8 + ln
    recs = []
    while at < len(raw):
        bs = struct.unpack_from("<I", raw, at)[0]
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    return names, recs


@pytest.fixture(scope="module")
def golden_bams(tmp_path_factory):
    """the three annotated golden sets as BAM files, with their contig names and record bytes"""
    d = tmp_path_factory.mktemp("report_cli")
    out = {}
    for tag in ("anno_c1", "anno_c2", "anno_c5"):
        sam, bam = d / (tag + ".sam"), d / (tag + ".bam")
        sam.write_text(_annotated_sam(tag))
        _bam_of(sam, bam)
        out[tag] = (str(bam),) + _bam_records(bam.read_bytes())
    return out


@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("tag", ["anno_c1", "anno_c2", "anno_c5"])
def test_cli_on_the_golden_bams_equals_the_model_line_for_line(golden_bams, tmp_path, tag, inflate):
    bam, bnames, bams = golden_bams[tag]
    assert M.report_text(bams, bnames, "stats") == M.report_text(tm.annotated(tag)[2], bnames, "stats")
    env = dict(os.environ, FADE_BAM_INFLATE=inflate)
    for sub, which in (("stats", "stats"), ("stats-clip", "clip")):
        want = HEADER[which] + M.report_text(bams, bnames, which)
        p = subprocess.run([FADE, sub, "--gpus", "1", bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout.split(b"\n") == want.split(b"\n")
        named = tmp_path / (sub + ".tsv")
        p = subprocess.run([FADE, sub, "--gpus", "1", "-t", "2", bam, str(named)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode == 0 and p.stdout == b"" and named.read_bytes() == want, p.stderr.decode()
    assert want.count(b"\n") > 20


def test_cli_on_a_bam_of_a_header_alone_writes_the_header_line(golden_bams, tmp_path):
    sam, bam = tmp_path / "h.sam", tmp_path / "h.bam"
    sam.write_text("".join(l + "\n" for l in _annotated_sam("anno_c1").splitlines() if l.startswith("@")))
    _bam_of(sam, bam)
    for sub, which in (("stats", "stats"), ("stats-clip", "clip")):
        p = subprocess.run([FADE, sub, "--gpus", "1", str(bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and p.stdout == HEADER[which], p.stderr.decode()


def test_cli_equals_the_files_annotate_wrote_in_the_same_run(tmp_path):
    """One `fade annotate -b --stats-tsv --clip-tsv` run: the host formats the two reports from the run's own results; the
    device then formats them again from the tags that run wrote."""
    gold = os.path.join(ROOT, "tests", "golden")
    for tag in ("anno_c1", "anno_c2", "anno_c5"):
        prm = dict(kv.split("=") for line in open(os.path.join(gold, tag + ".expected.tsv")) if line.startswith("#floor_len") for kv in line[1:].split())
        bam, anno, st, cl = tmp_path / (tag + ".bam"), tmp_path / (tag + ".anno.bam"), tmp_path / (tag + ".stats.tsv"), tmp_path / (tag + ".clip.tsv")
        _bam_of(os.path.join(gold, tag + ".sam"), bam)
        with open(anno, "wb") as fo:
            subprocess.check_call([FADE, "annotate", "--min-length", prm["floor_len"], "-w", prm["window"], "-b", "--stats-tsv", str(st), "--clip-tsv", str(cl),
                                   str(bam), os.path.join(gold, tag + ".fa")], stdout=fo, stderr=subprocess.DEVNULL, timeout=300)
        for sub, path in (("stats", st), ("stats-clip", cl)):
            p = subprocess.run([FADE, sub, "--gpus", "1", str(anno)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            assert p.returncode == 0 and p.stdout == path.read_bytes() and p.stdout.count(b"\n") > 20, (tag, sub, p.stderr.decode())


def test_30000_annotated_reads_in_many_calls_rows_in_order_and_equal_to_the_model(big):
    names, bams = _bam_records(big.read_bytes())
    env = dict(os.environ, FADE_BAM_CHUNK_MB="1", FADE_BAM_INFLATE="host", FADEHIP_BAM_PROF="1")
    for sub, which, floor in (("stats", "stats", 100), ("stats-clip", "clip", 1000)):
        want = HEADER[which] + M.report_text(bams, names, which)
        assert want.count(b"\n") - 1 >= floor
        p = subprocess.run([FADE, sub, "--gpus", "1", str(big)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert p.returncode == 0 and p.stdout == want, p.stderr.decode()[-2000:]
        calls = [int(l.split()[2]) for l in p.stderr.decode().splitlines() if l.startswith("[fadehip bam] ") and "front calls" in l]
        assert calls and calls[0] >= 5, p.stderr.decode()[-2000:]
