"""`fade annotate --extract PATH`: `fade extract`'s records built in the pass that writes the tags (FADEHIP_BAM_EXTRACT on the
file path, the host's build_extract_rec in the host pipeline).  The expectation is oracle/pyremap.extract_records over the
golden records with the golden tags; every format and path must write an extract file that decodes to it, in order, and a
main output that is what the same command gives without the option."""
import gzip
import os
import struct

import numpy as np
import pytest

import fade_amd
import samutil
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import _bam_of, _decode, _norm, _ok, _pg, _run
from test_gpu_bam_stream import _members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WARN = b"[W::fade extract] Output SAM/BAM will not be sorted"
TAGS = ["anno_c1", "anno_c2", "anno_c5"]


def _expected(tag, text=None):
    from oracle import pyremap
    header, in_recs = samutil.parse_sam(text or _annotated_sam(tag))
    names = [h.split("\t")[1][3:] for h in header if h.startswith("@SQ")]
    lines = pyremap.extract_records(in_recs, names)
    _, recs = samutil.parse_sam("\n".join([h for h in header if h.startswith("@SQ")] + lines) + "\n")
    return [_norm(r) for r in recs]


def _opts(tag):
    from test_gpu_cli import _expected as gold
    _, floor_len, window = gold(tag)
    return ["annotate", "--timing", "--min-length", str(floor_len), "-w", str(window)]


def _inputs(tag, tmp_path):
    bam = tmp_path / "in.bam"
    sam = os.path.join(GOLD, tag + ".sam")
    _bam_of(sam, bam)
    return str(bam), sam, os.path.join(GOLD, tag + ".fa")


def _records_of_bam(data):
    raw = gzip.decompress(data)
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    return raw[at:]


@pytest.mark.parametrize("tag", TAGS)
def test_extract_on_the_golden_inputs_every_format_and_path(tmp_path, tag):
    exp = _expected(tag)
    assert len(exp) >= 10
    bam, sam, fa = _inputs(tag, tmp_path)
    base = _opts(tag)
    paths = {
        "dev_inflate": (["-b", bam, fa], {"FADE_BAM_INFLATE": "device"}, "bam", True),
        "host_inflate": (["-b", bam, fa], {"FADE_BAM_INFLATE": "host"}, "bam", True),
        "ubam": (["-u", bam, fa], None, "bam", True),
        "sam_from_bam": ([bam, fa], None, "sam", False),
        "sam_in_sam_out": ([sam, fa], None, "sam", False),
        "host_pipeline_bam": (["-b", bam, fa], {"FADE_BAM_DEVICE": "0"}, "bam", False),
    }
    bodies = []
    for name, (args, env, fmt, on_device) in paths.items():
        x = tmp_path / (name + ".extract")
        p = _ok(_run(base + ["--extract", str(x)] + args, env))
        plain = _ok(_run(base + args, env))
        assert (b"file path on the device" in p.stderr) == on_device, name
        assert p.stderr.count(WARN) == 1 and WARN not in plain.stderr, name
        assert _decode(p.stdout, fmt) == _decode(plain.stdout, fmt), name     # the main output does not know about the option
        data = x.read_bytes()
        head, got = _decode(data, fmt)
        assert head == _decode(plain.stdout, fmt)[0], name                    # the main output's header
        assert len(got) == len(exp), (name, len(got), len(exp))
        bad = [(name, k, a, b) for k, (a, b) in enumerate(zip(got, exp)) if a != b]
        assert not bad, bad[:3]
        pg = [h for h in _pg(data, fmt) if "\tPN:fade\t" in h]  # (the only fade line: annotate's, none of extract)
        assert len(pg) == 1 and "ID:fade-annotate" in pg[0] and "--extract" in pg[0], pg
        if fmt == "bam":
            bodies.append(_records_of_bam(data))
    assert all(b == bodies[0] for b in bodies) and len(bodies) == 4           # device and host build the same bytes


@pytest.mark.parametrize("tag", TAGS)
def test_extract_beside_the_two_step_form_the_clip_and_the_reports(tmp_path, tag):
    bam, sam, fa = _inputs(tag, tmp_path)
    base = _opts(tag)
    x = tmp_path / "x.bam"
    one = _ok(_run(base + ["-b", "--extract", str(x), bam, fa]))
    assert b"file path on the device" in one.stderr
    # annotate -b to a file, then this build's own extract -b on it
    anno = tmp_path / "anno.bam"
    anno.write_bytes(_ok(_run(base + ["-b", bam, fa])).stdout)
    two = _ok(_run(["extract", "-b", str(anno)]))
    assert _records_of_bam(two.stdout) == _records_of_bam(x.read_bytes()) and len(_records_of_bam(two.stdout)) > 0
    # -c --extract: the main output is -c alone, the extract file is the one made without -c (built from the unclipped record)
    for env in (None, {"FADE_BAM_DEVICE": "0"}):
        xc = tmp_path / "xc.bam"
        both = _ok(_run(base + ["-c", "-b", "--extract", str(xc), bam, fa], env))
        clip = _ok(_run(base + ["-c", "-b", bam, fa], env))
        assert (b"file path on the device" in both.stderr) == (env is None)
        assert _records_of_bam(both.stdout) == _records_of_bam(clip.stdout)
        assert _records_of_bam(xc.read_bytes()) == _records_of_bam(x.read_bytes())
        assert both.stderr.count(WARN) == 1
    # --stats-tsv (and --stats) beside it: the report is unchanged
    t1, t2, xs = tmp_path / "a.tsv", tmp_path / "b.tsv", tmp_path / "xs.bam"
    with_x = _ok(_run(base + ["--stats", "-b", "--stats-tsv", str(t1), "--extract", str(xs), bam, fa]))
    without = _ok(_run(base + ["--stats", "-b", "--stats-tsv", str(t2), bam, fa]))
    assert t1.read_bytes() == t2.read_bytes() and len(t1.read_bytes()) > 0
    stats = lambda err: [l for l in err.decode().splitlines() if l.startswith(("read count", "Clipped", "% With", "Artifact"))]
    assert stats(with_x.stderr) == stats(without.stderr) and len(stats(without.stderr)) == 7
    assert _records_of_bam(xs.read_bytes()) == _records_of_bam(x.read_bytes())


def test_an_input_without_artifacts_gives_a_header_only_extract_file(tmp_path):
    tag = "anno_c1"
    lines = open(os.path.join(GOLD, tag + ".sam")).read().splitlines()
    keep = [l for l in lines if l.startswith("@") or ("S" not in l.split("\t")[5] and not int(l.split("\t")[1]) & 4)]
    assert sum(1 for l in keep if not l.startswith("@")) >= 10
    sam, bam = tmp_path / "in.sam", tmp_path / "in.bam"
    sam.write_text("\n".join(keep) + "\n")
    _bam_of(sam, bam)
    fa = os.path.join(GOLD, tag + ".fa")
    for args, env, fmt in ((["-b", str(bam), fa], None, "bam"), (["-b", str(bam), fa], {"FADE_BAM_DEVICE": "0"}, "bam"), ([str(sam), fa], None, "sam")):
        x = tmp_path / "none.extract"
        p = _ok(_run(_opts(tag) + ["--extract", str(x)] + args, env))
        head, got = _decode(x.read_bytes(), fmt)
        assert got == [] and head == _decode(p.stdout, fmt)[0] and any(h.startswith("@SQ") for h in head)
        if fmt == "bam":
            assert x.read_bytes().endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


@pytest.fixture(scope="module")
def synth20k(tmp_path_factory, oracle):
    """20,000 reads of C5 as a BAM of ~90 BGZF members; the oracle's artifact calls of it, counted on the CPU."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("extract20k")
    cfg, g, b = synth.make_config("C5", 20000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    G = oracle.GenomeHolder(g.names, [a.tobytes() for a in g.ascii_contigs()])
    reads, keep = oracle.make_reads({k: v for k, v in b.items() if k != "qname"})
    n_left = n_right = 0
    for i in range(len(names)):
        if b["cigar_off"][i + 1] > b["cigar_off"][i] and any((int(o) & 15) == 4 for o in b["cigar_ops"][b["cigar_off"][i]:b["cigar_off"][i + 1]]):
            rs = oracle.annotate_one(G, reads[i], 5, 100)["rs"]
            n_left += bool(rs & 2)
            n_right += bool(rs & 4)
    return dict(bam=bam, g=g, n_left=n_left, n_right=n_right)


def _stream(s, pieces, **kw):
    """The members of the BAM's records through a BamStream in the given pieces; ([(bytes, n)] per call)."""
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
    ms = _members(raw)
    cum, k = 0, 0
    while cum + struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0] <= at:
        cum += struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0]
        k += 1
    body = ms[k:]
    calls = [body[j:j + pieces] for j in range(0, len(body), pieces)] if pieces else [body]
    ctx = fade_amd.Context(device=0)
    try:
        ctx.genome_upload(s["g"].names, s["g"].ascii_contigs())
        st = ctx.bam_stream(names, floor_len=5, window=100, first_record=at - cum, **kw)
        out, main = [], []
        for j, c in enumerate(calls):
            st.front(b"".join(c), last=(j == len(calls) - 1))
            main.append(st.back())
            out.append(st.back_extract())
        st.close()
    finally:
        ctx.close()
    return out, b"".join(main), len(calls)


def _count(b):
    n = at = 0
    while at < len(b):
        at += 4 + struct.unpack_from("<I", b, at)[0]
        n += 1
    assert at == len(b)
    return n


def test_extract_over_several_calls_one_member_each(synth20k):
    s = synth20k
    assert s["n_left"] > 100 and s["n_right"] > 100, (s["n_left"], s["n_right"])
    per_call, main_many, n_calls = _stream(s, 1, extract=True)
    whole, main_one, _ = _stream(s, 0, extract=True)
    assert n_calls > 50 and len(whole) == 1
    for b, n in per_call:
        assert _count(b) == n                                  # each call's n_records matches its bytes
    assert sum(1 for b, n in per_call if n) > 40
    cat = b"".join(b for b, _ in per_call)
    assert cat == whole[0][0] and len(cat) > 0
    assert sum(n for _, n in per_call) == whole[0][1] == s["n_left"] + s["n_right"]   # the oracle's count
    clipped, _, _ = _stream(s, 0, extract=True, clip=True)
    assert clipped[0] == whole[0]                              # with CLIP, still from the unclipped record
    assert gzip.decompress(main_many) == gzip.decompress(main_one)


def test_extract_goes_by_the_computed_result_not_by_tags_the_record_brought(tmp_path):
    tag = "anno_c5"
    text = _annotated_sam(tag)
    exp = _expected(tag)
    _, in_recs = samutil.parse_sam(text)
    arts = [k for k, r in enumerate(in_recs) if int(r["tags"]["rs"][1]) & 6]
    lines = open(os.path.join(GOLD, tag + ".sam")).read().splitlines()
    body0 = next(i for i, l in enumerate(lines) if not l.startswith("@"))
    lines[body0 + arts[0]] += "\trs:Z:stale"
    lines[body0 + arts[1]] += "\tam:i:5"
    sam, bam = tmp_path / "in.sam", tmp_path / "in.bam"
    sam.write_text("\n".join(lines) + "\n")
    _bam_of(sam, bam)
    fa = os.path.join(GOLD, tag + ".fa")
    for args, env, fmt in ((["-b", str(bam), fa], None, "bam"), (["-b", str(bam), fa], {"FADE_BAM_DEVICE": "0"}, "bam"), ([str(sam), fa], None, "sam")):
        x = tmp_path / "stale.extract"
        p = _ok(_run(_opts(tag) + ["--extract", str(x)] + args, env))
        assert (b"file path on the device" in p.stderr) == (fmt == "bam" and env is None)
        assert _decode(x.read_bytes(), fmt)[1] == exp


def test_back_extract_state_errors(synth20k):
    ctx = fade_amd.Context(device=0)
    try:
        ctx.genome_upload(synth20k["g"].names, synth20k["g"].ascii_contigs())
        for kw in ({}, {"extract": True}):
            st = ctx.bam_stream(synth20k["g"].names, floor_len=5, window=100, **kw)
            with pytest.raises(fade_amd.FadeHipError) as e:   # without the flag; with it, before any back
                st.back_extract()
            assert e.value.code == -6
            st.close()
        st = ctx.bam_stream(synth20k["g"].names, floor_len=5, window=100, extract=True)
        st.front(b"", last=True)
        assert st.back() == b""
        assert st.back_extract() == (b"", 0)
        st.close()
    finally:
        ctx.close()
