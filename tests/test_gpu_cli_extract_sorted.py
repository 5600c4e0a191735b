"""`fade extract --gpus 1 --sorted [--write-index PATH]` and `fade annotate --extract PATH --extract-sorted` on the golden BAMs
and on 30,000 synthetic reads in many calls: the records are tests/recstore_model.py's order of what the plain
`fade extract --gpus 1` (or `fade annotate --extract PATH`) writes, byte for byte; the header says SO:coordinate and keeps its
@PG lines; the end-of-file marker is there; the index is tests/bai_model.py's over the written file and finds through the
real bytes what brute force finds; stdout may be a pipe; an input without artifacts gives a header, the marker and a valid
empty index; and annotate's main output does not know about the option."""
import gzip
import os
import subprocess

import pytest

import bai_model as bm
import bai_reader as br
import recstore_model as rm
import samutil
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import FADE, GOLD, _bam_of, _ok, _run, _split
from test_gpu_bgzf import EOF_MARK

pytestmark = pytest.mark.gpu

WARN = b"[W::fade extract] Output SAM/BAM will not be sorted"
SMALL = {"FADE_BAM_CHUNK_MB": "1", "FADEHIP_RECSTORE_BYTES": "4096"}   # many calls, an arena that grows many times
TAGS = ["anno_c1", "anno_c2", "anno_c5"]


def _header_text(data):
    raw = gzip.decompress(data)
    return raw[8:8 + int.from_bytes(raw[4:8], "little")].decode()


def _records(data):
    """The records' bytes of a BAM file's bytes, one behind the other."""
    body = _split(data)[1]
    at = 4
    for _ in range(int.from_bytes(body[:4], "little")):
        at += 8 + int.from_bytes(body[at:at + 4], "little")
    return rm.split(body[at:])


def _check_sorted(data, bai, plain, *options):
    """`data` (the sorted file) against `plain` (the unsorted one of the same input): records, header, marker, index.
    options: what the two runs' command lines differ in (the @PG line's command names it)."""
    assert _records(data) == rm.order(_records(plain))
    assert data.endswith(EOF_MARK)
    want = rm.header_sorted(_header_text(plain))
    def strip(text):
        for o in options:
            text = text.replace(o, "")
        return text.splitlines()
    assert strip(_header_text(data)) == strip(want)
    hd = _header_text(data).splitlines()[0].split("\t")
    assert hd[0] == "@HD" and hd.count("SO:coordinate") == 1 and sum(f.startswith("SO:") for f in hd) == 1
    n_ref, recs = br.bam_records(data)
    parsed = bm.read_bai(bai)
    assert len(parsed["refs"]) == n_ref and bai == bm.build(n_ref, recs)
    br.check_queries(data, bai, recs, n_ref)
    return recs


@pytest.fixture(scope="module", params=TAGS)
def gold(request, tmp_path_factory):
    tag = request.param
    d = tmp_path_factory.mktemp("xsorted_" + tag)
    raw, anno = os.path.join(GOLD, tag + ".sam"), d / "anno.sam"
    anno.write_text(_annotated_sam(tag))
    _bam_of(raw, d / "in.bam")
    _bam_of(anno, d / "anno.bam")
    from test_gpu_cli import _expected
    _, floor_len, window = _expected(tag)
    return dict(dir=d, bam=d / "in.bam", anno=d / "anno.bam", fa=os.path.join(GOLD, tag + ".fa"), opts=["--min-length", str(floor_len), "-w", str(window)])


@pytest.mark.parametrize("fmt", ["-b", "-u"])
def test_extract_sorted_on_the_golden_sets(gold, fmt):
    d = gold["dir"]
    plain = _ok(_run(["extract", "--gpus", "1", fmt, str(gold["anno"])]))
    assert plain.stderr.count(WARN) == 1 and len(_records(plain.stdout)) >= 6
    path = str(d / ("x%s.bai" % fmt))
    p = _ok(_run(["extract", "--gpus", "1", "--sorted", "--write-index", path, fmt, str(gold["anno"])], SMALL))      # (stdout is a pipe)
    assert WARN not in p.stderr and b"[W::" not in p.stderr
    recs = _check_sorted(p.stdout, open(path, "rb").read(), plain.stdout, " --sorted --write-index " + path)
    assert [l for l in _header_text(p.stdout).splitlines() if l.startswith("@PG")][-1].startswith("@PG\tID:fade-extract")
    assert len(recs) == len(_records(plain.stdout))
    if fmt == "-u" or not str(gold["anno"]).count("anno_c5"):
        return
    # without --write-index: the same file, no index; into a file instead of a pipe: the same bytes
    q = _ok(_run(["extract", "--gpus", "1", "--sorted", fmt, str(gold["anno"])]))
    assert _records(q.stdout) == _records(p.stdout) and q.stdout.endswith(EOF_MARK)
    with open(d / "to_file.bam", "wb") as fo:
        r = subprocess.run([FADE, "extract", "--gpus", "1", "--sorted", "--write-index", path + "2", fmt, str(gold["anno"])],
                           stdout=fo, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, **SMALL))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    # (its @PG line names another PATH, so its header's members and with them every offset differ: the index is held to its own file)
    assert len(_check_sorted((d / "to_file.bam").read_bytes(), open(path + "2", "rb").read(), plain.stdout, " --sorted --write-index " + path + "2")) == len(recs)


def test_annotate_extract_sorted_on_the_golden_sets(gold):
    d = gold["dir"]
    base = ["annotate", "--timing"] + gold["opts"] + ["-b"]    # (--timing: the run says which path it took)
    x0, x1 = str(d / "plain.extract.bam"), str(d / "sorted.extract.bam")
    plain = _ok(_run(base + ["--extract", x0, str(gold["bam"]), gold["fa"]]))
    p = _ok(_run(base + ["--extract", x1, "--extract-sorted", str(gold["bam"]), gold["fa"]], SMALL))
    assert b"file path on the device" in p.stderr and WARN not in p.stderr and plain.stderr.count(WARN) == 1
    assert _split(p.stdout) == _split(plain.stdout) and p.stdout.endswith(EOF_MARK)     # the main output does not know about the option
    _check_sorted(open(x1, "rb").read(), open(x1 + ".bai", "rb").read(), open(x0, "rb").read(), " --extract-sorted", x0, x1)


def test_an_input_without_artifacts_gives_a_header_the_marker_and_a_valid_empty_index(tmp_path):
    tag = "anno_c1"
    lines = _annotated_sam(tag).splitlines()
    keep = [l for l in lines if l.startswith("@") or not int(dict((f.split(":", 2)[0], f.split(":", 2)[2]) for f in l.split("\t")[11:]).get("rs", "0")) & 6]
    assert sum(1 for l in keep if not l.startswith("@")) >= 100
    sam, bam = tmp_path / "clean.sam", tmp_path / "clean.bam"
    sam.write_text("\n".join(keep) + "\n")
    _bam_of(sam, bam)
    path = str(tmp_path / "empty.bai")
    p = _ok(_run(["extract", "--gpus", "1", "--sorted", "--write-index", path, "-b", str(bam)]))
    n_ref, recs = br.bam_records(p.stdout)
    assert recs == [] and n_ref >= 1 and p.stdout.endswith(EOF_MARK) and _header_text(p.stdout).startswith("@HD\t")
    assert "SO:coordinate" in _header_text(p.stdout).splitlines()[0]
    assert open(path, "rb").read() == bm.build(n_ref, [])


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """30,000 reads of C5 (tests/test_gpu_annotate_clip.py's) as a BAM, and the annotated BAM `fade annotate -b` makes of it."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("xsortedbig")
    cfg, g, b = synth.make_config("C5", 30000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, fa, bam, anno = d / "in.sam", d / "ref.fa", d / "in.bam", d / "anno.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    fa.write_bytes(g.fasta_bytes())
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    anno.write_bytes(_ok(_run(["annotate", "-w", "100", "-b", str(bam), str(fa)])).stdout)
    return dict(dir=d, bam=bam, fa=fa, anno=anno)


def test_both_command_lines_on_30000_reads_in_many_calls(big):
    d = big["dir"]
    plain = _ok(_run(["extract", "--gpus", "1", "-b", str(big["anno"])]))
    n = len(_records(plain.stdout))
    assert n > 1000
    path = str(d / "big.bai")
    p = _ok(_run(["extract", "--gpus", "1", "--sorted", "--write-index", path, "--timing", "-b", str(big["anno"])], SMALL))
    assert b"--sorted: %d records sorted on the device" % n in p.stderr
    recs = _check_sorted(p.stdout, open(path, "rb").read(), plain.stdout, " --sorted --write-index " + path + " --timing")
    assert len(recs) == n
    x0, x1 = str(d / "plain.extract.bam"), str(d / "sorted.extract.bam")
    base = ["annotate", "-w", "100", "-u"]
    a0 = _ok(_run(base + ["--extract", x0, str(big["bam"]), str(big["fa"])], SMALL))
    a1 = _ok(_run(base + ["--extract", x1, "--extract-sorted", str(big["bam"]), str(big["fa"])], SMALL))
    assert _split(a1.stdout) == _split(a0.stdout)
    _check_sorted(open(x1, "rb").read(), open(x1 + ".bai", "rb").read(), open(x0, "rb").read(), " --extract-sorted", x0, x1)
    assert _records(open(x1, "rb").read()) == _records(p.stdout)           # the one-step form and the two-step form agree
