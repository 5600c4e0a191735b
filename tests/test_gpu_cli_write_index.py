"""`fade annotate --write-index` and `fade out --write-index` on coordinate-sorted BAM files: the index the binary writes
parses, is tests/bai_model.py's over the file that went to stdout (whose records' virtual offsets tests/bai_reader.py derives
from the file's own members), and finds through the real bytes what brute force finds; the BAM on stdout is what the run
without the option writes — its records byte for byte, its header but for the option in the @PG line's command."""
import gzip
import os

import pytest

import bai_model as bm
import bai_reader as br
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import GOLD, _bam_of, _ok, _run, _split
from test_gpu_cli_keep_sorted import _sorted_sam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """anno_c2, coordinate-sorted: the input of annotate, and the annotated set for `out`."""
    d = tmp_path_factory.mktemp("indexgold")
    raw, anno = d / "in.sam", d / "anno.sam"
    raw.write_text(_sorted_sam(open(os.path.join(GOLD, "anno_c2.sam")).read()))
    anno.write_text(_sorted_sam(_annotated_sam("anno_c2")))
    _bam_of(raw, d / "in.bam")
    _bam_of(anno, d / "anno.bam")
    return dict(dir=d, bam=d / "in.bam", anno=d / "anno.bam", fa=os.path.join(GOLD, "anno_c2.fa"))


def _pg_less_option(out, path):
    raw = gzip.decompress(out)
    l_text = int.from_bytes(raw[4:8], "little")
    return [l.replace(" --write-index " + path, "") for l in raw[8:8 + l_text].decode().splitlines() if l.startswith("@PG")]


def _both(gold, name, args, tail, env=None):
    """The command without the option and with it: (plain's stdout, the indexed run's stdout, the .bai's bytes)."""
    path = str(gold["dir"] / (name + ".bai"))
    plain = _ok(_run(args + tail, env))
    with_ix = _ok(_run(args + ["--write-index", path] + tail, env))
    assert _split(with_ix.stdout) == _split(plain.stdout)
    assert _pg_less_option(with_ix.stdout, path) == _pg_less_option(plain.stdout, path)
    assert with_ix.stderr == plain.stderr           # every message is what it was
    return plain.stdout, with_ix.stdout, open(path, "rb").read()


def _check(data, bai, min_records):
    n_ref, recs = br.bam_records(data)
    assert len(recs) >= min_records
    parsed = bm.read_bai(bai)                       # it parses, every byte used
    assert len(parsed["refs"]) == n_ref
    assert bai == bm.build(n_ref, recs)             # it is the model's over the written file
    br.check_queries(data, bai, recs, n_ref)        # and it finds what is there
    return recs


def test_annotate(gold):
    _, out, bai = _both(gold, "annotate", ["annotate", "-b"], [str(gold["bam"]), gold["fa"]])
    _check(out, bai, 100)


def test_annotate_uncompressed_in_small_calls(gold):
    _, out, bai = _both(gold, "annotate_u", ["annotate", "-u"], [str(gold["bam"]), gold["fa"]], {"FADE_BAM_CHUNK_MB": "1"})
    _check(out, bai, 100)


def test_annotate_clip_keep_sorted(gold):
    _, out, bai = _both(gold, "annotate_c", ["annotate", "-c", "--keep-sorted", "-b"], [str(gold["bam"]), gold["fa"]])
    _check(out, bai, 100)


def test_out_clip_keep_sorted(gold):
    _, out, bai = _both(gold, "out_c", ["out", "-c", "--keep-sorted", "-b"], [str(gold["anno"])])
    _check(out, bai, 100)


def test_out_ejects_and_indexes_what_is_left(gold):
    plain, out, bai = _both(gold, "out", ["out", "--gpus", "1", "-b"], [str(gold["anno"])])
    recs = _check(out, bai, 10)
    assert len(recs) < len(br.bam_records(gold["anno"].read_bytes())[1])


def test_a_pipe_as_stdout_works(gold):
    """(subprocess.PIPE is one: the driver counts the header's bytes itself and never asks stdout where it is)"""
    path = str(gold["dir"] / "pipe.bai")
    p = _ok(_run(["annotate", "-b", "--write-index=" + path, str(gold["bam"]), gold["fa"]]))
    _check(p.stdout, open(path, "rb").read(), 100)
