"""`fade annotate -c --keep-sorted` and `fade out -c --keep-sorted` on coordinate-sorted BAM files: the records of the same
command without the option, byte for byte, in stable order by key (tests/resort_model.py) — on a golden set and on 30,000
reads with FADE_BAM_CHUNK_MB at its smallest, so that the held tail crosses several calls; unsorted input is refused with
the record's index."""
import os
import struct

import pytest

import resort_model as rm
import samutil
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import GOLD, W1, W2, _bam_of, _ok, _run, _split
from test_gpu_bam_from_tags import _records, _records_of_bam_body

pytestmark = pytest.mark.gpu

W_KEEP = b"[W::fade-out] --keep-sorted: clipped records are written at their new coordinates"
SMALL = {"FADE_BAM_CHUNK_MB": "1"}


def _sorted_sam(text):
    """The SAM text with its records in coordinate order (stable; unmapped records last), as `samtools sort` leaves them."""
    lines = text.splitlines()
    head = [l for l in lines if l.startswith("@")]
    tid = {l.split("\t")[1][3:]: k for k, l in enumerate(l for l in head if l.startswith("@SQ"))}
    recs = [l for l in lines if l and not l.startswith("@")]
    key = lambda l: (tid.get(l.split("\t")[2], 1 << 32), int(l.split("\t")[3]))
    return "\n".join(head + sorted(recs, key=key)) + "\n"


def _recs(out):
    """The records of a BAM the binary wrote, as bytes."""
    return _records(_records_of_bam_body(_split(out)[1]))


def _check(inp, plain, kept, moved_min):
    """kept = plain's records (inp's, clipped, in input order) in stable key order; its keys do not decrease."""
    a, b, c = _recs(inp), _recs(plain), _recs(kept)
    assert len(a) == len(b) == len(c)
    assert [rm.key_in(r) for r in a] == sorted(rm.key_in(r) for r in a), "the test's input is coordinate-sorted"
    keys = [rm.key_out(x, y) for x, y in zip(a, b)]
    order = rm.stable_order(keys)
    assert sum(1 for k, i in enumerate(order) if k != i) >= moved_min, "the clip moves records of this input"
    assert c == [b[i] for i in order]
    assert [keys[i] for i in order] == sorted(keys)
    assert _split(plain)[0] == _split(kept)[0]  # the header (less @PG) is the same


def _said(p, keep):
    assert p.stderr.count(W2) == 1
    assert (p.stderr.count(W_KEEP), p.stderr.count(W1)) == ((1, 0) if keep else (0, 1)), p.stderr.decode()[-1500:]
    assert b"file path on the device" in p.stderr


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """anno_c2, coordinate-sorted: the input of annotate, and the annotated set for `out`."""
    d = tmp_path_factory.mktemp("keepgold")
    raw, anno = d / "in.sam", d / "anno.sam"
    raw.write_text(_sorted_sam(open(os.path.join(GOLD, "anno_c2.sam")).read()))
    anno.write_text(_sorted_sam(_annotated_sam("anno_c2")))
    _bam_of(raw, d / "in.bam")
    _bam_of(anno, d / "anno.bam")
    return dict(bam=d / "in.bam", anno=d / "anno.bam", fa=os.path.join(GOLD, "anno_c2.fa"))


def test_golden_set_annotate_and_out(gold):
    base = ["annotate", "--timing", "-c", "-b"]
    plain = _ok(_run(base + [str(gold["bam"]), gold["fa"]]))
    kept = _ok(_run(base + ["--keep-sorted", str(gold["bam"]), gold["fa"]]))
    _said(plain, False)
    _said(kept, True)
    _check(gold["bam"].read_bytes(), plain.stdout, kept.stdout, 1)
    plain = _ok(_run(["out", "--timing", "-c", "--gpus", "1", "-b", str(gold["anno"])]))
    _said(plain, False)
    for fmt in ("-b", "-u"):
        kept = _ok(_run(["out", "--timing", "-c", "--keep-sorted=true", fmt, str(gold["anno"])]))
        _said(kept, True)
        _check(gold["anno"].read_bytes(), plain.stdout, kept.stdout, 1)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """30,000 reads of C5 (30 % soft-clipped), coordinate-sorted, as a BAM of ~130 BGZF members; the same annotated; and the
    unsorted BAM the reads were made as."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("keepbig")
    cfg, g, b = synth.make_config("C5", 30000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    text = samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names)
    (d / "unsorted.sam").write_text(text)
    (d / "in.sam").write_text(_sorted_sam(text))
    (d / "ref.fa").write_bytes(g.fasta_bytes())
    for n in ("unsorted", "in"):
        _bam_of(d / (n + ".sam"), d / (n + ".bam"))
    (d / "anno.bam").write_bytes(_ok(_run(["annotate", "-w", "100", "-b", str(d / "in.bam"), str(d / "ref.fa")])).stdout)
    return d


def test_30000_reads_annotate_in_many_calls(big):
    base = ["annotate", "--timing", "-w", "100", "-c", "-b"]
    plain = _ok(_run(base + [str(big / "in.bam"), str(big / "ref.fa")], SMALL))
    kept = _ok(_run(base + ["--keep-sorted", str(big / "in.bam"), str(big / "ref.fa")], SMALL))
    _said(kept, True)
    _check((big / "in.bam").read_bytes(), plain.stdout, kept.stdout, 300)


@pytest.mark.parametrize("fmt", ["-b", "-u"])
def test_30000_annotated_reads_out_in_many_calls(big, fmt):
    plain = _ok(_run(["out", "--timing", "-c", "--gpus", "1", "-b", str(big / "anno.bam")], SMALL))
    kept = _ok(_run(["out", "--timing", "-c", "--keep-sorted", fmt, str(big / "anno.bam")], SMALL))
    _said(kept, True)
    _check((big / "anno.bam").read_bytes(), plain.stdout, kept.stdout, 300)


def test_unsorted_input_exits_with_the_record(big):
    recs = _recs((big / "unsorted.bam").read_bytes())
    first_bad = next(i for i in range(1, len(recs)) if rm.key_in(recs[i]) < rm.key_in(recs[i - 1]))
    for args in (["out", "-c", "--keep-sorted", "-b", str(big / "unsorted.bam")],
                 ["annotate", "-w", "100", "-c", "--keep-sorted", "-b", str(big / "unsorted.bam"), str(big / "ref.fa")]):
        p = _run(args, SMALL)
        assert p.returncode == 1, p.stderr.decode()[-1500:]
        assert b"record %d: not in coordinate order (--keep-sorted needs coordinate-sorted input)" % first_bad in p.stderr, p.stderr.decode()[-1500:]
