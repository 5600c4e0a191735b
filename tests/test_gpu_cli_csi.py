"""`--write-index PATH --csi` through the driver: `fade out --sort` on reads of a 2 Gbp contig, some of them beyond 2^29 — where
the same run without --csi ends with the BAI's message —, a small genome (depth 5, the chunks a .bai holds), `fade extract
--sorted` and `fade annotate --extract-sorted`.  The index file is BGZF with the end-of-file marker; its payload parses with
tests/csi_model.py's reader, is the model's over the records of the file that was written (tests/bai_reader.py derives their
virtual offsets from the file's own members), and finds through the real bytes what brute force finds."""
import os
import random
import re
import struct

import pytest

import bai_model as bm
import bai_reader as br
import csi_model as cm
import test_gpu_bam_index as bi
from test_gpu_annotate_clip import _ok, _run
from test_gpu_bgzf import EOF_MARK
from test_gpu_cli_write_index import gold  # noqa: F401  (the fixture: anno_c2 coordinate-sorted, raw and annotated, as BAM)
from test_gpu_csi_stream import _check_queries
from test_gpu_out_fragments import _bgzf

pytestmark = pytest.mark.gpu

CONTIGS = [("giant", 2_000_000_000), ("small", 100_000)]
SAID = re.compile(rb"\[I::([a-z -]+)\] --csi: (\S+) is a CSI index of min_shift 14 and depth (\d) \(coordinates up to 2\^(\d+)\)")


def _bam_bytes(records):
    text = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(CONTIGS))
    for n, ln in CONTIGS:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return _bgzf(head + b"".join(records))


@pytest.fixture(scope="module")
def giant(tmp_path_factory):
    """A few hundred tagged reads in no order: most of them spread over the 2 Gbp contig, the large positions of the issue,
    some on the small contig, an unmapped tail; a tenth are artifact reads that plain `fade out` drops."""
    rng = random.Random(23)
    specs = [(0, (1 << 29) - 10, "20M30S"), (0, 1 << 29, "50M"), (0, (1 << 30) + 77, "50M"), (0, (1 << 30) + 77, "25M200000000N25M"),
             (0, 1_999_999_900, "50M"), (0, 0, "50M")]
    for _ in range(300):
        specs.append((0, rng.choice([rng.randrange(1_999_000_000), (1 << 29) + rng.randrange(-40_000, 40_000), rng.randrange(100_000)]),
                      rng.choice(["50M", "50M", "25M3000N25M", "10S40M", "25M1D25M"])))
    for _ in range(60):
        specs.append((1, rng.randrange(99_000), "50M"))
    specs += [(-1, -1, "*")] * 9
    rng.shuffle(specs)
    records = [bi._rec(k, tid, pos, cigar=cigar, flag=4 if tid < 0 or k % 37 == 5 else 0, rs=2 if k % 10 == 3 and tid >= 0 else 0)
               for k, (tid, pos, cigar) in enumerate(specs)]
    d = tmp_path_factory.mktemp("cli_csi")
    bam = d / "giant.bam"
    bam.write_bytes(_bam_bytes(records))
    return dict(dir=d, bam=bam, n=len(records), kept=sum(1 for k, s in enumerate(specs) if not (k % 10 == 3 and s[0] >= 0)))


def _check(data, index_bytes, depth, min_records):
    """The written index against the written file; returns (records, the parsed index)."""
    n_ref, recs = br.bam_records(data)
    assert len(recs) >= min_records
    assert index_bytes.endswith(EOF_MARK)                                 # BGZF, with the marker
    mem = br.walk_members(index_bytes)
    assert mem[-1][1] == b"" and all(0 < len(p) <= 0xff00 for _, p in mem[:-1])
    payload = b"".join(p for _, p in mem)
    assert payload == cm.payload_of(index_bytes)
    csi = cm.read_csi(payload)                                            # it parses, every byte used
    assert (csi["min_shift"], csi["depth"], csi["aux"]) == (14, depth, b"") and len(csi["refs"]) == n_ref
    assert payload == cm.build(n_ref, recs, 14, depth)                    # it is the model's over the written file
    _check_queries(data, csi, recs, n_ref)                                # and it finds what is there
    return recs, csi


def _said(p, who, path, depth):
    m = SAID.findall(p.stderr)
    assert m == [(who, path.encode(), b"%d" % depth, b"%d" % (14 + 3 * depth))], p.stderr.decode()


def test_out_sort_on_a_2_gbp_contig(giant):
    path = str(giant["dir"] / "sorted.csi")
    p = _ok(_run(["out", "--gpus", "1", "--sort", "--write-index", path, "--csi", "-b", str(giant["bam"])]))
    recs, csi = _check(p.stdout, open(path, "rb").read(), 6, 300)
    _said(p, b"fade-out", path, 6)
    assert len(recs) == giant["kept"] < giant["n"]
    keys = [bm.key_of(r) for r in recs]
    assert keys == sorted(keys) and sum(1 for r in recs if r["tid"] == 0 and r["pos"] >= 1 << 29) > 100
    assert csi["n_no_coor"] == 9 and csi["refs"][1]["meta"] is not None
    bins = csi["refs"][0]["bins"]
    assert cm.first_bin(6) + (1 << 15) in bins and max(bins) < 299594 and 0 in bins   # (the record across 2^29 lies in the root)
    # the same run without --csi: today's refusal, with today's message, and no index
    bai = str(giant["dir"] / "sorted.bai")
    q = _run(["out", "--gpus", "1", "--sort", "--write-index", bai, "-b", str(giant["bam"])])
    assert q.returncode == 1 and b"ends beyond 2^29 on its reference (a BAI index cannot hold it)" in q.stderr, q.stderr.decode()
    assert not os.path.exists(bai) and b"--csi" not in q.stderr
    # without an index at all the sorted records are the same
    plain = _ok(_run(["out", "--gpus", "1", "--sort", "-b", str(giant["bam"])]))
    assert [(r["tid"], r["pos"], r["size"]) for r in br.bam_records(plain.stdout)[1]] == [(r["tid"], r["pos"], r["size"]) for r in recs]


def test_out_sort_uncompressed_in_a_store_that_grows(giant):
    path = str(giant["dir"] / "stored.csi")
    p = _ok(_run(["out", "--gpus", "1", "--sort", "--write-index=" + path, "--csi", "-u", str(giant["bam"])], {"FADEHIP_RECSTORE_BYTES": "4096"}))
    recs, _ = _check(p.stdout, open(path, "rb").read(), 6, 300)
    assert len(recs) == giant["kept"]
    _said(p, b"fade-out", path, 6)


def test_a_small_genome_gives_depth_5_and_the_chunks_of_the_bai(gold):  # noqa: F811
    d = gold["dir"]
    csi_path, bai_path = str(d / "small.csi"), str(d / "small.bai")
    args = ["out", "-c", "--keep-sorted", "-b"]
    p = _ok(_run(args + ["--write-index", csi_path, "--csi", str(gold["anno"])]))
    q = _ok(_run(args + ["--write-index", bai_path, str(gold["anno"])]))
    recs, csi = _check(p.stdout, open(csi_path, "rb").read(), 5, 100)
    _said(p, b"fade-out", csi_path, 5)
    assert b"--csi" not in q.stderr and [ln for ln in p.stderr.splitlines() if b"--csi" not in ln] == q.stderr.splitlines()
    n_ref, plain = br.bam_records(q.stdout)
    assert [(r["tid"], r["pos"], r["size"]) for r in plain] == [(r["tid"], r["pos"], r["size"]) for r in recs]
    bai = bm.read_bai(open(bai_path, "rb").read())
    # (the two files' @PG lines differ in the option, so a header member may differ in size: chunks are compared as counts)
    assert [{b: len(ch) for b, ch in ref["bins"].items()} for ref in bai["refs"]] == [{b: len(ch[1]) for b, ch in ref["bins"].items()} for ref in csi["refs"]]
    assert bai["n_no_coor"] == csi["n_no_coor"]


def test_extract_sorted(gold):  # noqa: F811
    path = str(gold["dir"] / "extract.csi")
    p = _ok(_run(["extract", "--gpus", "1", "--sorted", "--write-index", path, "--csi", "-b", str(gold["anno"])]))
    recs, _ = _check(p.stdout, open(path, "rb").read(), 5, 6)
    _said(p, b"fade extract", path, 5)
    plain = _ok(_run(["extract", "--gpus", "1", "--sorted", "-b", str(gold["anno"])]))
    assert [(r["tid"], r["pos"], r["size"]) for r in br.bam_records(plain.stdout)[1]] == [(r["tid"], r["pos"], r["size"]) for r in recs]


def test_annotate_extract_sorted_writes_path_csi(gold):  # noqa: F811
    x = str(gold["dir"] / "sorted.extract.bam")
    p = _ok(_run(["annotate", "-b", "--extract", x, "--extract-sorted", "--csi", str(gold["bam"]), gold["fa"]]))
    assert os.path.exists(x + ".csi") and not os.path.exists(x + ".bai")
    _check(open(x, "rb").read(), open(x + ".csi", "rb").read(), 5, 6)
    _said(p, b"fade-annotate", x + ".csi", 5)
