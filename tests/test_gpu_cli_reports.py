"""`fade annotate --stats-tsv / --clip-tsv`: the reports equal the restatement of `fade stats` / `fade stats-clip`
(tests/stats_report_ref.py) applied to the records the same run writes, and the records equal a run without the flags."""
import os
import subprocess

import numpy as np
import pytest

import samutil
import stats_report_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")


def _params(tag):
    for line in open(os.path.join(GOLD, tag + ".expected.tsv")):
        if line.startswith("#floor_len"):
            p = dict(kv.split("=") for kv in line[1:].split())
            return ["--min-length", p["floor_len"], "-w", p["window"]]
    return []


def _run(args, timeout=600):
    p = subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def _records(out, bam):
    if bam:
        return samutil.bam_to_sam_records(out)[2]
    return samutil.parse_sam(out.decode())[1]


def _key(r):
    return (r["qname"], r["flag"], r["rname"], r["pos"], r["cigar"], r["seq"], r["qual"], sorted(r["tags"].items()))


def _check(args, sam, fa, tmp_path, bam, sample=None):
    st, cl = tmp_path / "stats.tsv", tmp_path / "clip.tsv"
    base = _run(args + [sam, fa])
    out = _run(args + ["--stats-tsv", str(st), "--clip-tsv", str(cl), sam, fa])
    recs = _records(out, bam)
    assert [_key(r) for r in recs] == [_key(r) for r in _records(base, bam)]
    got_st = st.read_text().split("\n")
    got_cl = cl.read_text().split("\n")
    assert got_st[0] == R.STATS_HEADER and got_st[-1] == "" and got_cl[0] == R.CLIP_HEADER and got_cl[-1] == ""
    exp_cl = R.clip_rows(recs)
    assert got_cl[1:-1] == exp_cl
    exp_st = R.stats_rows(recs, sample)
    rows = [l.split("\t") for l in got_st[1:-1]]
    assert len(rows) == len(exp_st)
    for k, (g, e) in enumerate(zip(rows, exp_st)):
        assert len(g) == 21
        if e[12] is None:  # SW columns outside the sample
            g = [x if i not in (12, 13, 17) else None for i, x in enumerate(g)]
        assert g == e, (k, g, e)
    return len(rows), len(exp_cl)


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("tag", ["anno_c1", "anno_c2", "anno_c5"])
def test_reports_on_golden(tag, bam, tmp_path):
    args = ["annotate"] + _params(tag) + (["-b"] if bam else [])
    n_st, n_cl = _check(args, os.path.join(GOLD, tag + ".sam"), os.path.join(GOLD, tag + ".fa"), tmp_path, bam)
    assert n_st > 0 and n_cl > 0


def test_reports_on_100k_reads(tmp_path):
    from fade_amd import synth
    cfg = synth.config("C2")
    cfg.update(contig_len=2_000_000)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
    b = synth.make_reads(g, 100_000, 5, **cfg)
    sam, fa = tmp_path / "in.sam", tmp_path / "ref.fa"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths]))
    fa.write_bytes(g.fasta_bytes())
    rng = np.random.default_rng(5)
    sample = set(int(x) for x in rng.choice(200_000, 3000, replace=False))  # SW columns on a seeded sample of rows
    n_st, n_cl = _check(["annotate", "-b", "--batch", "20000"], str(sam), str(fa), tmp_path, True, sample)
    assert n_st > 1000 and n_cl > 5000
