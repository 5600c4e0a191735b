"""What `--repeats` costs: wall time of `fade stats --gpus 1` with and without the option, the same binary, the two forms
interleaved, on a synthetic BAM that the same build annotated first; and the seconds the driver reports for loading and sealing
a seeded synthetic BED of 5 M intervals (its `[timing] --repeats:` line).  A record only: no threshold hangs on it.

python tools/repeats_cost.py [--config C2] [--reads 1000000] [--intervals 5000000] [--runs 4] [--json OUT]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synthgen as sg  # noqa: E402
from fade_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C2")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--intervals", type=int, default=5_000_000)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno, bed = (os.path.join(tmp, "rpq_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam", "bed"))
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
w.write(sg.make_reads(g, a.reads, 100, cfg), 0)
w.close()
FADE = os.path.join(ROOT, "fade_amd", "fade")


def timed(argv, out=None):
    t0 = time.perf_counter()
    with open(out or os.devnull, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr.decode(errors="replace")


timed([FADE, "annotate", "-b", "-t", "16", "-w", str(cfg["window"]), bam, fa], anno)
print("input: %s, %d reads annotated by this build, %d bytes" % (anno, a.reads, os.path.getsize(anno)), flush=True)

# the BED: seeded, in no order, RepeatMasker-like lengths, over the genome's contigs
rng = np.random.default_rng(20261021)
n_contigs, contig_len = len(g.names), int(g.lengths[0])
with open(bed, "wb") as fo:
    for at in range(0, a.intervals, 500_000):
        m = min(500_000, a.intervals - at)
        c = rng.integers(0, n_contigs, m)
        s = rng.integers(0, contig_len - 1, m)
        e = np.minimum(s + rng.integers(1, 600, m), contig_len)
        fo.write("".join("chr%d\t%d\t%d\n" % t for t in zip((c + 1).tolist(), s.tolist(), e.tolist())).encode())
print("bed: %s, %d intervals, %d bytes" % (bed, a.intervals, os.path.getsize(bed)), flush=True)

o1, o2 = os.path.join(tmp, "rpq.plain.tsv"), os.path.join(tmp, "rpq.repeats.tsv")
plain, repeats, load_s, rows = [], [], [], 0
for rep in range(a.runs):
    t_p, _ = timed([FADE, "stats", "--gpus", "1", "--timing", "-t", "16", anno, o1])
    t_r, err = timed([FADE, "stats", "--gpus", "1", "--timing", "-t", "16", "--repeats", bed, anno, o2])
    m = re.search(r"\[timing\] --repeats: (\d+) intervals of (\d+) contigs loaded and sealed on the device in ([0-9.]+) s", err)
    if not m or int(m.group(1)) != a.intervals:
        sys.exit("no [timing] --repeats line for %d intervals in: %s" % (a.intervals, err[-1500:]))
    plain.append(t_p)
    repeats.append(t_r)
    load_s.append(float(m.group(3)))
    with open(o1, "rb") as f1, open(o2, "rb") as f2:
        l1, l2 = f1.read().split(b"\n"), f2.read().split(b"\n")
    rows = len(l1) - 2
    if len(l1) != len(l2) or any(y.rsplit(b"\t", 2)[0] != x for x, y in zip(l1[:-1], l2[:-1])):
        sys.exit("the rows with --repeats are not the plain rows with two more columns")
    print("run %d: plain %.3f s, --repeats %.3f s (load + seal %.3f s); %d rows" % (rep, t_p, t_r, load_s[-1], rows), flush=True)
hits = [sum(1 for y in l2[1:-1] if y.split(b"\t")[21 + k] == b"1") for k in (0, 1)]
res = dict(config=a.config, reads=a.reads, rows=rows, intervals=a.intervals, bed_bytes=os.path.getsize(bed), runs=a.runs, plain_s=plain, repeats_s=repeats,
           load_and_seal_s=load_s, plain_median_s=statistics.median(plain), repeats_median_s=statistics.median(repeats),
           load_and_seal_median_s=statistics.median(load_s), plain_spread_s=[min(plain), max(plain)], repeats_spread_s=[min(repeats), max(repeats)],
           repeats_minus_load_median_s=statistics.median([r - l for r, l in zip(repeats, load_s)]), rows_read_rpm_1=hits[0], rows_art_rpm_1=hits[1])
for p in (o1, o2, bam, fa, anno, bed):
    if os.path.exists(p):
        os.remove(p)
print(json.dumps(res))
if a.json:  # one file for every configuration measured: {config: result}
    every = json.load(open(a.json)) if os.path.exists(a.json) else {}
    every[a.config] = res
    with open(a.json, "w") as fo:
        json.dump(every, fo, indent=1)
