"""What `--keep-sorted` costs: wall time of `fade annotate -c -b` with and without the option, the same binary, the two forms
interleaved, on a synthetic BAM whose records this tool sorts by coordinate itself (the generator deals reads in random
order).  With --timing the binary also says how many records the largest held tail had; the tool records it.

python tools/keep_sorted_cost.py [--config C2] [--reads 4000000] [--runs 4] [--json OUT]"""
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
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--json", default="")
a = ap.parse_args()


def sorted_batch(b):
    """The batch in stable coordinate order: by (refID as uint32, pos + 1 as uint32), the key of the option."""
    n = len(b["pos"])
    order = np.lexsort(((b["pos"].astype(np.int64) + 1) & 0xffffffff, b["tid"].astype(np.int64) & 0xffffffff))
    out = {k: b[k][order] for k in ("tid", "pos", "flag", "has_sa", "l_seq")}

    def gather(off, data):
        lens = np.diff(off.astype(np.int64))[order]
        new_off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=new_off[1:])
        idx = np.repeat(off[:-1].astype(np.int64)[order] - new_off[:-1], lens) + np.arange(new_off[-1])
        return new_off, data[idx]

    co, out["cigar_ops"] = gather(b["cigar_off"], b["cigar_ops"])
    out["cigar_off"] = co.astype(np.uint32)
    so, out["seq_packed"] = gather(b["seq_off"], b["seq_packed"])
    out["seq_off"] = so.astype(np.uint32)
    qo, out["qual"] = gather(b["qual_off"], b["qual"])
    out["qual_off"] = qo
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa = os.path.join(tmp, "keepq_%s.bam" % a.config), os.path.join(tmp, "keepq_%s.fa" % a.config)
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
w.write(sorted_batch(sg.make_reads(g, a.reads, 100, cfg)), 0)
w.close()
print("input: %s, %d reads sorted by coordinate, %d bytes" % (bam, a.reads, os.path.getsize(bam)), flush=True)
FADE = os.path.join(ROOT, "fade_amd", "fade")
common = ["--timing", "-t", "16", "-w", str(cfg["window"])]


def timed(argv, out):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr.decode(errors="replace")


plain, kept, held, sizes = [], [], (0, 0), {}
o1, o2 = os.path.join(tmp, "keepq.plain.bam"), os.path.join(tmp, "keepq.kept.bam")
for rep in range(a.runs):
    t_p, _ = timed([FADE, "annotate", "-c", "-b"] + common + [bam, fa], o1)
    t_k, err = timed([FADE, "annotate", "-c", "--keep-sorted", "-b"] + common + [bam, fa], o2)
    m = re.search(r"--keep-sorted: at most (\d+) records \((\d+) bytes\) held", err)
    held = (int(m.group(1)), int(m.group(2))) if m else held
    plain.append(t_p)
    kept.append(t_k)
    sizes = dict(plain_bytes=os.path.getsize(o1), keep_sorted_bytes=os.path.getsize(o2))
    print("run %d: -c %.3f s, -c --keep-sorted %.3f s; largest held tail %d records (%d bytes)" % (rep, t_p, t_k, held[0], held[1]), flush=True)
for p in (o1, o2):
    if os.path.exists(p):
        os.remove(p)
res = dict(config=a.config, reads=a.reads, runs=a.runs, clip_s=plain, clip_keep_sorted_s=kept,
           clip_median_s=statistics.median(plain), clip_keep_sorted_median_s=statistics.median(kept),
           clip_spread_s=[min(plain), max(plain)], clip_keep_sorted_spread_s=[min(kept), max(kept)],
           ratio_keep_sorted_over_clip=statistics.median(kept) / statistics.median(plain),
           largest_held_records=held[0], largest_held_bytes=held[1], **sizes)
print(json.dumps(res))
if a.json:  # one file for every configuration measured: {config: result}
    every = json.load(open(a.json)) if os.path.exists(a.json) else {}
    every[a.config] = res
    with open(a.json, "w") as fo:
        json.dump(every, fo, indent=1)
