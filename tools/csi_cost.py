"""What `--write-index --csi` costs against the BAI it stands in for: wall time of `fade out --gpus 1 -b --write-index` writing
a .bai with the PARENT commit's build against `--write-index --csi` with this build, on the workload of
tools/write_index_cost.py — synthetic reads this tool sorts by coordinate itself, one million by default —, annotated once
with this build.  The two binaries run interleaved, the same number of times each, behind one warm-up run each that is not
counted (the first run pays the page cache and the device's first use); medians and the min .. max spread are reported, and
whether the difference of the medians is larger than the wider of the two spreads.

python tools/csi_cost.py --parent-fade PATH/TO/PARENT/fade [--config C2] [--reads 1000000] [--runs 7] [--json OUT]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ap = argparse.ArgumentParser()
ap.add_argument("--parent-fade", required=True, help="the `fade` binary of the parent commit's build (its libfadehip.so beside it)")
ap.add_argument("--config", default="C2")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--json", default="")
a = ap.parse_args()

import synthgen as sg  # noqa: E402
from fade_amd import synth  # noqa: E402


def sorted_batch(b):
    """(tools/write_index_cost.py's.)  The batch in stable coordinate order: by (refID as uint32, pos + 1 as uint32), the key the index rule checks."""
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
bam, fa, anno = (os.path.join(tmp, "csiq_%s.%s" % (a.config, e)) for e in ("bam", "fa", "anno.bam"))
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
w.write(sorted_batch(sg.make_reads(g, a.reads, 100, cfg)), 0)
w.close()
FADE = os.path.join(ROOT, "fade_amd", "fade")
PARENT = os.path.abspath(a.parent_fade)
out, bai, csi = (os.path.join(tmp, "csiq.out." + e) for e in ("bam", "bai", "csi"))


def timed(argv, to):
    t0 = time.perf_counter()
    with open(to, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt


timed([FADE, "annotate", "-b", "-t", "16", "-w", str(cfg["window"]), bam, fa], anno)
print("input: %s, %d reads sorted by coordinate and annotated, %d bytes" % (anno, a.reads, os.path.getsize(anno)), flush=True)
forms = dict(parent_bai=[PARENT, "out", "--gpus", "1", "-t", "16", "-b", "--write-index", bai, anno],
             csi=[FADE, "out", "--gpus", "1", "-t", "16", "-b", "--write-index", csi, "--csi", anno])
for argv in forms.values():  # warm-up: not counted
    timed(argv, out)
times = {k: [] for k in forms}
for rep in range(a.runs):
    for k, argv in forms.items():
        times[k].append(timed(argv, out))
    print("run %d: parent .bai %.3f s, --csi %.3f s" % (rep, times["parent_bai"][-1], times["csi"][-1]), flush=True)
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: max(v) - min(v) for k, v in times.items()}
diff = med["csi"] - med["parent_bai"]
res = dict(config=a.config, reads=a.reads, runs=a.runs, warm_up_runs=1, command="fade out --gpus 1 -t 16 -b --write-index PATH [--csi]",
           parent_bai_s=times["parent_bai"], csi_s=times["csi"], parent_bai_median_s=med["parent_bai"], csi_median_s=med["csi"],
           parent_bai_spread_s=[min(times["parent_bai"]), max(times["parent_bai"])], csi_spread_s=[min(times["csi"]), max(times["csi"])],
           csi_minus_parent_bai_median_s=diff, ratio_csi_over_parent_bai=med["csi"] / med["parent_bai"],
           difference_beyond_spread=abs(diff) > max(spread.values()),
           bai_bytes=os.path.getsize(bai), csi_bytes=os.path.getsize(csi), output_bam_bytes=os.path.getsize(out))
for p in (bam, fa, anno, out, bai, csi):
    if os.path.exists(p):
        os.remove(p)
print(json.dumps(res))
if a.json:  # one file for every configuration measured: {config: result}
    every = json.load(open(a.json)) if os.path.exists(a.json) else {}
    every[a.config] = res
    with open(a.json, "w") as fo:
        json.dump(every, fo, indent=1)
