"""What `--write-index` costs: wall time of `fade annotate -b` with and without the option, the same binary, the two forms
interleaved, on a synthetic BAM whose records this tool sorts by coordinate itself (the generator deals reads in random
order); then the index stage's kernel time from one `rocprofv3 --kernel-trace --stats` run of its own with the option.

python tools/write_index_cost.py [--config C2] [--reads 4000000] [--runs 4] [--json OUT] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import shutil
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
ap.add_argument("--no-trace", action="store_true")
a = ap.parse_args()


def sorted_batch(b):
    """The batch in stable coordinate order: by (refID as uint32, pos + 1 as uint32), the key the index rule checks."""
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
bam, fa = os.path.join(tmp, "wixq_%s.bam" % a.config), os.path.join(tmp, "wixq_%s.fa" % a.config)
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
w.write(sorted_batch(sg.make_reads(g, a.reads, 100, cfg)), 0)
w.close()
print("input: %s, %d reads sorted by coordinate, %d bytes" % (bam, a.reads, os.path.getsize(bam)), flush=True)
FADE = os.path.join(ROOT, "fade_amd", "fade")
common = ["--timing", "-t", "16", "-w", str(cfg["window"])]
o1, o2, bai = os.path.join(tmp, "wixq.plain.bam"), os.path.join(tmp, "wixq.indexed.bam"), os.path.join(tmp, "wixq.indexed.bam.bai")


def timed(argv, out, env=None):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt


plain, indexed, sizes = [], [], {}
for rep in range(a.runs):
    t_p = timed([FADE, "annotate", "-b"] + common + [bam, fa], o1)
    t_i = timed([FADE, "annotate", "-b", "--write-index", bai] + common + [bam, fa], o2)
    plain.append(t_p)
    indexed.append(t_i)
    sizes = dict(bam_bytes=os.path.getsize(o2), bai_bytes=os.path.getsize(bai))
    print("run %d: -b %.3f s, -b --write-index %.3f s; .bai %d bytes" % (rep, t_p, t_i, sizes["bai_bytes"]), flush=True)
res = dict(config=a.config, reads=a.reads, runs=a.runs, plain_s=plain, write_index_s=indexed,
           plain_median_s=statistics.median(plain), write_index_median_s=statistics.median(indexed),
           plain_spread_s=[min(plain), max(plain)], write_index_spread_s=[min(indexed), max(indexed)],
           ratio_write_index_over_plain=statistics.median(indexed) / statistics.median(plain), **sizes)

if not a.no_trace:
    # the stage's kernels alone: one traced run with the option (the binary leaves by exit(), so that the trace is written)
    d = os.path.join(tmp, "wixq_trace")
    shutil.rmtree(d, ignore_errors=True)
    env = dict(os.environ, FADE_FAST_EXIT="0")
    timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
           FADE, "annotate", "-b", "--write-index", bai] + common + [bam, fa], o2, env)
    rows, total_ns = {}, 0
    for f in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name, ns, calls = r.get("Name", ""), int(float(r.get("TotalDurationNs", 0) or 0)), int(float(r.get("Calls", 0) or 0))
            total_ns += ns
            if "bam_index_" in name:
                short = name.split("bam_index_")[1].split("(")[0].split("ENS")[0]
                rows["bam_index_" + short] = dict(calls=calls, total_us=ns / 1e3)
    res["stage_kernels"] = rows
    res["stage_kernels_total_ms"] = sum(v["total_us"] for v in rows.values()) / 1e3
    res["all_kernels_total_ms"] = total_ns / 1e6
    shutil.rmtree(d, ignore_errors=True)
for p in (o1, o2, bai):
    if os.path.exists(p):
        os.remove(p)
print(json.dumps(res))
if a.json:  # one file for every configuration measured: {config: result}
    every = json.load(open(a.json)) if os.path.exists(a.json) else {}
    every[a.config] = res
    with open(a.json, "w") as fo:
        json.dump(every, fo, indent=1)
