"""`fade stats --gpus 1` and `fade stats-clip --gpus 1` on a file annotated earlier, against `fade extract --gpus 1 -b` on the
same file — the run with the same front half and the same NO_OUTPUT shape, the yardstick (--yardstick PATH: the `fade` of the
parent commit; default: this tree's, whose extract path the reports do not touch).  Wall time of the processes on the
synthetic BAM of tools/fade_out_rate.py that `fade annotate -b` has annotated.  One untimed run, then --runs timed runs per
leg, the three legs interleaved.  Reported: the median and the spread (max - min) of each leg, what a report adds to the
yardstick's median, and the rows and bytes each report wrote.

python tools/fade_stats_rate.py [--config C2] [--reads 1000000] [--runs 5] [--threads 16] [--json profiles/fade_stats_rate.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synthgen as sg  # noqa: E402
from fade_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C2")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--yardstick", default="")
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno = (os.path.join(tmp, "statsrate_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam"))
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
done = 0
while done < a.reads:
    m = min(1_000_000, a.reads - done)
    w.write(sg.make_reads(g, m, 100 + done // 1_000_000, cfg), done // 2)
    done += m
w.close()
FADE = os.path.join(ROOT, "fade_amd", "fade")
T = ["-t", str(a.threads)]


def timed(argv, out, on_device=True):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    if on_device and b"file path on the device" not in p.stderr:
        sys.exit("%s did not take the file path on the device: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-800:]))
    return dt


timed([FADE, "annotate", "-b", "-w", str(cfg["window"])] + T + [bam, fa], anno, on_device=False)
print("input: %s, %d reads, %d bytes annotated" % (anno, a.reads, os.path.getsize(anno)), flush=True)
legs = {"extract": [a.yardstick or FADE, "extract", "--gpus", "1", "--timing", "-b"] + T + [anno],
        "stats": [FADE, "stats", "--gpus", "1", "--timing"] + T + [anno],
        "stats_clip": [FADE, "stats-clip", "--gpus", "1", "--timing"] + T + [anno]}
outs = {k: os.path.join(tmp, "statsrate.%s.out" % k) for k in legs}
times = {k: [] for k in legs}
for rep in range(a.runs + 1):  # (the first round is not timed)
    for k in legs:
        dt = timed(legs[k], outs[k])
        if rep:
            times[k].append(dt)
res = dict(config=a.config, reads=a.reads, runs=a.runs, threads=a.threads, input_bytes=os.path.getsize(anno), yardstick=a.yardstick or "fade_amd/fade of this tree", legs={})
for k in legs:
    leg = dict(median_s=statistics.median(times[k]), spread_s=max(times[k]) - min(times[k]), runs_s=[round(t, 4) for t in times[k]],
               output_bytes=os.path.getsize(outs[k]))
    if k != "extract":
        with open(outs[k], "rb") as f:
            leg["rows"] = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b"")) - 1
        leg["added_to_yardstick_s"] = leg["median_s"] - statistics.median(times["extract"])
    res["legs"][k] = leg
    print("%-10s %.3f s (spread %.3f)%s" % (k, leg["median_s"], leg["spread_s"],
                                          "" if k == "extract" else " | %d rows, %+.3f s against the yardstick" % (leg["rows"], leg["added_to_yardstick_s"])), flush=True)
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
