"""What `fade extract --sorted --write-index` costs: wall time of `fade extract --gpus 1 -b` from the parent commit's binary
(--parent-fade PATH, built elsewhere from the commit before the option), from this tree's binary — which must lie within the
spread of the parent's own repeats: that path launches nothing new — and from this tree's binary with `--sorted --write-index`.
The file is the one-million-read C2 file of tools/fade_out_rate.py, annotated by `fade annotate -b`.  One untimed run, then
--runs timed runs of each leg, interleaved, in this one call.  Then, in a run of its own, `rocprofv3 --kernel-trace --stats`
of the sorted leg: the kernel time of the sort's passes, the gather and the append.  Reported: medians, spreads (min, max),
the sorted run's cost over the unsorted one, the --timing lines of the last sorted run.  No threshold: nobody has measured
this before, and no timing against samtools is claimed.

python tools/extract_sorted_cost.py [--parent-fade PATH] [--reads 1000000] [--runs 5] [--json profiles/extract_sorted_cost.json] [--no-trace]"""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synthgen as sg  # noqa: E402
from fade_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-fade", default="", help="the `fade` binary of the commit before --sorted (its library beside it)")
ap.add_argument("--config", default="C2")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--json", default="")
ap.add_argument("--no-trace", action="store_true")
a = ap.parse_args()
FADE = os.path.join(ROOT, "fade_amd", "fade")

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno, scratch, bai = (os.path.join(tmp, "xsorted_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam", "out.bam", "out.bam.bai"))
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
done = 0
while done < a.reads:
    m = min(1_000_000, a.reads - done)
    w.write(sg.make_reads(g, m, 100 + done // 1_000_000, cfg), done // 2)
    done += m
w.close()
with open(anno, "wb") as fo:
    subprocess.check_call([FADE, "annotate", "-t", str(a.threads), "-w", str(cfg["window"]), "-b", bam, fa], stdout=fo)
print("input: %s, %d reads, %d bytes" % (anno, a.reads, os.path.getsize(anno)), flush=True)


def timed(argv, out_path, env=None):
    t0 = time.perf_counter()
    with open(out_path, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr.decode(errors="replace")


tail = ["--gpus", "1", "--timing", "-t", str(a.threads), "-b", anno]
sorted_argv = [FADE, "extract", "--sorted", "--write-index", bai] + tail
legs = {"new": [FADE, "extract"] + tail, "new_sorted_indexed": sorted_argv}
if a.parent_fade:
    legs = dict(parent=[a.parent_fade, "extract"] + tail, **legs)
times, said, sizes = {k: [] for k in legs}, {}, {}
for rep in range(-1, a.runs):  # (run -1 is not timed)
    for name, argv in legs.items():
        dt, err = timed(argv, scratch)
        if rep >= 0:
            times[name].append(dt)
        said[name] = [l for l in err.splitlines() if l.startswith("[timing]")]
        sizes[name] = os.path.getsize(scratch)
    if rep >= 0:
        print("run %d: %s" % (rep, ", ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
med = {k: statistics.median(v) for k, v in times.items()}
res = dict(config=a.config, reads=a.reads, runs=a.runs, input_bytes=os.path.getsize(anno), output_bytes=sizes, bai_bytes=os.path.getsize(bai),
           seconds=times, median_s=med, spread_s={k: [min(v), max(v)] for k, v in times.items()},
           sorted_over_unsorted_s=med["new_sorted_indexed"] - med["new"], sorted_over_unsorted_ratio=med["new_sorted_indexed"] / med["new"],
           timing_lines_sorted=said["new_sorted_indexed"], parent_measured=bool(a.parent_fade))
if a.parent_fade:
    lo, hi = res["spread_s"]["parent"]
    res["new_within_parent_spread"] = lo <= med["new"] <= hi

if not a.no_trace:
    # the store's kernels alone: one traced run of the sorted leg (the binary leaves by exit(), so that the trace is written)
    d = os.path.join(tmp, "xsorted_trace")
    shutil.rmtree(d, ignore_errors=True)
    timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--"] + sorted_argv, scratch, dict(os.environ, FADE_FAST_EXIT="0"))
    rows, total_ns = {}, 0
    groups = {"recstore_append (count, scan, append)": ("recstore_count", "recstore_append"), "recstore_sort_begin": ("recstore_sort_begin",),
              "sort passes (bam_resort hist, scan, scatter)": ("bam_resort_hist", "bam_resort_scan", "bam_resort_scatter"),
              "cut and offsets (bam_resort cut, offsets_scan, offsets)": ("bam_resort_cut", "bam_resort_offsets"), "recstore_gather": ("recstore_gather",),
              "compressor (bgzf deflate, scan, pack)": ("bgzf_deflate", "bgzf_scan", "bgzf_pack"), "index stage (bam_index_*)": ("bam_index_",)}
    for f in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name, ns, calls = r.get("Name", ""), int(float(r.get("TotalDurationNs", 0) or 0)), int(float(r.get("Calls", 0) or 0))
            total_ns += ns
            for label, keys in groups.items():
                if any(k in name for k in keys):
                    row = rows.setdefault(label, dict(calls=0, total_us=0.0))
                    row["calls"] += calls
                    row["total_us"] += ns / 1e3
    res["store_kernels"] = rows
    res["all_kernels_total_ms"] = total_ns / 1e6
    shutil.rmtree(d, ignore_errors=True)
for p in (scratch, bai, bam, fa, anno):
    if os.path.exists(p):
        os.remove(p)
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
