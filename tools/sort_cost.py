"""What `fade out --sort` costs: wall time of `fade out -c -b --gpus 1` from the parent commit's binary (--parent-fade PATH, built
elsewhere from the commit before the option), from this tree's binary — expected inside the spread of the parent's own
repeats: that path launches nothing new — from this tree's binary with `-c --sort`, from the same with FADEHIP_RECSTORE_BUDGET
set so that the file leaves in about four windows, and from plain `fade out --sort --write-index` (under -c a file of this
size has reads that clip to nothing, which `--write-index` refuses).  The file is the one-million-read C2 file of
tools/fade_out_rate.py, annotated by `fade annotate -b`, its records shuffled here (seeded).  One untimed run, then --runs timed
runs of each leg, interleaved, in this one call.  Then, in a run of its own, `rocprofv3 --kernel-trace --stats` of the
sorted and indexed leg: the kernel time of bam_sortwin_kernel, the append, the sort's passes (bam_resort_scan_kernel, one block,
also by itself), the gather, the compressor and the index stage.  Reported: medians, spreads (min, max), the --timing lines,
and the store's arrays as its exact counts size them (records and bytes written; 20 bytes of items and 37 of sort arrays per
record).  No threshold, and no timing against samtools is claimed.

python tools/sort_cost.py [--parent-fade PATH] [--reads 1000000] [--runs 5] [--json profiles/sort_cost.json] [--no-trace]"""
import argparse
import gzip
import random
import struct
import zlib
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
ap.add_argument("--parent-fade", default="", help="the `fade` binary of the commit before --sort (its library beside it)")
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
bam, fa, anno, scratch, bai = (os.path.join(tmp, "sortcost_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam", "out.bam", "out.bam.bai"))
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


def bgzf(payload):
    out = []
    for at in range(0, len(payload), 0xff00):
        p = payload[at:at + 0xff00]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        d = c.compress(p) + c.flush()
        out.append(b"\x1f\x8b\x08\x04" + bytes(6) + b"\x06\x00BC\x02\x00" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out)


# the annotated records in a seeded random order (the header's members of their own, so that the first record starts a member)
raw = gzip.decompress(open(anno, "rb").read())
at = 8 + struct.unpack_from("<i", raw, 4)[0]
for _ in range(struct.unpack_from("<i", raw, at)[0]):
    at += 8 + struct.unpack_from("<i", raw, at + 4)[0]
at += 4
offs, p = [], at
while p < len(raw):
    offs.append(p)
    p += 4 + struct.unpack_from("<I", raw, p)[0]
offs.append(p)
order = list(range(len(offs) - 1))
random.Random(20261021).shuffle(order)
rec_bytes = len(raw) - at
with open(anno, "wb") as fo:
    fo.write(bgzf(raw[:at]))
    fo.write(bgzf(b"".join(raw[offs[k]:offs[k + 1]] for k in order)))
    fo.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
n_records = len(order)
del raw
print("input: %s, %d reads shuffled, %d bytes, %d bytes of records" % (anno, n_records, os.path.getsize(anno), rec_bytes), flush=True)


def timed(argv, out_path, env=None):
    t0 = time.perf_counter()
    with open(out_path, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr.decode(errors="replace")


tail = ["-c", "--gpus", "1", "--timing", "-t", str(a.threads), "-b", anno]
sorted_argv = [FADE, "out", "--sort"] + tail   # (no --write-index under -c: a file of this size has reads that clip to nothing, and such a file cannot be indexed)
indexed_argv = [FADE, "out", "--sort", "--write-index", bai] + tail[1:]   # plain `fade out` (the artifact reads ejected): sorted AND indexed
budget = (rec_bytes + 64 * n_records) * 10 // 35   # (the clip shortens some records: about four windows)
legs = {"new": [FADE, "out"] + tail, "new_sorted": sorted_argv, "new_sorted_windows": sorted_argv, "new_eject_sorted_indexed": indexed_argv}
envs = {"new_sorted_windows": dict(os.environ, FADEHIP_RECSTORE_BUDGET=str(budget))}
if a.parent_fade:
    legs = dict(parent=[a.parent_fade, "out"] + tail, **legs)
times, said, sizes = {k: [] for k in legs}, {}, {}
for rep in range(-1, a.runs):  # (run -1 is not timed)
    for name, argv in legs.items():
        dt, err = timed(argv, scratch, envs.get(name))
        if rep >= 0:
            times[name].append(dt)
        said[name] = [l for l in err.splitlines() if l.startswith("[timing]") or "--sort:" in l]
        sizes[name] = os.path.getsize(scratch)
    if rep >= 0:
        print("run %d: %s" % (rep, ", ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
med = {k: statistics.median(v) for k, v in times.items()}
res = dict(config=a.config, reads=a.reads, runs=a.runs, input_bytes=os.path.getsize(anno), output_bytes=sizes, bai_bytes=os.path.getsize(bai) if os.path.exists(bai) else 0,
           seconds=times, median_s=med, spread_s={k: [min(v), max(v)] for k, v in times.items()},
           sorted_over_unsorted_s=med["new_sorted"] - med["new"], sorted_over_unsorted_ratio=med["new_sorted"] / med["new"],
           windows_over_one_window_s=med["new_sorted_windows"] - med["new_sorted"], windows_budget_bytes=budget,
           said_sorted=said["new_sorted"], said_windows=said["new_sorted_windows"], said_eject_sorted_indexed=said["new_eject_sorted_indexed"], parent_measured=bool(a.parent_fade),
           store_input=dict(records=n_records, record_bytes_before_clip=rec_bytes, item_array_bytes=20 * n_records, sort_array_bytes=37 * n_records))
if a.parent_fade:
    lo, hi = res["spread_s"]["parent"]
    res["new_within_parent_spread"] = lo <= med["new"] <= hi

if not a.no_trace:
    # the store's kernels alone: one traced run of the sorted leg (the binary leaves by exit(), so that the trace is written)
    d = os.path.join(tmp, "sortcost_trace")
    shutil.rmtree(d, ignore_errors=True)
    timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--"] + indexed_argv, scratch, dict(os.environ, FADE_FAST_EXIT="0"))
    rows, total_ns = {}, 0
    groups = {"bam_sortwin_kernel": ("bam_sortwin_kernel",), "bam_sortwin_rekey_kernel": ("bam_sortwin_rekey",), "bam_resort_scan_kernel alone (one block)": ("bam_resort_scan",),
              "recstore_append (count, scan, append)": ("recstore_count", "recstore_append"), "recstore_sort_begin": ("recstore_sort_begin",),
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
