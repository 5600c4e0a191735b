"""`fade out -b`, `fade out -c -b` and `fade extract -b` on a file annotated earlier, with and without `--gpus 1`: wall time of
the processes on a synthetic BAM (name-sorted pairs: `fade out` takes the grouped mode) that `fade annotate -b` has annotated.
Every leg is one untimed run, then --runs timed runs; the legs of a subcommand are interleaved.  Reported: the median and the
spread (max - min) of each leg.  The yardstick is the host loop; a leg is "faster" only when the medians are apart by more than
the host runs' own spread.  Nothing is reported for a subcommand whose two outputs hold different records.

python tools/fade_out_rate.py [--config C2] [--reads 1000000] [--runs 5] [--threads 16] [--json profiles/fade_out_rate.json]"""
import argparse
import gzip
import hashlib
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
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno = (os.path.join(tmp, "outrate_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam"))
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


def timed(argv, out):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr


def records_digest(path):
    """sha256 of the BAM's record bytes (everything behind the header and the reference list), and their number of bytes."""
    h, n = hashlib.sha256(), 0
    with gzip.open(path, "rb") as f:
        l_text = int.from_bytes(f.read(8)[4:], "little")
        f.read(l_text)
        for _ in range(int.from_bytes(f.read(4), "little")):
            f.read(int.from_bytes(f.read(4), "little") + 4)
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            h.update(b)
            n += len(b)
    return h.hexdigest(), n


timed([FADE, "annotate", "-b", "-w", str(cfg["window"])] + T + [bam, fa], anno)
print("input: %s, %d reads, %d bytes annotated" % (anno, a.reads, os.path.getsize(anno)), flush=True)
res = dict(config=a.config, reads=a.reads, runs=a.runs, threads=a.threads, input_bytes=os.path.getsize(anno), legs={})
for name, sub in (("out", ["out"]), ("out_c", ["out", "-c"]), ("extract", ["extract"])):
    outs = {k: os.path.join(tmp, "outrate.%s.%s.bam" % (name, k)) for k in ("host", "device")}
    argv = {"host": [FADE] + sub + ["-b"] + T + [anno], "device": [FADE] + sub + ["--gpus", "1", "--timing", "-b"] + T + [anno]}
    times = {"host": [], "device": []}
    for rep in range(a.runs + 1):  # (the first round is not timed)
        for k in ("host", "device"):
            dt, err = timed(argv[k], outs[k])
            if k == "device" and b"file path on the device" not in err:
                sys.exit("%s did not take the file path on the device: %s" % (name, err.decode(errors="replace")[-800:]))
            if rep:
                times[k].append(dt)
    dig = {k: records_digest(outs[k]) for k in outs}
    if dig["host"] != dig["device"]:
        sys.exit("%s: the records differ (%s against %s): nothing to report" % (name, dig["host"], dig["device"]))
    leg = {}
    for k in times:
        leg[k] = dict(median_s=statistics.median(times[k]), spread_s=max(times[k]) - min(times[k]), runs_s=[round(t, 4) for t in times[k]])
    gap = leg["host"]["median_s"] - leg["device"]["median_s"]
    leg["record_bytes"] = dig["host"][1]
    leg["verdict"] = "device faster" if gap > leg["host"]["spread_s"] else "host faster" if -gap > leg["host"]["spread_s"] else "not apart by more than the host runs' spread"
    res["legs"][name] = leg
    print("%-8s host %.3f s (spread %.3f) | --gpus 1 %.3f s (spread %.3f) | %s" %
          (name, leg["host"]["median_s"], leg["host"]["spread_s"], leg["device"]["median_s"], leg["device"]["spread_s"], leg["verdict"]), flush=True)
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
