"""`fade out --fragments -b` on a shuffled annotated file against the one-pass, records-only eject it stands beside: wall time of
the processes on the annotated synthetic BAM of tools/fade_out_rate.py with its records shuffled (no order a sort would have
left).  The yardstick is `fade out --gpus 1 -b` of ANOTHER build of the driver on the same file (--parent-fade: the parent
commit's binary, which ejects the artifact reads alone and orphans their mates); without one, this build's.  One untimed run
of every leg, then --runs timed runs, the legs interleaved; reported: the median and the spread (max - min) of each leg, the
per-pass --timing lines of the last --fragments run, and how many records each leg wrote.  No ratio is promised: the second
read of the file and the set's kernels are what the option costs, whole fragments are what it buys.

python tools/fade_out_fragments_rate.py [--config C2] [--reads 1000000] [--runs 5] [--threads 16] [--parent-fade PATH]
                                        [--json profiles/fade_out_fragments_rate.json]"""
import argparse
import gzip
import json
import os
import random
import statistics
import struct
import subprocess
import sys
import time
import zlib

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
ap.add_argument("--parent-fade", default="")
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno, shuf = (os.path.join(tmp, "fragrate_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam", "shuffled.bam"))
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
PARENT = a.parent_fade or FADE
T = ["-t", str(a.threads)]
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def timed(argv, out):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr


def split(path):
    """(the bytes in front of the first record, the records) of a BAM file."""
    raw = gzip.open(path, "rb").read()
    at = 12 + struct.unpack_from("<i", raw, 4)[0]
    for _ in range(struct.unpack_from("<i", raw, at - 4)[0]):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    head, recs = raw[:at], []
    while at < len(raw):
        e = at + 4 + struct.unpack_from("<I", raw, at)[0]
        recs.append(raw[at:e])
        at = e
    return head, recs


def write_bgzf(path, data):
    with open(path, "wb") as fo:
        for at in range(0, len(data), 0xff00):
            chunk = data[at:at + 0xff00]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = co.compress(chunk) + co.flush()
            fo.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(body) + 25) + body +
                     struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        fo.write(EOF_MEMBER)


timed([FADE, "annotate", "-b", "-w", str(cfg["window"])] + T + [bam, fa], anno)
head, recs = split(anno)
random.Random(20261019).shuffle(recs)
write_bgzf(shuf, head + b"".join(recs))
del recs
print("input: %s, %d reads shuffled, %d bytes" % (shuf, a.reads, os.path.getsize(shuf)), flush=True)
res = dict(config=a.config, reads=a.reads, runs=a.runs, threads=a.threads, input_bytes=os.path.getsize(shuf), parent_fade=bool(a.parent_fade), legs={})
legs = {"fragments": [FADE, "out", "--fragments", "--timing", "-b"] + T + [shuf],
        "records_only": [PARENT, "out", "--gpus", "1", "--timing", "-b"] + T + [shuf]}
outs = {k: os.path.join(tmp, "fragrate.%s.bam" % k) for k in legs}
times, last_err = {k: [] for k in legs}, {}
for rep in range(a.runs + 1):  # (the first round is not timed)
    for k in legs:
        dt, err = timed(legs[k], outs[k])
        if b"file path on the device" not in err:
            sys.exit("%s did not take the file path on the device: %s" % (k, err.decode(errors="replace")[-800:]))
        last_err[k] = err.decode(errors="replace")
        if rep:
            times[k].append(dt)
for k in legs:
    res["legs"][k] = dict(median_s=statistics.median(times[k]), spread_s=max(times[k]) - min(times[k]), runs_s=[round(t, 4) for t in times[k]],
                          records_written=len(split(outs[k])[1]), timing=[l for l in last_err[k].splitlines() if l.startswith("[timing]")])
    print("%-13s %.3f s (spread %.3f), %d records written" % (k, res["legs"][k]["median_s"], res["legs"][k]["spread_s"], res["legs"][k]["records_written"]), flush=True)
    for l in res["legs"][k]["timing"]:
        print("    " + l, flush=True)
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
