"""What `fade out -c --fix-mates` costs: wall time of `fade out -c --keep-sorted -b` from the parent commit's binary (--parent-fade
PATH, built elsewhere from the commit before the option), from this tree's binary, and from this tree's binary with
`--fix-mates` — three passes over the file against one.  The file is the one-million-read C2 file of tools/fade_out_rate.py,
annotated by `fade annotate -b`, given mate information from unclipped geometry (the generator writes none: every pair of
reads of one name becomes segments 1 and 2, every second fragment gets an MC:Z field, and the rule itself — the mate map on
the device, with rs 0 everywhere — writes next_refID, next_pos, tlen, the flags and MC) and sorted by coordinate.
One untimed run, then --runs timed runs of each leg, interleaved.  Reported: medians, spreads (min, max), and the --timing
lines of the last run with the option.  No threshold: nobody has measured three passes against one before.

python tools/fix_mates_cost.py [--parent-fade PATH] [--reads 1000000] [--runs 5] [--json profiles/fix_mates_cost.json] [--keep-input]"""
import argparse
import gzip
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synthgen as sg  # noqa: E402
import fade_amd  # noqa: E402
from fade_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-fade", default="", help="the `fade` binary of the commit before --fix-mates (its library beside it)")
ap.add_argument("--config", default="C2")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--json", default="")
ap.add_argument("--keep-input", action="store_true", help="leave the prepared file where it is (its path is printed), for a profiler run of its own")
a = ap.parse_args()
FADE = os.path.join(ROOT, "fade_amd", "fade")
EOF_MEMBER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa, anno, paired = (os.path.join(tmp, "fixmates_%s.%s" % (a.config, x)) for x in ("bam", "fa", "anno.bam", "paired.bam"))
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

# ---- mate information from unclipped geometry, by the rule itself; then coordinate order
raw = gzip.decompress(open(anno, "rb").read())
l_text, = struct.unpack_from("<i", raw, 4)
at = 8 + l_text
n_ref, = struct.unpack_from("<i", raw, at)
at += 4
for _ in range(n_ref):
    at += 8 + struct.unpack_from("<i", raw, at)[0]
head, recs, k = raw[:at], [], 0
while at < len(raw):
    n = 4 + struct.unpack_from("<I", raw, at)[0]
    r = bytearray(raw[at:at + n])
    flag, = struct.unpack_from("<H", r, 18)
    struct.pack_into("<H", r, 18, (flag & ~0xC1) | 1 | (0x40 if k % 2 == 0 else 0x80))  # (the file holds name-sorted pairs)
    if (k // 2) % 2 == 0:  # every second fragment carries MC: a placeholder the rule fills
        r += b"MCZ*\0"
        struct.pack_into("<I", r, 0, len(r) - 4)
    recs.append(bytes(r))
    at += n
    k += 1
del raw
ctx = fade_amd.Context(device=0)
out, STEP = [], 200_000  # (an even number: a fragment's two reads lie in one call)
for lo in range(0, len(recs), STEP):
    part = recs[lo:lo + STEP]
    zero = np.zeros(len(part), np.int32)
    ms = ctx.mateset()
    ms.add_batch(part, zero, zero, zero)
    fixed_recs, fixed = ms.fix_batch(part, zero, zero, zero)
    ms.close()
    out += fixed_recs
ctx.close()
keys = np.array([((struct.unpack_from("<i", r, 4)[0] & 0xffffffff) << 32) | ((struct.unpack_from("<i", r, 8)[0] + 1) & 0xffffffff) for r in out], dtype=np.uint64)
order = np.argsort(keys, kind="stable")
body = head + b"".join(out[i] for i in order)
with open(paired, "wb") as fo:
    for lo in range(0, len(body), 0xff00):
        chunk = body[lo:lo + 0xff00]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        data = co.compress(chunk) + co.flush()
        fo.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(data) + 25) + data + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    fo.write(EOF_MEMBER)
n_reads = len(out)
del out, recs, body
print("input: %s, %d reads with mate information, sorted by coordinate, %d bytes" % (paired, n_reads, os.path.getsize(paired)), flush=True)


def timed(argv, out_path):
    t0 = time.perf_counter()
    with open(out_path, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt, p.stderr.decode(errors="replace")


tail = ["--timing", "-t", str(a.threads), "-b", paired]
legs = {"new": [FADE, "out", "-c", "--keep-sorted"] + tail, "new_fix_mates": [FADE, "out", "-c", "--keep-sorted", "--fix-mates"] + tail}
if a.parent_fade:
    legs = dict(parent=[a.parent_fade, "out", "-c", "--keep-sorted"] + tail, **legs)
times, said, sizes = {k: [] for k in legs}, {}, {}
scratch = os.path.join(tmp, "fixmates.out.bam")
for rep in range(-1, a.runs):  # (run -1 is not timed)
    for name, argv in legs.items():
        dt, err = timed(argv, scratch)
        if rep >= 0:
            times[name].append(dt)
        said[name] = [l for l in err.splitlines() if l.startswith("[timing]")]
        sizes[name] = os.path.getsize(scratch)
    if rep >= 0:
        print("run %d: %s" % (rep, ", ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
in_bytes = os.path.getsize(paired)
for p in (scratch, bam, anno, fa) + (() if a.keep_input else (paired,)):
    if os.path.exists(p):
        os.remove(p)
res = dict(config=a.config, reads=n_reads, runs=a.runs, input_bytes=in_bytes, output_bytes=sizes,
           seconds=times, median_s={k: statistics.median(v) for k, v in times.items()}, spread_s={k: [min(v), max(v)] for k, v in times.items()},
           timing_lines_fix_mates=said["new_fix_mates"], parent_measured=bool(a.parent_fade))
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
