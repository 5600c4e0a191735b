"""`fade annotate --eject -b` (one pass) against `fade annotate -b` to a file followed by `fade out -b` (two passes), wall time
of the processes on a synthetic BAM (name-sorted pairs: the grouped mode), the two forms interleaved.  The two-step form may
run another build (--two-step-fade: the binary of the commit before the option existed).  Nothing is reported when the
records of the two outputs differ.

python tools/eject_fused_vs_two_step.py [--config C2] [--reads 10000000] [--runs 4] [--two-step-fade PATH] [--json OUT]"""
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
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--two-step-fade", default=os.path.join(ROOT, "fade_amd", "fade"))
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa = os.path.join(tmp, "ejectq_%s.bam" % a.config), os.path.join(tmp, "ejectq_%s.fa" % a.config)
g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
g.write_fasta(fa)
w = sg.BamWriter(bam, g)
done = 0
while done < a.reads:
    m = min(1_000_000, a.reads - done)
    w.write(sg.make_reads(g, m, 100 + done // 1_000_000, cfg), done // 2)
    done += m
w.close()
print("input: %s, %d reads, %d bytes" % (bam, a.reads, os.path.getsize(bam)), flush=True)
FADE = os.path.join(ROOT, "fade_amd", "fade")
common = ["-t", "16", "-w", str(cfg["window"])]


def timed(argv, out):
    t0 = time.perf_counter()
    with open(out, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode:
        sys.exit("%s failed: %s" % (" ".join(argv), p.stderr.decode(errors="replace")[-1500:]))
    return dt


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


fused, two, two_parts, sizes = [], [], [], {}
o1, o2, mid = os.path.join(tmp, "ejectq.fused.bam"), os.path.join(tmp, "ejectq.two.bam"), os.path.join(tmp, "ejectq.anno.bam")
for rep in range(a.runs):
    f = timed([FADE, "annotate", "--eject", "-b"] + common + [bam, fa], o1)
    t_a = timed([a.two_step_fade, "annotate", "-b"] + common + [bam, fa], mid)
    t_o = timed([a.two_step_fade, "out", "-b", mid], o2)
    fused.append(f)
    two.append(t_a + t_o)
    two_parts.append((t_a, t_o))
    sizes.update(fused_bytes=os.path.getsize(o1), two_step_bytes=os.path.getsize(o2), annotated_bytes=os.path.getsize(mid))
    if rep == 0:
        d1, d2 = records_digest(o1), records_digest(o2)
        if d1 != d2:
            sys.exit("the two forms' records differ (%d / %d bytes of records): nothing to report" % (d1[1], d2[1]))
        sizes["record_bytes"], sizes["records_sha256"] = d1[1], d1[0]
    print("run %d: fused %.3f s, two-step %.3f s (annotate %.3f + out %.3f)" % (rep, f, t_a + t_o, t_a, t_o), flush=True)
for p in (o1, o2, mid):
    os.remove(p)
res = dict(config=a.config, reads=a.reads, runs=a.runs, fused_s=fused, two_step_s=two, two_step_parts_s=two_parts,
           fused_median_s=statistics.median(fused), two_step_median_s=statistics.median(two),
           fused_spread_s=[min(fused), max(fused)], two_step_spread_s=[min(two), max(two)],
           ratio_two_step_over_fused=statistics.median(two) / statistics.median(fused), **sizes)
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
