"""`fade annotate -b --extract x.bam` (one pass) against `fade annotate -b` to a file followed by `fade extract -b` on it (two
passes), wall time of the processes on a synthetic BAM, the two forms interleaved, and `annotate -b` without the option beside
them (the cost of the flag).  The two-step form may run another build (--two-step-fade: the binary of the commit before the
option existed).  The inflated records of the two extract files must be equal.

python tools/extract_fused_vs_two_step.py [--config C2] [--reads 10000000] [--runs 4] [--two-step-fade PATH] [--json OUT]"""
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
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--two-step-fade", default=os.path.join(ROOT, "fade_amd", "fade"))
ap.add_argument("--json", default="")
a = ap.parse_args()

cfg = synth.config(a.config)
tmp = os.environ.get("TMPDIR", "/tmp")
bam, fa = os.path.join(tmp, "extractq_%s.bam" % a.config), os.path.join(tmp, "extractq_%s.fa" % a.config)
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


def records(path):
    import gzip
    import struct
    raw = gzip.decompress(open(path, "rb").read())
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    return raw[at:]


fused, plain, two, two_parts, sizes = [], [], [], [], {}
o1, x1, o2, mid = (os.path.join(tmp, "extractq." + n) for n in ("fused.bam", "fused.extract.bam", "two.extract.bam", "anno.bam"))
for rep in range(a.runs):
    f = timed([FADE, "annotate", "-b", "--extract", x1] + common + [bam, fa], o1)
    t_p = timed([FADE, "annotate", "-b"] + common + [bam, fa], o1)
    t_a = timed([a.two_step_fade, "annotate", "-b"] + common + [bam, fa], mid)
    t_o = timed([a.two_step_fade, "extract", "-b", mid], o2)
    fused.append(f)
    plain.append(t_p)
    two.append(t_a + t_o)
    two_parts.append((t_a, t_o))
    if rep == 0:
        r1, r2 = records(x1), records(o2)
        if r1 != r2:
            sys.exit("the extract files differ: %d against %d bytes of records" % (len(r1), len(r2)))
        sizes = dict(extract_record_bytes=len(r1), annotated_bytes=os.path.getsize(mid), records_equal=True)
    print("run %d: fused %.3f s, annotate -b alone %.3f s, two-step %.3f s (annotate %.3f + extract %.3f)" % (rep, f, t_p, t_a + t_o, t_a, t_o), flush=True)
for p in (o1, x1, o2, mid):
    os.remove(p)
res = dict(config=a.config, reads=a.reads, runs=a.runs, fused_s=fused, annotate_alone_s=plain, two_step_s=two, two_step_parts_s=two_parts,
           fused_median_s=statistics.median(fused), annotate_alone_median_s=statistics.median(plain), two_step_median_s=statistics.median(two),
           fused_spread_s=[min(fused), max(fused)], annotate_alone_spread_s=[min(plain), max(plain)], two_step_spread_s=[min(two), max(two)],
           ratio_two_step_over_fused=statistics.median(two) / statistics.median(fused), **sizes)
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as fo:
        json.dump(res, fo, indent=1)
