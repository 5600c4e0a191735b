#!/usr/bin/env python3
"""How long `fade annotate` takes from process start until the genome is resident on the device, for the two FASTA loaders.

    python tools/genome_load_rate.py WORKDIR [--bases N] [--runs K] [--parent-fade PATH] [--out profiles/genome_load.json]

Writes under WORKDIR a 60-column FASTA of N bases (default 10^9) in 25 large and 3,000 short contigs, its .fai, a BGZF copy
(64 KB members, zlib level 6, as bgzip writes them) with the same index, and a SAM whose header names every contig.  Then,
with the files in the page cache (one untimed run first), it runs `fade annotate --timing` K times per file and loader and reads
the time at which the genome was resident off stderr:

  * this build with the index beside the FASTA (fadehip_genome_upload_fasta: the library reads the file, the device packs it);
  * this build under FADE_FASTA_INDEX=0 (the whole-file loader);
  * with --parent-fade, the `fade` of another build (the commit before: a clean checkout, built) — it has no index path and no
    "genome resident" line, so its figure is "annotate begins" + its own "fasta" + "create+genome upload" clocks.

Per series: every run, the median, the spread (max - min), the peak host RSS of the whole process (ru_maxrss from wait4:
the annotate pipeline's own buffers come after the genome and count too) and, where `--timing` prints them, the host's peak
RSS at the moment the genome is resident and the seconds of the upload call alone.  Needs the GPU.
"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LARGE, N_SHORT, LINE = 25, 3000, 60
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def contig_lengths(total):
    short = [500 + (k * 7919) % 4500 for k in range(N_SHORT)]
    rest = total - sum(short)
    weights = np.array([25 - 0.8 * k for k in range(N_LARGE)])  # a largest-to-smallest spread like chr1 .. chr22, X, Y
    large = [int(rest * w / weights.sum()) // 2 * 2 + 1 for w in weights]
    return [("chr%d" % (k + 1), n) for k, n in enumerate(large)] + [("scaffold_%04d" % k, n) for k, n in enumerate(short)]


def write_fasta(path, contigs, seed=20261018):
    """The file, and its index worked out while writing."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fai, at = [], 0
    with open(path, "wb") as f:
        for name, n in contigs:
            head = b">" + name.encode() + b"\n"
            f.write(head)
            at += len(head)
            fai.append((name, n, at, LINE, LINE + 1))
            for a in range(0, n, LINE << 20):
                m = min(LINE << 20, n - a)
                bases = ACGT[rng.integers(0, 4, size=m, dtype=np.uint8)]
                full = m // LINE
                block = np.full((full, LINE + 1), 10, dtype=np.uint8)
                block[:, :LINE] = bases[:full * LINE].reshape(full, LINE)
                block.tofile(f)
                at += block.size
                if m % LINE:
                    f.write(bases[full * LINE:].tobytes() + b"\n")
                    at += m % LINE + 1
    return fai


def write_fai(path, fai):
    with open(path, "w") as f:
        for e in fai:
            f.write("%s\t%d\t%d\t%d\t%d\n" % e)


def _member(payload):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 12 + 6 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def write_bgzf(src, dst, threads=16, block=0xff00):
    """src as BGZF members of 0xff00 payload bytes plus the end-of-file member (zlib releases the GIL: a thread pool)."""
    with open(src, "rb") as f, open(dst, "wb") as g, ThreadPoolExecutor(threads) as pool:
        while True:
            chunk = f.read(block * 64 * threads)
            if not chunk:
                break
            for m in pool.map(_member, [chunk[a:a + block] for a in range(0, len(chunk), block)]):
                g.write(m)
        g.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00")


def write_sam(path, contigs):
    with open(path, "w") as f:
        f.write("@HD\tVN:1.6\tSO:unsorted\n")
        for name, n in contigs:
            f.write("@SQ\tSN:%s\tLN:%d\n" % (name, n))
        f.write("r0\t0\tchr1\t1001\t60\t10S40M\t*\t0\t0\t%s\t%s\n" % ("ACGT" * 12 + "AC", "I" * 50))


def resident_seconds(stderr):
    """(seconds from process start to genome resident, loader named by --timing or None, seconds inside the upload call or None,
    host peak RSS in MB when the genome is resident or None)."""
    m = re.search(r"\[timing\] genome: (.*?), .*?([0-9.]+) s to upload; since process start ([0-9.]+) s \(genome resident\), host peak (\d+) MB", stderr)
    if m:
        return float(m.group(3)), ("indexed" if m.group(1).startswith("indexed") else "whole-file"), float(m.group(2)), int(m.group(4))
    begins = re.search(r"since process start ([0-9.]+) s \(annotate begins", stderr)
    clocks = re.search(r"\[timing\] total [0-9.]+ s: fasta ([0-9.]+), create\+genome upload ([0-9.]+)", stderr)
    if not (begins and clocks):
        raise RuntimeError("no genome timing in:\n" + stderr[-2000:])
    return float(begins.group(1)) + float(clocks.group(1)) + float(clocks.group(2)), None, None, None


def series(fade, sam, fasta, runs, env):
    e = dict(os.environ)
    e.pop("FADE_FASTA_INDEX", None)
    e.update(env)
    out = []
    for k in range(runs + 1):  # the first run only warms the page cache
        with tempfile.TemporaryFile() as err:
            p = subprocess.Popen([fade, "annotate", "--timing", sam, fasta], stdout=subprocess.DEVNULL, stderr=err, env=e)
            _, status, ru = os.wait4(p.pid, 0)  # (ru_maxrss of this child alone, in KB)
            p.returncode = os.waitstatus_to_exitcode(status)
            err.seek(0)
            text = err.read().decode()
        if p.returncode != 0:
            raise RuntimeError("%s failed:\n%s" % (fade, text[-2000:]))
        r = resident_seconds(text) + (ru.ru_maxrss / 1024.0,)
        if k:
            out.append(r)
        print("  run %d: %s" % (k, r), flush=True)
    t = sorted(r[0] for r in out)
    up = [r[2] for r in out if r[2] is not None]
    return {"runs_s": [r[0] for r in out], "median_s": float(np.median(t)), "spread_s": round(t[-1] - t[0], 4), "loader": out[0][1],
            "upload_call_median_s": float(np.median(up)) if up else None,
            "peak_rss_mb_at_genome_resident": max(r[3] for r in out) if out[0][3] is not None else None,
            "peak_rss_mb_whole_run": round(max(r[4] for r in out), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("workdir")
    ap.add_argument("--bases", type=float, default=1e9)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-fade", default=None, help="`fade` of the build to compare with (the commit before)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genome_load.json"))
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, gz, sam = (os.path.join(a.workdir, n) for n in ("ref.fa", "ref.fa.gz", "in.sam"))
    contigs = contig_lengths(int(a.bases))
    print("writing %s (%d bases in %d contigs)" % (fa, sum(n for _, n in contigs), len(contigs)), flush=True)
    fai = write_fasta(fa, contigs)
    write_fai(fa + ".fai", fai)
    print("writing %s" % gz, flush=True)
    write_bgzf(fa, gz)
    write_fai(gz + ".fai", fai)
    write_sam(sam, contigs)
    fade = os.path.join(ROOT, "fade_amd", "fade")
    res = {"bases": sum(n for _, n in contigs), "contigs": len(contigs), "line_bases": LINE, "runs": a.runs,
           "bytes": {"plain": os.path.getsize(fa), "bgzf": os.path.getsize(gz)},
           "what": "seconds from process start to genome resident (fade annotate --timing), warm page cache", "series": {}}
    for label, path in (("plain", fa), ("bgzf", gz)):
        todo = [("indexed", fade, {}), ("whole_file", fade, {"FADE_FASTA_INDEX": "0"})]
        if a.parent_fade:
            todo.append(("parent", a.parent_fade, {}))
        for who, exe, env in todo:
            print("%s, %s" % (label, who), flush=True)
            s = series(exe, sam, path, a.runs, env)
            assert who == "parent" or s["loader"] == {"indexed": "indexed", "whole_file": "whole-file"}[who], s
            res["series"]["%s/%s" % (label, who)] = s
        base = res["series"]["%s/%s" % (label, "parent" if a.parent_fade else "whole_file")]
        new = res["series"][label + "/indexed"]
        res["series"][label + "/factor"] = {"old_over_new": base["median_s"] / new["median_s"], "old": "parent" if a.parent_fade else "whole_file",
                                            "faster_by_more_than_the_old_spread": base["median_s"] - new["median_s"] > base["spread_s"]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["series"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
