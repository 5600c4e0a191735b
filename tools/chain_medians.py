"""A slot's chain between its score passes, from a kernel trace of the two-slot streamed loop.
  python tools/chain_medians.py loop [batches]    the loop itself: C2, 1 M records a batch, two slots, the benchmark's
                                                  upload / run / results order (run it under rocprofv3 --kernel-trace)
  python tools/chain_medians.py solo [batches]    solo batches (one slot, serial): gate_ms of last_profile, one line
  python tools/chain_medians.py summary DIR       medians over the last 40 score kernels of the trace under DIR
FADEHIP_LIB chooses the library, as everywhere."""
import csv
import glob
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fade_amd
    from fade_amd import synth
    import synthgen as sg
    cfg = synth.config("C2")
    g = sg.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
    ctx = fade_amd.Context(device=0)
    ctx.genome_upload(g.names, g.ascii_contigs())
    pinned = [ctx.pinned_batch(sg.with_bounds(sg.make_reads(g, 1_000_000, 100 * (k + 1), cfg))) for k in range(4)]
    return ctx, cfg, pinned


def loop(reps):
    ctx, cfg, pinned = _setup()
    n_slots, nb = 2, len(pinned)
    busy = [False] * n_slots
    for seq in range(reps):
        slot = seq % n_slots
        if busy[slot]:
            ctx.annotate_results(slot)
        if seq < n_slots:
            ctx.annotate_upload(slot, pinned[seq % nb])
        ctx.annotate_run(slot, cfg["floor_len"], cfg["window"])
        busy[slot] = True
        if seq + n_slots < reps:
            ctx.annotate_upload(slot, pinned[(seq + n_slots) % nb])
    for slot in range(n_slots):
        if busy[slot]:
            ctx.annotate_results(slot)
    ctx.close()


def solo(reps):
    ctx, cfg, pinned = _setup()
    out = []
    for k in range(reps + 2):
        ctx.annotate_upload(0, pinned[k % len(pinned)])
        ctx.annotate_run(0, cfg["floor_len"], cfg["window"])
        ctx.annotate_results(0)
        if k >= 2:
            out.append(ctx.last_profile(0)["gate_ms"])
    print("gate_ms of %d solo batches: %s; median %.4f" % (reps, " ".join("%.4f" % x for x in out), statistics.median(out)))
    ctx.close()


def summary(d):
    kf = glob.glob(d + "/**/*_kernel_trace.csv", recursive=True)[0]
    kinds = {"score": [], "pass2": [], "gate": [], "gather": []}
    for r in csv.DictReader(open(kf)):
        name = r["Kernel_Name"]
        m = re.search(r"sw_pk_kernel<\d+, (\d)", name)
        kind = ("score" if m.group(1) == "1" else "pass2") if m else "gate" if "gate_kernel" in name else "gather" if "patch_gather" in name else None
        if kind:
            kinds[kind].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for v in kinds.values():
        v.sort()
    sc, gt, p2 = kinds["score"], kinds["gate"], kinds["pass2"]
    assert len(sc) == len(gt), (len(sc), len(gt))  # batch k: the k-th gate and the k-th score kernel (the two slots alternate)
    n, first = len(sc), max(0, len(sc) - 40)
    us = lambda x: x / 1e3
    med = lambda xs: statistics.median(xs) if xs else float("nan")
    a = [us(gt[k + 2][0] - sc[k][1]) for k in range(first, n - 2)]
    b = [us(sc[k + 2][0] - gt[k + 2][0]) for k in range(first, n - 2)]
    c = [us(max(0, sc[k][1] - sc[k + 1][0])) for k in range(first, n - 1)]
    print("kernels: %d score, %d gate, %d pass2, %d gather" % (n, len(gt), len(p2), len(kinds["gather"])))
    print("score kernel: median %.1f us; start-to-start %.1f us" % (med([us(e - s) for s, e in sc[first:]]), med([us(sc[k + 1][0] - sc[k][0]) for k in range(first, n - 1)])))
    print("gate: median %.1f us; pass 2: median %.1f us" % (med([us(e - s) for s, e in gt[first:]]), med([us(e - s) for s, e in p2[first:]])))
    print("(a) median %.1f us (min %.1f, max %.1f)" % (med(a), min(a), max(a)))
    print("(b) median %.1f us (min %.1f, max %.1f)" % (med(b), min(b), max(b)))
    print("(a)+(b): median %.1f us" % med([x + y for x, y in zip(a, b)]))
    print("(c) median %.1f us (min %.1f, max %.1f)" % (med(c), min(c), max(c)))


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "loop":
        loop(int(sys.argv[2]) if len(sys.argv) > 2 else 60)
    elif what == "solo":
        solo(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    else:
        summary(sys.argv[2])
