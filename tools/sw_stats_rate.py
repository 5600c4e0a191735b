"""Throughput of fadehip_sw_stats_batch (parasail's stats mode, `fade stats`'s inverted-repeat search, stats.d:123,164) on
stem-loop-shaped pairs: the query is as[0 .. round(0.75 |as|)], the reference ar = rc(as), |as| up to one 150 bp C2 read.
Reports pairs/s and GCUPS over sum(lq * lr) per call (H2D, host sort and D2H included).  Kernel time alone: run it under
`rocprofv3 --kernel-trace --stats`.
GPU box: python tools/sw_stats_rate.py [--n 1000000] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import fade_amd  # noqa: E402

COMP = np.zeros(256, np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b


def stemloop_batch(rng, n, max_len=150):
    """n stem loops of 20 .. max_len bases (a stem of 30-50 % reverse-complemented with 5 % noise), as concatenated query
    and reference buffers with offsets."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    L = rng.integers(10, max_len // 2 + 1, n) * 2
    stem = (L * rng.uniform(0.3, 0.5, n)).astype(np.int64)
    S = acgt[rng.integers(0, 4, (n, max_len))]
    I = np.arange(max_len)[None, :]
    rows = np.broadcast_to(np.arange(n)[:, None], S.shape)
    m = I < stem[:, None]
    dst = np.clip(L[:, None] - 1 - I, 0, max_len - 1)
    src = S[m]
    noisy = rng.random(len(src)) < 0.05
    val = COMP[src]
    val[noisy] = acgt[rng.integers(0, 4, int(noisy.sum()))]
    S[rows[m], dst[m]] = val
    lq = (3 * L + 2) // 4  # D's round(0.75 * |as|): half away from zero
    q = S[I < lq[:, None]]
    ar = COMP[S[rows, dst]]
    r = ar[I < L[:, None]]
    q_off = np.zeros(n + 1, np.int64)
    r_off = np.zeros(n + 1, np.int64)
    np.cumsum(lq, out=q_off[1:])
    np.cumsum(L, out=r_off[1:])
    return q, q_off, r, r_off, int((lq * L).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    q, qo, r, ro, cells = stemloop_batch(rng, a.n)
    ctx = fade_amd.Context(device=0)
    ctx.sw_stats_batch_packed(q, qo, r, ro)  # warm: buffers and stream
    best = None
    for _ in range(a.reps):
        t = time.perf_counter()
        ctx.sw_stats_batch_packed(q, qo, r, ro)
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    print("%d pairs, %.3e cells: best of %d %.2f ms per call, %.0f pairs/s, %.1f GCUPS (call wall time)" % (
        a.n, cells, a.reps, best * 1e3, a.n / best, cells / best / 1e9), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
