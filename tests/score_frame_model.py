"""A numpy model of the eight-lane score pass (sw_pk_kernel<R, 1, false, 8>) as the device computes it: 16-bit halves, the
hat domain at scale 8, the pair key that wraps mod 2^16, the 32-step key windows and their folds, the per-lane pick and the
butterfly over the group's lanes.  frame=True is the column-drift frame (sw_pk_kernel<..., FRAME>), frame=False the
recurrence it replaces.  Not a test module: tests/test_score_frame_model.py and tests/test_gpu_score_frame.py import it.

One alignment is one 16-bit half of the device's registers, so the model carries uint16 arrays of shape (alignments, 8 lanes)
and does every packed operation on them with the wrap or the saturation the instruction has.  v_pk_maximum3_f16 orders its
operands as integers only while they are non-negative and below the f16 infinity: the model takes the integer maximum and
records the largest operand it was ever given (`peak`), which the caller holds against 0x7c00.
"""
import numpy as np

LG = 8
SCALE = 8
KW = 32
PAD = 7          # class of a pad row / pad column: W' = 0
F16_INF = 0x7c00
U16 = np.uint16


def frame_fits(match, open_, ext, rows, steps, lg=LG):
    """fadehip_kernels.hpp frame_fits: the launch's largest framed value stays below the f16 infinity."""
    return (match >= 0 and ext >= 0 and open_ >= ext and steps >= 0 and
            8 * match * rows + 8 * ext * (steps + lg + 1) + 8 * open_ + 8 * 15 < F16_INF)


def host_steps(max_lr):
    """Sweep steps the host plans for a class list whose longest window has max_lr columns (plan_two_pass: n_blocks1 * 4)."""
    return 4 * ((max_lr + 15 + 3) // 4)


def longest_framed_window(match, open_, ext, rows):
    """The longest window (columns) whose launch the host still frames."""
    lr = 1
    while frame_fits(match, open_, ext, rows, host_steps(lr + 1)):
        lr += 1
    return lr if frame_fits(match, open_, ext, rows, host_steps(lr)) else 0


_CLASS = np.full(256, PAD, dtype=np.uint8)
_CLASS[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)


def _classes(seq):
    c = _CLASS[np.frombuffer(seq.encode() if isinstance(seq, str) else seq, dtype=np.uint8)]
    assert (c < 4).all(), "the model takes A, C, G, T only"
    return c


def score_pass(pairs, R, match=2, mismatch=-3, open_=10, ext=2, frame=True):
    """pairs: [(query, window)] of A/C/G/T strings, len(query) <= 8 R.  Returns (results, peak): results[i] =
    (score, end_query, end_ref) with (0, 0, 0) where nothing scores, as the device's Fwd; peak = the largest max3 operand."""
    n = len(pairs)
    rows = LG * R
    lq = np.array([len(q) for q, _ in pairs])
    lr = np.array([len(r) for _, r in pairs])
    assert lq.max() <= rows
    steps = 4 * ((int(lr.max()) + LG - 1 + 3) // 4)      # the wave sweeps whole blocks of four steps
    qc = np.full((n, rows), 255, dtype=np.uint8)
    rc = np.full((n, steps + LG), 254, dtype=np.uint8)     # columns -lig .. and past the window are pads
    for i, (q, r) in enumerate(pairs):
        qc[i, :len(q)] = _classes(q)
        rc[i, LG:LG + len(r)] = _classes(r)
    qc = qc.reshape(n, LG, R)
    ext8, open8 = U16(ext * SCALE), U16(open_ * SCALE)
    oe8, ext64 = U16(open8 - ext8), U16((ext * SCALE * 8) & 0xffff)
    wm, wx = U16((match + open_) * SCALE), U16((mismatch + open_) * SCALE)
    lig = np.arange(LG)
    peak = [0]

    def max3(a, b, c):
        peak[0] = max(peak[0], int(a.max()), int(b.max()), int(c.max()))
        return np.maximum(np.maximum(a, b), c)

    def smax(a, b):  # v_pk_max_i16
        return np.maximum(a.view(np.int16), b.view(np.int16)).view(U16)

    zero = np.zeros((n, LG), dtype=U16)
    if frame:
        fl_h = np.broadcast_to((ext8 * (LG - 1 - lig)).astype(U16), (n, LG)).copy()
        fl_e = fl_h + oe8
        kd8 = (fl_h * U16(8)).astype(U16)
        Hl = [fl_h.copy() for _ in range(R)]
        hu_out, hu_prev = fl_h.copy(), fl_h.copy()
    else:
        Hl = [zero.copy() for _ in range(R)]
        hu_out, hu_prev = zero.copy(), zero.copy()
    Eh = [zero.copy() for _ in range(R)]
    fu_out = zero.copy()
    NK = (R + 1) // 2
    key = [zero.copy() for _ in range(NK)]
    GH = [zero.copy() for _ in range(NK)]
    GT = [zero.copy() for _ in range(NK)]
    with np.errstate(over="ignore"):
        for t in range(steps):
            col = rc[:, LG + t - lig]                                     # (n, LG): the class of column t - lig
            if frame:
                fl_h = fl_h + ext8
                fl_e = fl_e + ext8
                kd8 = kd8 + ext64
            hu = np.roll(hu_out, 1, axis=1)
            fu = np.roll(fu_out, 1, axis=1)
            hu[:, 0] = fl_h[:, 0] if frame else 0
            fu[:, 0] = 0
            tk = U16(KW - 1 - (t & (KW - 1)))
            tk_even, tk_odd = U16(2 * tk + 1), U16(2 * tk)
            if frame:
                tkf_even, tkf_odd = (tk_even - kd8).astype(U16), (tk_odd - kd8).astype(U16)
            hd = hu_prev
            hu_prev = hu
            kprev = None
            for r in range(R):
                q = qc[:, :, r]
                w = np.where((q > 3) | (col > 3), U16(0), np.where(q == col, wm, wx)).astype(U16)
                Dp = hd + w
                hl = Hl[r]
                if frame:
                    En = max3(hl, Eh[r], fl_e)
                    Fn = smax(hu, fu) - ext8
                    T = max3(Dp, En, Fn)
                    H = T - oe8
                    k = (H * U16(8) + (tkf_odd if r & 1 else tkf_even)).astype(U16)
                else:
                    En = smax(hl, Eh[r] - ext8)
                    Fn = smax(hu, fu - ext8)
                    T = max3(Dp, En, Fn)
                    H = np.where(T > open8, T - open8, U16(0)).astype(U16)   # v_pk_sub_u16 clamp
                    k = (H * U16(8) + (tk_odd if r & 1 else tk_even)).astype(U16)
                if r & 1:
                    key[r >> 1] = max3(key[r >> 1], kprev, k)
                elif (R & 1) and r == R - 1:
                    key[r >> 1] = max3(key[r >> 1], k, k)
                else:
                    kprev = k
                hd = hl
                Hl[r] = H
                Eh[r] = En
                hu = H
                fu = Fn
            hu_out, fu_out = hu, fu
            if (t & (KW - 1)) == KW - 1 or t == steps - 1:
                # fold the window's keys into (GH, GT): a later window wins only with a strictly larger H
                wbase = U16((t // KW) * (2 * KW) + (2 * KW - 1))
                for p in range(NK):
                    wk = key[p]
                    wH = wk & U16(0xffc0)
                    better = wH > GH[p]
                    GT[p] = np.where(better, wbase - (wk & U16(63)), GT[p]).astype(U16)
                    GH[p] = np.maximum(GH[p], wH)
                    key[p] = zero.copy()
    # per-lane pick (an earlier pair wins a tie), then the group's maximum of (H, -column, -row)
    best = np.zeros((n, LG), dtype=np.int64)
    bk = np.zeros((n, LG), dtype=np.int64)
    for p in range(NK):
        h8 = (GH[p] >> 6).astype(np.int64) << 3
        gt = GT[p].astype(np.int64)
        tt, row = gt >> 1, lig * R + 2 * p + (gt & 1)
        k32 = np.where(h8 > 0, (h8 << 16) | (0xffff - tt), 0)
        take = (row < lq[:, None]) & (k32 > bk)
        cand = (k32 >> 16 << 32) | (((k32 + lig) & 0xffff) << 16) | (0xffff - row)
        best = np.where(take, cand, best)
        bk = np.where(take, k32, bk)
    best = np.where(bk >> 16 > 0, best, 0).max(axis=1)
    out = []
    for c in best:
        c = int(c)
        out.append(((c >> 32) // SCALE, 0xffff - (c & 0xffff), 0xffff - ((c >> 16) & 0xffff)) if c else (0, 0, 0))
    return out, peak[0]
