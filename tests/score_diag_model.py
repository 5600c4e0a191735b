"""A numpy model of the eight-lane score pass in its row-and-step drift frame (sw_pk_kernel<R, 1, false, 8, false, 0, true, true>),
beside score_frame_model.score_pass (the column-drift frame and the unframed recurrence).  Not a test module:
tests/test_score_diag_model.py and tests/test_gpu_score_diag.py import it.

Every value of lane-local row r at sweep step t carries the wave-uniform drift D(r, t) = 8 ext (t + r + C0):
  Hl, hu, hd, hu_prev = H + D            Eh, fu = E-hat + D - 8 ext, F-hat + D - 8 ext
  Dp = hd + 8 (W' + ext)                 (D(r, t) - D(r - 1, t - 1) = 2 * 8 ext, and T is kept at D - 8 ext)
  En = max3(hl, Eh, floorE)              floorE = D(r, t) + 8 open - 8 ext: the zero floor of local alignment
  Fn = max(hu, fu)                       (D(r, t) - 8 ext = D(r - 1, t): the decay down a column is the frame's own)
  T  = max3(Dp, En, Fn)                  H = T - (8 open - 8 ext)
  k  = 8 H + C_parity(t)                 = the true pair key + 128 ext (r >> 1), taken off GH after the sweep
hu and fu that arrive from the lane to the left lose (R - 1) 8 ext; the first lane of a group takes hu = D(0, t) - 8 ext and fu = 0;
fu of row R - 1 starts at (R - 1) 8 ext, which is F-hat = 0 there.
As in score_frame_model one alignment is one 16-bit half, every packed operation wraps or saturates as its instruction does, and
`peak` is the largest operand v_pk_maximum3_f16 was ever given, which must stay below 0x7c00.
"""
import numpy as np

from score_frame_model import F16_INF, KW, LG, PAD, SCALE, U16, _classes, host_steps  # noqa: F401

C0 = 2   # keeps every stored H, E and table operand non-negative (hu_prev starts at D(0, -1) - 8 ext = 0)


def diag_fits(match, open_, ext, rows, steps, lg=LG):
    """fadehip_kernels.hpp diag_fits, term for term: the largest max3 operand (the score of `rows` rows, D(R - 1, steps), the
    hat offset, one table entry), the largest offset key, the table byte, and open >= ext >= 0."""
    R = rows // lg
    return (match >= 0 and ext >= 0 and open_ >= ext and steps >= 0 and
            8 * match * rows + 8 * ext * (steps + R - 1 + C0) + 8 * open_ + 8 * (15 + ext) < F16_INF and
            64 * match * rows + 63 + 128 * ext * (R - 1) // 2 < F16_INF and
            8 * (15 + ext) <= 255)


def longest_diag_window(match, open_, ext, rows):
    """The longest window (columns) whose launch the host still sweeps in this frame."""
    lr = 0
    while lr < 4096 and diag_fits(match, open_, ext, rows, host_steps(lr + 1)):
        lr += 1
    return lr


def score_pass_diag(pairs, R, match=2, mismatch=-3, open_=10, ext=2):
    """pairs: [(query, window)] of A/C/G/T strings, len(query) <= 8 R.  Returns (results, peak) as score_frame_model.score_pass."""
    n = len(pairs)
    rows = LG * R
    lq = np.array([len(q) for q, _ in pairs])
    lr = np.array([len(r) for _, r in pairs])
    assert lq.max() <= rows
    steps = 4 * ((int(lr.max()) + LG - 1 + 3) // 4)
    qc = np.full((n, rows), 255, dtype=np.uint8)
    rc = np.full((n, steps + LG), 254, dtype=np.uint8)
    for i, (q, r) in enumerate(pairs):
        qc[i, :len(q)] = _classes(q)
        rc[i, LG:LG + len(r)] = _classes(r)
    qc = qc.reshape(n, LG, R)
    ext8, open8 = ext * SCALE, open_ * SCALE
    oe8 = U16(open8 - ext8)
    wm, wx = U16((match + open_ + ext) * SCALE), U16((mismatch + open_ + ext) * SCALE)   # real classes: 8 (W' + ext)
    assert wm <= 255 and wx <= 255, "a table entry is a byte"
    hand = U16((R - 1) * ext8)
    lig = np.arange(LG)
    peak = [0]

    def D(r, t):
        return ext8 * (t + r + C0)

    def max3(a, b, c):
        peak[0] = max(peak[0], int(np.max(a)), int(np.max(b)), int(np.max(c)))
        return np.maximum(np.maximum(a, b), c).astype(U16)

    def smax(a, b):  # v_pk_max_i16
        return np.maximum(a.view(np.int16), b.view(np.int16)).view(U16)

    def full(v):
        return np.full((n, LG), v & 0xffff, dtype=U16)

    zero = full(0)
    Hl = [full(D(r, -1)) for r in range(R)]
    hu_out, hu_prev = full(D(R - 1, -1)), full(D(0, -1) - ext8)
    Eh = [zero.copy() for _ in range(R)]
    # F-hat = 0 in row R - 1.  hu_out and fu_out never fall below `hand` (asserted per step), so the device's 32-bit subtraction
    # of both halves at once, folded into the DPP move of the hand-off, borrows nothing from the upper half
    fu_out = full(hand)
    NK = (R + 1) // 2
    key = [zero.copy() for _ in range(NK)]
    GH = [zero.copy() for _ in range(NK)]
    GT = [zero.copy() for _ in range(NK)]
    with np.errstate(over="ignore"):
        for t in range(steps):
            col = rc[:, LG + t - lig]
            assert (hu_out >= hand).all() and (fu_out >= hand).all()
            hu = (np.roll(hu_out, 1, axis=1) - hand).astype(U16)
            fu = (np.roll(fu_out, 1, axis=1) - hand).astype(U16)
            hu[:, 0] = U16(D(0, t) - ext8)
            fu[:, 0] = 0
            tk = KW - 1 - (t & (KW - 1))
            c_even = U16((2 * tk + 1 - 8 * ext8 * (t + C0)) & 0xffff)
            c_odd = U16((2 * tk - 8 * ext8 * (t + C0 + 1)) & 0xffff)
            hd = hu_prev
            hu_prev = hu
            kprev = None
            for r in range(R):
                q = qc[:, :, r]
                w = np.where((q > 3) | (col > 3), U16(0), np.where(q == col, wm, wx)).astype(U16)
                Dp = (hd + w).astype(U16)
                hl = Hl[r]
                En = max3(hl, Eh[r], U16(D(r, t)) + oe8)
                Fn = smax(hu, fu)
                T = max3(Dp, En, Fn)
                H = (T - oe8).astype(U16)
                k = (H * U16(8) + (c_odd if r & 1 else c_even)).astype(U16)
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
                wbase = U16((t // KW) * (2 * KW) + (2 * KW - 1))
                for p in range(NK):
                    wk = key[p]
                    wH = wk & U16(0xffc0)
                    better = wH > GH[p]
                    GT[p] = np.where(better, wbase - (wk & U16(63)), GT[p]).astype(U16)
                    GH[p] = np.maximum(GH[p], wH)
                    key[p] = zero.copy()
        for p in range(NK):   # the offset comes off once per pair (every fold saw 8 H + 128 ext p >= 128 ext p)
            GH[p] = (GH[p] - U16(128 * ext * p)).astype(U16)
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
