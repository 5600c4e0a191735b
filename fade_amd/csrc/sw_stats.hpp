// sw_stats.hpp — local alignment in parasail's stats mode (fadehip_sw_stats_batch): what
//     Parasail("ACTGN", open, ext, match, mismatch).aligner!("sw", "stats", "striped", "16")
// returns at stats.d:87,123,164 — score, end cell, and matches / similar / length of the path that ends in the best cell.
//
// One wavefront per pair.  Lane k owns R consecutive query rows of a strip of 64 R rows and sweeps the reference one column
// per step, one step behind lane k - 1 (anti-diagonal wavefront): at step t it computes column j = t - k of its rows.  What
// a row below needs from the row above — H and F of column j with the statistics that ride with them — reaches lane k
// from lane k - 1 through one DPP wave shift per value; the row's own left neighbour (H, E of column j - 1) stays in the
// lane's registers.  Queries of up to 512 bases are one strip.  Longer ones (up to FADEHIP_MAX_LONG_QUERY) take strips of
// 512 rows; lane 63 leaves the strip's last row in the wave's scratch row, and lane 0 of the next strip reads it back.
//
// Statistics follow H's chosen predecessor: zero > diagonal > query-only (F) > ref-only (E)
// (FADEHIP_RULE_HDIR_DIAG_F_E; off: E before F), a gap opens only on strict > (FADEHIP_RULE_GAP_TIE_EXTENDS), a cell
// whose H is 0 carries zeros.  matches and similar are both bounded by min(lq, lr) <= 32,768, so they travel as the two
// 16-bit halves of one dword (one add updates both); score and length (lq + lr can reach 65,536) stay int32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fadehip.h"

namespace fadehip {

struct StatsWork {
    uint64_t q_base, r_base;  // byte offsets of the pair's strings in the concatenated buffers
    int32_t lq, lr;
    int32_t idx;              // the pair's index in the caller's order (where its result goes)
    int32_t pad;
};
static_assert(sizeof(StatsWork) == 32, "StatsWork layout");

struct StatsScoring {
    int32_t open, ext, match, mismatch;
    uint32_t rules;
};

constexpr int STATS_WAVES_PER_BLOCK = 4;
constexpr int STATS_STRIP_R = 8;  // rows per lane of the multi-strip kernel: 512-row strips
#define STATS_DPP_WAVE_SHR1 0x138
constexpr int32_t STATS_NEG_INF = -(1 << 29);

// ACTGN + wildcard, case-insensitive (A.1): 0..4, everything else 5
__device__ __forceinline__ int stats_code(uint32_t c) {
    c &= 0xdfu;  // upper-case (other bytes may change but stay outside ACGTN)
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : c == 'N' ? 4 : 5;
}

__device__ __forceinline__ int32_t stats_shr1(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, STATS_DPP_WAVE_SHR1, 0xf, 0xf, true);
}

// The best cell so far in the order of the end-cell rule (A.3): higher score first; ties by smaller ref index, then
// smaller query index (FADEHIP_RULE_END_MIN_REF_THEN_QUERY) or first in row-major order (rule off).
__device__ __forceinline__ bool stats_better(bool min_ref, int s, int i, int j, int bs, int bi, int bj) {
    if (s != bs) return s > bs;
    if (min_ref) return j < bj || (j == bj && i < bi);
    return i < bi || (i == bi && j < bj);
}

// Scratch (multi-strip pairs only): per wave, one row of lr entries of {H, F, H ms, H len, F ms, F len, -, -}.
template <int R>
__global__ __launch_bounds__(64 * STATS_WAVES_PER_BLOCK) void sw_stats_kernel(
        const StatsWork *__restrict__ work, int32_t n_work, const uint8_t *__restrict__ qs, const uint8_t *__restrict__ rs,
        fadehip_sw_stats_result *__restrict__ out, int4 *__restrict__ scratch, int32_t scratch_cols, StatsScoring sc) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * STATS_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * STATS_WAVES_PER_BLOCK;
    const bool f_first = (sc.rules & FADEHIP_RULE_HDIR_DIAG_F_E) != 0;
    const bool tie_ext = (sc.rules & FADEHIP_RULE_GAP_TIE_EXTENDS) != 0;
    const bool eq_char = (sc.rules & FADEHIP_RULE_EQ_BY_CHAR) != 0;
    const bool n_match = (sc.rules & FADEHIP_RULE_N_MATCHES_N) != 0;
    const bool min_ref = (sc.rules & FADEHIP_RULE_END_MIN_REF_THEN_QUERY) != 0;
    int4 *my_scratch = scratch ? scratch + (size_t)wave * (size_t)scratch_cols * 2 : nullptr;

    for (int p = wave; p < n_work; p += n_waves) {
        const StatsWork w = work[p];
        const int lq = w.lq, lr = w.lr;
        int bs = -1, bi = 0, bj = 0;
        uint32_t bms = 0;
        int bl = 0;
        if (lq > 0 && lr > 0) {
            const uint8_t *q = qs + w.q_base;
            const uint8_t *r = rs + w.r_base;
            for (int s0 = 0; s0 < lq; s0 += 64 * R) {
                const int nrow = min(64 * R, lq - s0);
                const int nl = (nrow + R - 1) / R;  // lanes with rows in this strip
                const bool first = s0 == 0, last = s0 + 64 * R >= lq;
                // the lane's rows: code, byte, score of an equal residue (A.1: N vs N per FADEHIP_RULE_N_MATCHES_N)
                int qc[R], qeq[R];
                uint32_t qraw[R];
                int32_t Hl[R], Hl_len[R], E[R], E_len[R];
                uint32_t Hl_ms[R], E_ms[R];
#pragma unroll
                for (int k = 0; k < R; k++) {
                    const int i = s0 + lane * R + k;
                    const uint32_t c = i < lq ? q[i] : 0u;
                    qraw[k] = c;
                    qc[k] = stats_code(c);
                    qeq[k] = qc[k] == 5 ? 0 : (qc[k] == 4 && !n_match) ? sc.mismatch : sc.match;
                    Hl[k] = 0;
                    Hl_ms[k] = 0;
                    Hl_len[k] = 0;
                    E[k] = STATS_NEG_INF;
                    E_ms[k] = 0;
                    E_len[k] = 0;
                }
                // this lane's bottom row at the previous step (what lane + 1 receives), and the diagonal of row 0
                int32_t oH = 0, oF = STATS_NEG_INF, oHl = 0, oFl = 0;
                uint32_t oHms = 0, oFms = 0;
                int32_t dH = 0, dl = 0;
                uint32_t dms = 0;
                const int steps = lr + nl - 1;
                for (int t = 0; t < steps; t++) {
                    int32_t uH = stats_shr1(oH), uF = stats_shr1(oF), uHl = stats_shr1(oHl), uFl = stats_shr1(oFl);
                    uint32_t uHms = (uint32_t)stats_shr1((int32_t)oHms), uFms = (uint32_t)stats_shr1((int32_t)oFms);
                    const int j = t - lane;
                    if (lane == 0) {
                        if (first || j >= lr) {
                            uH = 0; uF = STATS_NEG_INF; uHl = 0; uFl = 0; uHms = 0; uFms = 0;
                        } else {
                            const int4 a = my_scratch[2 * j], b = my_scratch[2 * j + 1];
                            uH = a.x; uF = a.y; uHms = (uint32_t)a.z; uHl = a.w;
                            uFms = (uint32_t)b.x; uFl = b.y;
                        }
                    }
                    if (j == 0) { dH = 0; dms = 0; dl = 0; }
                    if (j >= 0 && j < lr && lane < nl) {
                        const uint32_t rc_raw = r[j];
                        const int rc = stats_code(rc_raw);
                        // row above (H, F of column j) and diagonal (H of column j - 1) of the lane's first row
                        int32_t aH = uH, aF = uF, aHl = uHl, aFl = uFl;
                        uint32_t aHms = uHms, aFms = uFms;
                        int32_t gH = dH, gl = dl;
                        uint32_t gms = dms;
#pragma unroll
                        for (int k = 0; k < R; k++) {
                            const int sub = (rc == 5) ? 0 : (qc[k] == rc) ? qeq[k] : (qc[k] == 5) ? 0 : sc.mismatch;
                            // F: query-only gap from the row above; E: ref-only gap from the left (A.2, A.9)
                            const int32_t F_opn = aH - sc.open, F_ext = aF - sc.ext;
                            const bool f_open = tie_ext ? (F_opn > F_ext) : (F_opn >= F_ext);
                            const int32_t F = f_open ? F_opn : F_ext;
                            const uint32_t F_ms = f_open ? aHms : aFms;
                            const int32_t F_len = (f_open ? aHl : aFl) + 1;
                            const int32_t E_opn = Hl[k] - sc.open, E_ext = E[k] - sc.ext;
                            const bool e_open = tie_ext ? (E_opn > E_ext) : (E_opn >= E_ext);
                            const int32_t Ek = e_open ? E_opn : E_ext;
                            const uint32_t Ek_ms = e_open ? Hl_ms[k] : E_ms[k];
                            const int32_t Ek_len = (e_open ? Hl_len[k] : E_len[k]) + 1;
                            const int32_t D = gH + sub;
                            const uint32_t eq = eq_char ? (qraw[k] == rc_raw) : (sub > 0);
                            const uint32_t D_ms = gms + eq + ((uint32_t)(sub > 0) << 16);
                            const int32_t D_len = gl + 1;
                            const int32_t H = max(max(D, 0), max(Ek, F));
                            // A.8: the chosen predecessor's statistics; H == 0 carries zeros
                            uint32_t H_ms;
                            int32_t H_len;
                            if (H == 0) { H_ms = 0; H_len = 0; }
                            else if (H == D) { H_ms = D_ms; H_len = D_len; }
                            else if (f_first ? (H == F) : (H != Ek)) { H_ms = F_ms; H_len = F_len; }
                            else { H_ms = Ek_ms; H_len = Ek_len; }
                            const int i = s0 + lane * R + k;
                            if (i < lq && stats_better(min_ref, H, i, j, bs, bi, bj)) {
                                bs = H; bi = i; bj = j; bms = H_ms; bl = H_len;
                            }
                            // the old left neighbour is the next row's diagonal
                            gH = Hl[k]; gms = Hl_ms[k]; gl = Hl_len[k];
                            Hl[k] = H; Hl_ms[k] = H_ms; Hl_len[k] = H_len;
                            E[k] = Ek; E_ms[k] = Ek_ms; E_len[k] = Ek_len;
                            aH = H; aF = F; aHms = H_ms; aHl = H_len; aFms = F_ms; aFl = F_len;
                        }
                        oH = aH; oF = aF; oHms = aHms; oHl = aHl; oFms = aFms; oFl = aFl;
                        if (!last && lane == 63) {
                            my_scratch[2 * j] = make_int4(aH, aF, (int32_t)aHms, aHl);
                            my_scratch[2 * j + 1] = make_int4((int32_t)aFms, aFl, 0, 0);
                        }
                    }
                    dH = uH; dms = uHms; dl = uHl;
                }
                // the next strip's lane 0 reads what lane 63 wrote: make the row visible to the whole wave
                if (!last) __threadfence();
            }
        }
        // wave reduction of the best cell under the end-cell order
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int os = __shfl_xor(bs, m, 64), oi = __shfl_xor(bi, m, 64), oj = __shfl_xor(bj, m, 64);
            const uint32_t oms = (uint32_t)__shfl_xor((int)bms, m, 64);
            const int ol = __shfl_xor(bl, m, 64);
            if (stats_better(min_ref, os, oi, oj, bs, bi, bj)) {
                bs = os; bi = oi; bj = oj; bms = oms; bl = ol;
            }
        }
        if (lane == 0) {
            fadehip_sw_stats_result res;
            if (bs < 0) {  // an empty query or reference: nothing aligned, all zeros
                res.score = res.end_query = res.end_ref = res.matches = res.similar = res.length = 0;
            } else {
                res.score = bs;
                res.end_query = bi;
                res.end_ref = bj;
                res.matches = (int32_t)(bms & 0xffffu);
                res.similar = (int32_t)(bms >> 16);
                res.length = bl;
            }
            out[w.idx] = res;
        }
    }
}

}  // namespace fadehip
