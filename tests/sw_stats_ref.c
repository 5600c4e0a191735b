/*
 * sw_stats_ref.c — scalar full-matrix restatement of parasail's local alignment in stats mode, the call of
 * stats.d:87,123,164 (Parasail("ACTGN", 3, 8, 10, -5).aligner!("sw","stats","striped","16")), as DESIGN.md Appendix A
 * states it (A.1-A.4 for score and end cell, as oracle/sw_scalar.c; A.8-A.11 for the statistics).  Test code only:
 * tests/sw_stats_ref.py builds it into a temporary directory.
 *
 * H, E (ref-only gap, from the left) and F (query-only gap, from above) each carry {matches, similar, length} of the
 * path that reaches them.  H takes its chosen predecessor's: zero > diagonal > F > E (rule HDIR_DIAG_F_E; off: E
 * before F); a gap opens on strict > (GAP_TIE_EXTENDS; off: >=); a diagonal step adds 1 to length, 1 to similar when
 * the substitution score is > 0, 1 to matches when the residues are equal (EQ_BY_CHAR; off: when the score is > 0);
 * a gap step adds 1 to length; H == 0 carries zeros.
 */
#include <ctype.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum {
    R_END_MIN_REF = 1 << 0, R_HDIR_DIAG_F_E = 1 << 1, R_GAP_TIE_EXTENDS = 1 << 2, R_EQ_BY_CHAR = 1 << 3,
    R_N_MATCHES_N = 1 << 6
};
#define NEG_INF (INT_MIN / 4)

typedef struct { int32_t score, end_query, end_ref, matches, similar, length; } stats_res;
typedef struct { int h, m, s, l; } cell;

static int code_of(unsigned char c) {
    switch (toupper(c)) {
    case 'A': return 0;
    case 'C': return 1;
    case 'T': return 2;
    case 'G': return 3;
    case 'N': return 4;
    default: return 5; /* wildcard: scores 0 against everything */
    }
}

static int sub_score(int a, int b, int match, int mismatch, unsigned rules) {
    if (a == 5 || b == 5) return 0;
    if (a != b) return mismatch;
    if (a == 4 && !(rules & R_N_MATCHES_N)) return mismatch;
    return match;
}

int stats_ref(const int32_t sc[4], unsigned rules, const char *q, int lq, const char *r, int lr, stats_res *out) {
    const int open = sc[0], ext = sc[1], match = sc[2], mismatch = sc[3];
    memset(out, 0, sizeof *out);
    if (lq <= 0 || lr <= 0) return 0;
    cell *Hup = (cell *)calloc((size_t)lr + 1, sizeof(cell)); /* H[i-1][j-1] at index j */
    cell *Hcur = (cell *)calloc((size_t)lr + 1, sizeof(cell));
    cell *Fup = (cell *)malloc(((size_t)lr + 1) * sizeof(cell));
    if (!Hup || !Hcur || !Fup) { free(Hup); free(Hcur); free(Fup); return -1; }
    for (int j = 0; j <= lr; j++) { Fup[j].h = NEG_INF; Fup[j].m = Fup[j].s = Fup[j].l = 0; }
    int best = -1, bi = 0, bj = 0;
    cell bc = {0, 0, 0, 0};
    for (int i = 0; i < lq; i++) {
        const int qa = code_of((unsigned char)q[i]);
        cell E = {NEG_INF, 0, 0, 0};
        Hcur[0].h = Hcur[0].m = Hcur[0].s = Hcur[0].l = 0; /* H[i][-1] */
        for (int j = 0; j < lr; j++) {
            const cell up = Hup[j + 1], diag = Hup[j], left = Hcur[j];
            /* F: from above */
            const int f_opn = up.h - open, f_ext = Fup[j + 1].h - ext;
            const int f_open = (rules & R_GAP_TIE_EXTENDS) ? f_opn > f_ext : f_opn >= f_ext;
            cell F = f_open ? up : Fup[j + 1];
            F.h = f_open ? f_opn : f_ext;
            F.l += 1;
            /* E: from the left */
            const int e_opn = left.h - open, e_ext = E.h - ext;
            const int e_open = (rules & R_GAP_TIE_EXTENDS) ? e_opn > e_ext : e_opn >= e_ext;
            cell nE = e_open ? left : E;
            nE.h = e_open ? e_opn : e_ext;
            nE.l += 1;
            E = nE;
            /* D: diagonal */
            const int s = sub_score(qa, code_of((unsigned char)r[j]), match, mismatch, rules);
            cell D = diag;
            D.h = diag.h + s;
            D.m += (rules & R_EQ_BY_CHAR) ? (q[i] == r[j]) : (s > 0);
            D.s += s > 0;
            D.l += 1;
            int h = D.h;
            if (E.h > h) h = E.h;
            if (F.h > h) h = F.h;
            if (h < 0) h = 0;
            cell H;
            if (h == 0) { H.m = H.s = H.l = 0; }
            else if (h == D.h) H = D;
            else if (rules & R_HDIR_DIAG_F_E) H = (h == F.h) ? F : E;
            else H = (h == E.h) ? E : F;
            H.h = h;
            if (h > best) { best = h; bi = i; bj = j; bc = H; }
            else if (h == best && (rules & R_END_MIN_REF) && j < bj) { bi = i; bj = j; bc = H; }
            Hcur[j + 1] = H;
            Fup[j + 1] = F;
        }
        cell *t = Hup; Hup = Hcur; Hcur = t;
    }
    out->score = best < 0 ? 0 : best;
    out->end_query = bi;
    out->end_ref = bj;
    out->matches = bc.m;
    out->similar = bc.s;
    out->length = bc.l;
    free(Hup); free(Hcur); free(Fup);
    return 0;
}

/* n pairs over concatenated strings with n + 1 offsets each (the layout of fadehip_sw_stats_batch) */
int stats_ref_batch(const int32_t sc[4], unsigned rules, int n, const char *q, const int64_t *q_off, const char *r,
                    const int64_t *r_off, stats_res *out) {
    for (int k = 0; k < n; k++)
        if (stats_ref(sc, rules, q + q_off[k], (int)(q_off[k + 1] - q_off[k]), r + r_off[k], (int)(r_off[k + 1] - r_off[k]),
                      out + k))
            return -1;
    return 0;
}
