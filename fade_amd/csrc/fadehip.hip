// fadehip.hip — the alignment engine of the C ABI (include/fadehip.h) over the gfx950 kernels in fadehip_kernels.hpp and
// sw_stats.hpp.  (The context, its memory and the error channel: fadehip_ctx.hip; BGZF: fadehip_bgzf.hip; BAM records and the
// file path: fadehip_bam.hip.)
// Host side of the drop-in boundary for source/anno.d:44-50 / source/analysis.d:67.
// No CPU fallback lives here: every entry point either runs the HIP path or returns an error.
//
// Level 2 is an asynchronous pipeline: upload is one hipMemcpyAsync of a pinned batch block, run
// enqueues every kernel and the D2H of the results without reading anything back — launches are sized from host-side
// bounds, the real counts stay on the device, persistent waves draw the traced re-computation's work from a table a
// planning kernel builds — and results / collect waits for the slot.
#include "fadehip_host.hpp"
#include "fadehip_kernels.hpp"
#include "sw_stats.hpp"
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace fadehip;
using namespace fadehip::host;

namespace {

// Growing a scratch buffer while a run is being enqueued: kernels already queued may still use the old allocation, so it
// is only parked here and freed once the slot has been waited for (hipFree would also stall every other stream).
int reserve_run(fadehip_ctx *ctx, std::vector<void *> &trash, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return 0;
    if (b.p) trash.push_back(b.p);
    b.p = nullptr;
    b.cap = 0;
    size_t want = std::max<size_t>(bytes + bytes / 8, 256);  // (headroom: a stream's batches differ a little in size)
    want = (want + 255) & ~(size_t)255;
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

}  // namespace

namespace fadehip::host {

int build_score_tab(fadehip_ctx *ctx, const fadehip_params &p, ScoreTab &sc) {
    if (p.open <= 0 || p.ext <= 0 || p.ext > p.open)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "gap penalties must satisfy 0 < ext <= open (got open=%d ext=%d)", p.open, p.ext);
    const int lo = std::min(std::min(p.match, p.mismatch), 0) + p.open;
    const int hi = std::max(std::max(p.match, p.mismatch), 0) + p.open;
    if (lo < 0 || hi > 15)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED,
                       "scores + open must fit 4 bits for the profile registers (match=%d mismatch=%d open=%d)",
                       p.match, p.mismatch, p.open);
    for (int cq = 0; cq < 8; cq++) {
        uint32_t v = 0;
        for (int cr = 0; cr < 8; cr++) {
            int w;
            if (cq >= PAD_CLASS || cr >= PAD_CLASS) w = -p.open;  // pad row/column: W' = 0
            else if (cq == 5 || cr == 5) w = 0;                   // parasail wildcard
            else if (cq == 4 && cr == 4) w = (p.rules & FADEHIP_RULE_N_MATCHES_N) ? p.match : p.mismatch;  // Appendix A.1
            else w = (cq == cr) ? p.match : p.mismatch;
            v |= (uint32_t)(w + p.open) << (4 * cr);
        }
        sc.prof[cq] = v;
    }
    sc.open = p.open;
    sc.ext = p.ext;
    sc.match = p.match;
    sc.mismatch = p.mismatch;
    sc.rules = p.rules;
    return 0;
}

}  // namespace fadehip::host

namespace {

void fill_ascii_table(uint8_t t[256]) {
    memset(t, 0, 256);
    const char *s = "=ACMGRSVTWYHKDBN";
    for (int k = 1; k < 16; k++) {
        t[(unsigned char)s[k]] = (uint8_t)k;
        t[(unsigned char)(s[k] | 0x20)] = (uint8_t)k;  // analysis.d:63 upper-cases the window
    }
}

}  // namespace

namespace fadehip::host {

// c_ascii_code filled, and waited for, on the context's first stream (fadehip_create).  Without relocatable device code
// every unit that sees fadehip_kernels.hpp would hold a copy of the table of its own: this unit alone includes the header,
// so the copy filled here is the one pack_ascii_kernel reads.
hipError_t upload_ascii_code(hipStream_t st) {
    uint8_t table[256];
    fill_ascii_table(table);
    const hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_ascii_code), table, 256, 0, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

}  // namespace fadehip::host

namespace {

int new_event(fadehip_ctx *ctx, Slot &s, int *idx) {
    if (s.ev_used == (int)s.ev.size()) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreate(&e));
        s.ev.push_back(e);
    }
    *idx = s.ev_used++;
    return 0;
}

int record(fadehip_ctx *ctx, Slot &s, int *idx, hipStream_t on = nullptr) {
    int rc = new_event(ctx, s, idx);
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(s.ev[*idx], on ? on : s.stream));
    return 0;
}

// The wave kernel of a row class.  mode 0: single pass with full trace (FADEHIP_KERNEL=pk), 1: score pass, 2: traced
// re-computation (default rules), 3: traced re-computation with rule switches; SW_INT32: the int32 single-pass kernel
// (FADEHIP_KERNEL=int32).  longw: windows beyond one staged chunk (CH_COLS columns) in this launch (packed kernels only).
constexpr int SW_INT32 = -1;
template <int C = 0>
const void *sw_kernel(int cls, int mode, bool longw) {
    if constexpr (C >= NUM_CLASSES) {
        return nullptr;
    } else {
        if (cls != C) return sw_kernel<C + 1>(cls, mode, longw);
        constexpr int R = class_rows(C);
        switch (mode) {
        case SW_INT32: return (const void *)sw_forward_kernel<R>;
        case 0: return longw ? (const void *)sw_pk_kernel<R, 0, true> : (const void *)sw_pk_kernel<R, 0>;
        case 1: return longw ? (const void *)sw_pk_kernel<R, 1, true> : (const void *)sw_pk_kernel<R, 1>;
        case 2: return longw ? (const void *)sw_pk_kernel<R, 2, true> : (const void *)sw_pk_kernel<R, 2>;
        default: return longw ? (const void *)sw_pk_kernel<R, 3, true> : (const void *)sw_pk_kernel<R, 3>;
        }
    }
}

// The long list's wave kernel (one alignment per wavefront) at R rows per lane: run_long_wave picks R.
const void *sw64_kernel(int R) {
    switch (R) {
    case 12: return (const void *)sw_forward64_kernel<12>;
    case 16: return (const void *)sw_forward64_kernel<16>;
    case 24: return (const void *)sw_forward64_kernel<24>;
    case 32: return (const void *)sw_forward64_kernel<32>;
    case 48: return (const void *)sw_forward64_kernel<48>;
    default: return (const void *)sw_forward64_kernel<64>;
    }
}

// The score pass on eight-lane groups, or nullptr where the class keeps its sixteen-lane kernel.  A lane owns R8 rows, a
// group 8 R8: rows come in steps of 8 instead of 16 (36-base reads: 40 rows instead of 64; 50: 56 / 64; 76: 80 / 96; 100, 101:
// 104 / 128; 150, 151: 152 / 160), sixteen alignments per wavefront, a skew of 7 steps.  Taken for the batch's top class
// (a class below it holds reads of any length up to its rows) when every read of the batch fits the rows — the batch's
// longest read is known on the host — and they are fewer than the sixteen-lane class's.  No snapshots in this geometry
// (pass 2 re-computes from step 0): the caller asks only for launches that leave none.
// The kernel sweeps in the column-drift frame (sw_pk_kernel<..., FRAME>: one packed instruction less per cell) when the
// context asks for it and the launch's `steps` sweep steps keep every framed value below the f16 infinity (frame_fits, from
// the scoring and the kernel's rows).  Three tiers: the frame whose drift follows the row as well (sw_pk_kernel<..., FRAME, DIAG>:
// one more instruction less per cell; FADEHIP_SCORE_DIAG=0 turns only this one off) where its own bound holds (diag_fits), else the
// column-drift frame, else the unframed kernel.  *framed: 0 unframed, 1 column drift, 2 row and step drift.
template <int R8>
const void *g8_pick(const fadehip_ctx *ctx, int steps, int *framed) {
    const ScoreTab &sc = ctx->sc;
    const int match = std::max(std::max(sc.match, sc.mismatch), 0);
    *framed = !ctx->score_frame ? 0 : ctx->score_diag && diag_fits(match, sc.open, sc.ext, 8 * R8, steps) ? 2 : frame_fits(match, sc.open, sc.ext, 8 * R8, steps) ? 1 : 0;
    return *framed == 2 ? (const void *)sw_pk_kernel<R8, 1, false, 8, false, 0, true, true>
           : *framed ? (const void *)sw_pk_kernel<R8, 1, false, 8, false, 0, true> : (const void *)sw_pk_kernel<R8, 1, false, 8>;
}
const void *g8_kernel(const fadehip_ctx *ctx, int cls, int max_lq, int steps, int *framed) {
    const int score_g8 = ctx->score_g8, rows16 = 16 * class_rows(cls);
    *framed = 0;
    if (!score_g8 || max_lq > rows16) return nullptr;
    if (max_lq <= 40 && rows16 > 40) return g8_pick<5>(ctx, steps, framed);
    if (max_lq <= 56 && rows16 > 56) return g8_pick<7>(ctx, steps, framed);
    if (max_lq <= 80 && rows16 > 80) return g8_pick<10>(ctx, steps, framed);
    if (max_lq <= 104 && rows16 > 104) return g8_pick<13>(ctx, steps, framed);
    if (max_lq <= 152 && rows16 > 152 && rows16 <= 160)
        return score_g8 == 2 ? (const void *)sw_pk_kernel<19, 1, false, 8, false, 2> : g8_pick<19>(ctx, steps, framed);
    return nullptr;
}

// every alignment kernel takes one SwArgs by value and runs in blocks of one wavefront
int launch_sw(fadehip_ctx *ctx, const void *fn, int grid, size_t lds, hipStream_t st, SwArgs a) {
    void *args[] = {&a};
    HIPCHK(ctx, hipLaunchKernel(fn, dim3((unsigned)grid), dim3(64), args, lds, st));
    return 0;
}

// waves of a pass-2 kernel the device holds at once: the size of its persistent launch
int resident_waves(fadehip_ctx *ctx, int cls, int mode, size_t lds, bool longw) {
    const uint64_t key = ((uint64_t)cls << 40) | ((uint64_t)mode << 32) | ((uint64_t)longw << 36) | (uint64_t)lds;
    std::lock_guard<std::mutex> l(ctx->resident_mu);
    auto it = ctx->resident.find(key);
    if (it != ctx->resident.end()) return it->second;
    int per_cu = 0;
    const void *fn = sw_kernel(cls, mode, longw);
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, lds) != hipSuccess || per_cu <= 0) per_cu = 4;
    const int w = per_cu * std::max(ctx->cu_count, 1);
    ctx->resident[key] = w;
    return w;
}

// One list of a run, as the class runners see it.  The defaults are level 1's (no gate, no per-read status, untimed).
struct ClassRun {
    int cls = 0;
    const Work *work = nullptr;
    const Meta *meta = nullptr;
    int n_bound = 0;                      // items on the list, at most
    const uint32_t *count_dev = nullptr;  // where the device keeps the real count
    int max_lr = 0;                       // longest window, at most
    const uint8_t *q_nib = nullptr, *r_nib = nullptr;
    fadehip_aln *out = nullptr;
    uint8_t *rs = nullptr;
    int floor_len = 0, gate = 0;
    int64_t budget = 0;
    bool timed = false;
};

// The score arguments every wave kernel's launch shares, for items [i0, i0 + n) of the list.
SwArgs sw_args(const fadehip_ctx *ctx, const Slot &s, const ClassRun &c, int64_t i0, int n) {
    SwArgs a;
    memset(&a, 0, sizeof a);
    a.work = c.work + i0;
    a.n_items = n;
    a.q_nib = c.q_nib;
    a.r_nib = c.r_nib;
    a.fwd = (Fwd *)s.fwd.p + i0;
    a.sc = ctx->sc;
    return a;
}

// The common traceback for items [i0, i0 + n) of the list.  t holds what differs between the forward kernels (R, packed,
// the trace and its stride, and count_dev / item_base where n is a bound); everything else is filled in here.
int launch_traceback(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c, int64_t i0, int n, TbArgs t) {
    t.work = c.work + i0;
    t.meta = c.meta ? c.meta + i0 : nullptr;
    t.fwd = (Fwd *)s.fwd.p + i0;
    t.n_items = n;
    t.q_nib = c.q_nib;
    t.r_nib = c.r_nib;
    t.sc = ctx->sc;
    t.out = c.out;
    t.rs = c.rs;
    t.stats = (c.rs && c.gate) ? s.d_stats() : nullptr;
    t.floor_len = c.floor_len;
    t.gate = c.gate;
    t.early_out = 0;
    hipLaunchKernelGGL(traceback_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// The three timing events of one chunk of a timed run: 0 before the forward launch, 1 between it and the traceback, 2
// behind the traceback, which also files the chunk's two spans.  An untimed run records nothing.
struct ChunkSpans {
    bool timed;
    int e[3] = {-1, -1, -1};
    int mark(fadehip_ctx *ctx, Slot &s, int k, hipStream_t on) {
        if (!timed) return 0;
        const int rc = record(ctx, s, &e[k], on);
        if (rc || k < 2) return rc;
        s.fwd_spans.push_back({e[0], e[1]});
        s.tb_spans.push_back({e[1], e[2]});
        return 0;
    }
};

// Sizes of the two-pass path for one class list: launch geometry and scratch.  Computed for every class of a run before
// its first launch, so that the slot's scratch buffers are sized ONCE per run (to the maximum over the classes) and
// nothing is re-allocated between kernels that are already queued.
struct TwoPassPlan {
    int n_ck = 0;
    uint64_t ck_stride = 0;
    int n_blocks1 = 0, ref_stride1 = 0;
    size_t lds1 = 0;
    int mode2 = 2;
    bool longw = false;  // some window of the launch may be longer than one staged chunk
    int64_t chunk_oct = 1;
    int total_oct = 0;
    uint64_t wave_stride = 0;
    int p2_waves = 1;
    size_t ckpt_bytes = 0, fwd_bytes = 0, trace_bytes = 0, cand_bytes = 0;
};

int plan_two_pass(fadehip_ctx *ctx, const Slot &s, const ClassRun &c, TwoPassPlan &p) {
    const int cls = c.cls, R = class_rows(cls), max_lr = c.max_lr, n_items = c.n_bound;
    // Wave snapshots (every CK_COLS steps, so that pass 2 can resume a sweep instead of repeating it) are only worth
    // their stores — four times the algorithmic bytes of the score pass at C2, twelve times at C3 — when pass 2 has many
    // candidates.  The forced-diagonal shortcut leaves it a few hundred per million reads, so a run leaves snapshots
    // only if the slot's previous run sent more than 1/32 of its alignments to pass 2; without them a candidate is
    // traced from step 0 (same bytes out: test_snapshots_on_and_off_give_the_same_bytes).
    p.n_ck = s.use_ckpt ? (max_lr + 15 + CK_COLS - 1) / CK_COLS : 0;
    p.ck_stride = (uint64_t)p.n_ck * ck_dwords(R) * 64;  // dwords per pass-1 octet
    p.n_blocks1 = (max_lr + 15 + 3) / 4;
    // LDS per 16-lane group: the window's columns (2 bytes each), a chunk of CH_COLS at a time when it is longer than that
    p.ref_stride1 = std::min((((p.n_blocks1 * 4) * 2 + 15) / 16) * 16, (CH_COLS + 16) * 2);
    p.lds1 = (size_t)p.ref_stride1 * 4;
    const bool alt_rules = (ctx->sc.rules & (FADEHIP_RULE_HDIR_DIAG_F_E | FADEHIP_RULE_GAP_TIE_EXTENDS)) !=
                           (FADEHIP_RULE_HDIR_DIAG_F_E | FADEHIP_RULE_GAP_TIE_EXTENDS);
    p.mode2 = alt_rules ? 3 : 2;
    // chunk so that the snapshots of a chunk fit half the budget (the other half is pass-2 trace scratch)
    const int64_t ck_bytes = (int64_t)p.ck_stride * 4;
    p.total_oct = (n_items + 7) / 8;
    p.chunk_oct = std::max<int64_t>(1, std::min<int64_t>(p.total_oct, (c.budget / 2) / std::max<int64_t>(ck_bytes, 1)));
    // Pass 2 is a persistent launch; a wave traces into its own scratch region, sized for a whole window (a path that
    // left its steps is traced again from step 0).  How many waves: what the previous batch of this class needed (its
    // octets are known by the time its results are fetched), twice over, within what the device holds at once; before
    // any batch has run, a moderate guess.  Few waves cost time only when candidates abound; many cost time always,
    // because each must find a wave slot next to the other slots' score passes before it can see that nothing is left.
    p.wave_stride = (uint64_t)p.n_blocks1 * R * 64;  // dwords
    p.longw = p.n_blocks1 > CH_BLOCKS;
    const int resident = resident_waves(ctx, cls, p.mode2, p.lds1, p.longw);
    const int bound_waves = (int)std::min<int64_t>(p.chunk_oct + NUM_BUCKETS, resident);
    int p2_waves = s.p2_last_octs[cls] >= 0 ? std::min(2 * s.p2_last_octs[cls] + 64, bound_waves) : std::min(1024, bound_waves);
    if (ctx->p2_waves_fixed > 0) p2_waves = std::min(ctx->p2_waves_fixed, bound_waves);
    // ... and within the scratch the budget allows
    p.p2_waves = (int)std::max<int64_t>(1, std::min<int64_t>(p2_waves, (c.budget / 2) / std::max<int64_t>((int64_t)p.wave_stride * 4, 1)));
    p.ckpt_bytes = (size_t)(p.chunk_oct * ck_bytes);
    p.fwd_bytes = (size_t)n_items * sizeof(Fwd);
    p.trace_bytes = (size_t)p.p2_waves * (size_t)p.wave_stride * 4;
    p.cand_bytes = sizeof(Cand) * (size_t)NUM_BUCKETS * (size_t)std::min<int64_t>(n_items, p.chunk_oct * 8);
    return 0;
}

// A slot's patch block (Slot::patch, h_patch), what ends a run in the early order: PatchHead | the run's counter block | entries
constexpr size_t PATCH_ZB_OFF = sizeof(PatchHead), PATCH_LIST_OFF = PATCH_ZB_OFF + Slot::ZB_STRIDE;
static_assert(PATCH_LIST_OFF % 16 == 0 && Slot::ZB_BYTES % 4 == 0, "the gather copies dwords; entries stay 16-byte aligned");

// Two-pass path for one class list, enqueued without a read-back: pass 1 scores every alignment (and,
// when the run asks for them, leaves wave snapshots every CK_COLS steps); the selection — inside the score pass's waves —
// finishes what needs no DP (non-candidates, forced diagonals) and buckets the remaining candidates by the steps to
// re-compute; pass 2 — ONE persistent launch — turns the bucket counts into its table, re-computes those steps with
// trace, walks the tracebacks and traces again, from further back, the few paths that left their steps.
int run_class_two_pass(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c) {
    const int cls = c.cls, n_items = c.n_bound;
    TwoPassPlan p;
    int rc;
    if ((rc = plan_two_pass(ctx, s, c, p))) return rc;
    // (level 2 sized these for all classes before the run's first launch; a buffer that still has to grow here is parked,
    // not freed: earlier launches of this run may be using it)
    if ((rc = reserve_run(ctx, s.trash, s.ckpt, p.ckpt_bytes)) || (rc = reserve_run(ctx, s.trash, s.fwd, p.fwd_bytes)) ||
        (rc = reserve_run(ctx, s.trash, s.trace, p.trace_bytes)) || (rc = reserve_run(ctx, s.trash, s.cand, p.cand_bytes)))
        return rc;
    s.prof_counts[2] = std::max<int64_t>(s.prof_counts[2], (int64_t)p.trace_bytes);
    uint32_t *const sel_counters = s.d_sel(cls);
    const void *const score_fn = sw_kernel(cls, 1, p.longw), *const trace_fn = sw_kernel(cls, p.mode2, p.longw);
    if (!score_fn || !trace_fn) return set_err(ctx, FADEHIP_E_INVALID, "bad class %d", cls);
    int framed = 0;  // (the plan's blocks of four steps cover every window of the class list: what sizes LDS bounds the drift)
    const void *const g8_fn = !p.longw && p.n_ck == 0 ? g8_kernel(ctx, cls, s.max_lq, 4 * p.n_blocks1, &framed) : nullptr;
    if (p.total_oct > p.chunk_oct) s.early = false;  // (one patch list per run: a run without snapshots is one chunk anyway)
    const bool early = s.early;
    for (int64_t o0 = 0; o0 < p.total_oct; o0 += p.chunk_oct) {
        const int octs = (int)std::min<int64_t>(p.chunk_oct, p.total_oct - o0);
        const int i0 = (int)(o0 * 8);
        const int n = std::min(n_items - i0, octs * 8);
        if (!s.sel_fresh[cls]) HIPCHK(ctx, hipMemsetAsync(sel_counters, 0, sizeof(uint32_t) * NUM_BUCKETS, st));
        s.sel_fresh[cls] = false;
        SwArgs a = sw_args(ctx, s, c, i0, n);
        a.ref_stride = p.ref_stride1;
        a.ckpt = (uint32_t *)s.ckpt.p;
        a.ck_stride = p.ck_stride;
        a.n_ck = p.n_ck;
        a.count_dev = c.count_dev;
        a.item_base = (uint32_t)i0;
        // the selection rides in the score pass's waves
        a.sel.enabled = 1;
        a.sel.no_ckpt = p.n_ck == 0 ? 1 : 0;
        a.sel.meta = c.meta ? c.meta + i0 : nullptr;
        a.sel.floor_len = c.floor_len;
        a.sel.trace_all = ctx->prm.trace_all;
        a.sel.span_slack = ctx->span_slack;
        a.sel.cand = (Cand *)s.cand.p;
        a.sel.cap = (uint32_t)n;
        a.sel.bucket_n = sel_counters;
        a.sel.out = c.out;
        a.sel.rs = c.rs;
        a.sel.stats = (c.rs && c.gate) ? s.d_stats() : nullptr;
        a.sel.gate = c.gate;
        a.sel.match = getenv("FADEHIP_NO_SHORTCUT") ? 0 : ctx->sc.match;  // read per run: a test flips it on a live ctx
        a.sel.mismatch = ctx->sc.mismatch;
        // the score pass goes to the slot's CU-masked stream (fork / join by events); its timing events are recorded there
        hipStream_t sst = s.score_stream ? s.score_stream : st;
        if (sst != st) {
            int ef = -1;
            if ((rc = record(ctx, s, &ef, st))) return rc;
            HIPCHK(ctx, hipStreamWaitEvent(sst, s.ev[ef], 0));
        }
        ChunkSpans sp{c.timed};
        if ((rc = sp.mark(ctx, s, 0, sst))) return rc;
        const void *fn1 = score_fn;
        int waves1 = octs;
        size_t lds = p.lds1;
        if (ctx->score_persist && class_rows(cls) == 10 && !p.longw && s.tickets_used < (int)Slot::N_TICKETS) {
            // the A/B variant: as many waves as the CUs of the stream hold at once, each drawing octets by ticket
            const int res = resident_waves(ctx, cls, 1, p.lds1, p.longw);
            const int cus = std::max(ctx->cu_count, 1), mine = s.score_stream ? std::max(cus - 8 * ctx->tail_cus_per_xcd, 1) : cus;
            fn1 = (const void *)sw_pk_kernel<10, 1, false, 16, true>;
            waves1 = std::max(1, std::min(octs, (int)((int64_t)res * mine / cus)));
            a.ticket = s.d_ticket(s.tickets_used++);
        } else if (g8_fn) {  // sixteen alignments per wavefront, two groups' windows in LDS
            if (ctx->debug && o0 == 0) fprintf(stderr, "[fadehip] class of %d rows: score pass on eight-lane groups (longest read of the batch: %d), column-drift frame %s, row drift %s\n", 16 * class_rows(cls), s.max_lq, framed ? "on" : "off", framed == 2 ? "on" : "off");
            fn1 = g8_fn;
            waves1 = (n + 15) / 16;
            lds = 2 * p.lds1;
        }
        if ((rc = launch_sw(ctx, fn1, waves1, lds, sst, a))) return rc;
        if ((rc = sp.mark(ctx, s, 1, sst))) return rc;
        hipStream_t p2st = st;  // where pass 2 runs
        if (sst != st || early) {
            int ej = sp.e[1];  // the join waits for the timing event where there is one
            if (ej < 0 && (rc = record(ctx, s, &ej, sst))) return rc;
            if (sst != st) HIPCHK(ctx, hipStreamWaitEvent(st, s.ev[ej], 0));
            if (early) {
                // Early order: every entry but the candidates' is final here (select_one wrote it), so the array leaves now,
                // behind the score pass on its stream, and pass 2 runs beside the copy (variants: the copy on the slot's
                // stream, pass 2 on the tail stream).  The copy may read a candidate's entry while pass 2 writes it: those
                // entries, and only those, come again in the patch list.
                if (s.tail_stream) {
                    p2st = s.tail_stream;
                    HIPCHK(ctx, hipStreamWaitEvent(p2st, s.ev[ej], 0));
                }
                HIPCHK(ctx, hipMemcpyAsync(s.res.p + s.res_aln_off, s.aln.p, sizeof(fadehip_aln) * (size_t)s.out_cap, hipMemcpyDeviceToHost,
                                           s.tail_stream ? st : sst));
                // ... and so does rs: select_one wrote every record's byte, pass 2 sets bits in the candidates' only, and a
                // candidate's final byte comes in its patch entry
                HIPCHK(ctx, hipMemcpyAsync(s.res.p, c.rs, (size_t)s.n_reads, hipMemcpyDeviceToHost, s.tail_stream ? st : sst));
            }
        }
        // pass 2 + tracebacks + re-traced paths: one persistent launch
        if (s.tickets_used >= (int)Slot::N_TICKETS)
            return set_err(ctx, FADEHIP_E_UNSUPPORTED, "more than %d pass-2 launches in one run (raise trace_bytes)", (int)Slot::N_TICKETS);
        SwArgs b2 = a;
        b2.sel.enabled = 0;
        b2.n_items = 0;
        b2.cand = (const Cand *)s.cand.p;
        b2.cand_cap = (uint32_t)n;
        b2.bucket_n = sel_counters;
        b2.cand_total = &s.d_plan()->cand_total;
        b2.trace = (uint32_t *)s.trace.p;
        b2.quad_stride = p.wave_stride;
        b2.count_dev = nullptr;
        b2.ticket = s.d_ticket(s.tickets_used++);
        b2.meta = c.meta ? c.meta + i0 : nullptr;
        b2.out = c.out;
        b2.rs = c.rs;
        b2.stats = (c.rs && c.gate) ? s.d_stats() : nullptr;
        b2.floor_len = c.floor_len;
        b2.gate = c.gate;
        b2.early_out = (c.gate && c.meta && !ctx->prm.trace_all) ? 1 : 0;
        b2.rerun_total = &s.d_plan()->rerun_total;
        if ((rc = launch_sw(ctx, trace_fn, std::min(p.p2_waves, octs + NUM_BUCKETS), p.lds1, p2st, b2))) return rc;
        if ((rc = sp.mark(ctx, s, 2, p2st))) return rc;
        if (early) {
            // the entries pass 2 left, gathered for the host; then what ran beside the slot's stream (the copy, or pass 2 and
            // the gather) joins it again: the slot's stream still completes only when the whole run has
            PatchArgs pa;
            pa.cand = b2.cand;
            pa.cand_cap = b2.cand_cap;
            pa.bucket_n = sel_counters;
            pa.work = b2.work;
            pa.out = c.out;
            pa.out_cap = s.out_cap;
            pa.head = (PatchHead *)s.patch.p;
            pa.list = (PatchEntry *)((uint8_t *)s.patch.p + PATCH_LIST_OFF);
            pa.cap = s.patch_cap;
            pa.rs = c.rs;
            pa.zb = (const uint32_t *)s.zb();
            pa.zb_out = (uint32_t *)((uint8_t *)s.patch.p + PATCH_ZB_OFF);
            pa.zb_next = (uint32_t *)((uint8_t *)s.zblock.p + (s.zoff ^ Slot::ZB_STRIDE));  // the next run's counters, zeroed in passing
            pa.zb_dwords = (uint32_t)(Slot::ZB_BYTES / 4);
            s.zb_next_clean = true;
            const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(64, (s.patch_sent * (uint32_t)(sizeof(PatchEntry) / 4) + 255) / 256));
            hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks), dim3(256), 0, p2st, pa);
            HIPCHK(ctx, hipGetLastError());
            int et = -1;
            if ((rc = record(ctx, s, &et, s.tail_stream ? p2st : sst))) return rc;
            HIPCHK(ctx, hipStreamWaitEvent(st, s.ev[et], 0));
        }
    }
    return 0;
}

// Single-pass kernels (FADEHIP_KERNEL=pk|int32, and scoring schemes beyond the two-pass ranges): forward with full
// trace + traceback for one class list whose item count the host knows, chunked so the trace fits the budget.
int run_class_single(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c) {
    const int cls = c.cls, R = class_rows(cls), n_items = c.n_bound, max_lr = c.max_lr;
    const bool packed = ctx->use_packed;
    const int per_wave = packed ? 8 : 4;  // alignments per wavefront
    const int n_blocks = (max_lr + 15 + 3) / 4;
    // dwords of trace per wave: 4 bits per cell slot either way
    const uint64_t quad_stride = (uint64_t)n_blocks * (packed ? R : R / 2) * 64;
    const int ref_stride = packed ? std::min((((n_blocks * 4) * 2 + 15) / 16) * 16, (CH_COLS + 16) * 2) : (((n_blocks * 4) + 15) / 16) * 16;
    const size_t lds = (size_t)ref_stride * 4;
    if (lds > 64 * 1024)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "reference window of %d bases needs %zu B LDS per wave (max 64 KiB)", max_lr, lds);
    const int64_t quad_bytes = (int64_t)quad_stride * 4;
    int64_t max_quads = std::max<int64_t>(1, c.budget / quad_bytes);
    const int total_quads = (n_items + per_wave - 1) / per_wave;
    const int64_t chunk_quads = std::min<int64_t>(max_quads, total_quads);
    int rc = reserve_run(ctx, s.trash, s.trace, (size_t)(chunk_quads * quad_bytes));
    if (rc) return rc;
    rc = reserve_run(ctx, s.trash, s.fwd, (size_t)n_items * sizeof(Fwd));
    if (rc) return rc;
    const void *const fn = sw_kernel(cls, packed ? 0 : SW_INT32, n_blocks > CH_BLOCKS);
    if (!fn) return set_err(ctx, FADEHIP_E_INVALID, "bad class %d", cls);
    for (int64_t q0 = 0; q0 < total_quads; q0 += chunk_quads) {
        const int quads = (int)std::min<int64_t>(chunk_quads, total_quads - q0);
        const int i0 = (int)(q0 * per_wave);
        const int n = std::min(n_items - i0, quads * per_wave);
        SwArgs a = sw_args(ctx, s, c, i0, n);
        a.trace = (uint32_t *)s.trace.p;
        a.quad_stride = quad_stride;
        a.ref_stride = ref_stride;
        ChunkSpans sp{c.timed};
        if ((rc = sp.mark(ctx, s, 0, st))) return rc;
        if ((rc = launch_sw(ctx, fn, quads, lds, st, a))) return rc;
        if ((rc = sp.mark(ctx, s, 1, st))) return rc;
        TbArgs t = {};  // (count_dev stays null: n is exact here, the host read the counts back)
        t.R = R;
        t.packed = packed ? 1 : 0;
        t.trace = (const uint32_t *)s.trace.p;
        t.quad_stride = quad_stride;
        if ((rc = launch_traceback(ctx, s, st, c, i0, n, t))) return rc;
        if ((rc = sp.mark(ctx, s, 2, st))) return rc;
        s.prof_counts[2] += (int64_t)quads * quad_bytes;
    }
    return 0;
}

// Long list on the wave kernel with one alignment per wavefront (sw_forward64_kernel): reads of up to 4,096 bases, windows
// of up to LONG_WAVE_MAX_WINDOW columns, under the default Appendix A.3 / A.4 rules only: the kernel picks its end cell by
// END_MIN_REF_THEN_QUERY, opens gaps by GAP_TIE_EXTENDS and writes trace bit 4 as "F < T", which traceback_path reads as
// "E < T" when HDIR_DIAG_F_E is off (run_long keeps such lists away from here).
// n_bound / max_lq / max_lr are upper bounds, the live count stays on the device.
constexpr int LONG_WAVE_MAX_QUERY = 4096, LONG_WAVE_MAX_WINDOW = 65000;
int run_long_wave(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c, int max_lq) {
    const int n_items = c.n_bound, max_lr = c.max_lr;
    // rows per lane: the smallest of 12 / 16 / 24 / 32 / 48 / 64 that holds the list's longest read (64: 256 VGPRs + 220 AGPRs, one wave per SIMD)
    const int R = max_lq <= 768 ? 12 : max_lq <= 1024 ? 16 : max_lq <= 1536 ? 24 : max_lq <= 2048 ? 32 : max_lq <= 3072 ? 48 : 64;
    if (ctx->debug) fprintf(stderr, "[fadehip] long list of %d alignments (longest read %d, widest window %d): wave64 R=%d\n", n_items, max_lq, max_lr, R);
    const int n_blocks = (max_lr + 63 + 3) / 4;
    const uint64_t quad_stride = (uint64_t)n_blocks * (R / 2) * 64;  // dwords of trace per alignment
    const size_t lds = (size_t)(((n_blocks * 4) + 15) / 16) * 16;
    const int64_t item_bytes = (int64_t)quad_stride * 4;
    const int64_t chunk = std::min<int64_t>(n_items, std::max<int64_t>(1, c.budget / item_bytes));
    int rc;
    if ((rc = reserve_run(ctx, s.trash, s.fwd, (size_t)n_items * sizeof(Fwd))) || (rc = reserve_run(ctx, s.trash, s.trace, (size_t)(chunk * item_bytes)))) return rc;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, n_items - i0);
        SwArgs a = sw_args(ctx, s, c, i0, n);
        a.trace = (uint32_t *)s.trace.p;
        a.quad_stride = quad_stride;
        a.ref_stride = (int32_t)lds;
        a.count_dev = c.count_dev;
        a.item_base = (uint32_t)i0;
        ChunkSpans sp{c.timed};
        if ((rc = sp.mark(ctx, s, 0, st))) return rc;
        if ((rc = launch_sw(ctx, sw64_kernel(R), n, lds, st, a))) return rc;
        if ((rc = sp.mark(ctx, s, 1, st))) return rc;
        TbArgs t = {};
        t.R = R;
        t.packed = 3;
        t.trace = (const uint32_t *)s.trace.p;
        t.quad_stride = quad_stride;
        t.count_dev = c.count_dev;
        t.item_base = (uint32_t)i0;
        if ((rc = launch_traceback(ctx, s, st, c, i0, n, t))) return rc;
        if ((rc = sp.mark(ctx, s, 2, st))) return rc;
        s.prof_counts[2] += (int64_t)n * item_bytes;
    }
    return 0;
}

// Queries longer than 512 bases (or windows beyond the wave kernels' LDS): what the one-alignment-per-wave kernel holds
// goes there; sw_long_kernel (thread per alignment, full trace) + the common traceback keep the rest (longer reads, wider
// windows, and any list under a non-default end-cell, gap-tie or traceback-direction rule: sw_long_kernel reads all three
// switches.  FADEHIP_LONG_THREAD=1 sends everything to it, for A/B runs).  FADEHIP_DEBUG names the runner of each list.
int run_long(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c, int max_lq) {
    const int n_items = c.n_bound, max_lr = c.max_lr;
    const uint32_t need_rules = FADEHIP_RULE_END_MIN_REF_THEN_QUERY | FADEHIP_RULE_GAP_TIE_EXTENDS | FADEHIP_RULE_HDIR_DIAG_F_E;
    if (max_lq <= LONG_WAVE_MAX_QUERY && max_lr <= LONG_WAVE_MAX_WINDOW && (ctx->sc.rules & need_rules) == need_rules && !getenv("FADEHIP_LONG_THREAD"))
        return run_long_wave(ctx, s, st, c, max_lq);
    if (ctx->debug) fprintf(stderr, "[fadehip] long list of %d alignments (longest read %d, widest window %d): thread\n", n_items, max_lq, max_lr);
    const int lhalf = (max_lr + 1) / 2;
    const int64_t per_item = (int64_t)max_lq * lhalf + 8 * (int64_t)max_lr;
    const int64_t chunk = std::min<int64_t>(n_items, c.budget / std::max<int64_t>(per_item, 1));
    if (chunk < 1)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "a %d x %d alignment needs %lld B of trace, more than trace_bytes", max_lq, max_lr,
                       (long long)per_item);
    int rc;
    if ((rc = reserve_run(ctx, s.trash, s.fwd, (size_t)n_items * sizeof(Fwd)))) return rc;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, n_items - i0);
        if ((rc = reserve_run(ctx, s.trash, s.trace, (size_t)max_lq * (size_t)lhalf * (size_t)n)) ||
            (rc = reserve_run(ctx, s.trash, s.lrows, 8 * (size_t)max_lr * (size_t)n)))
            return rc;
        LongArgs a;
        memset(&a, 0, sizeof a);
        a.work = c.work + i0;
        a.n_items = n;
        a.q_nib = c.q_nib;
        a.r_nib = c.r_nib;
        a.hrow = (int32_t *)s.lrows.p;
        a.frow = (int32_t *)s.lrows.p + (size_t)max_lr * (size_t)n;
        a.trace = (uint8_t *)s.trace.p;
        a.lhalf = lhalf;
        a.max_lq = max_lq;
        a.max_lr = max_lr;
        a.fwd = (Fwd *)s.fwd.p + i0;
        a.sc = ctx->sc;
        a.count_dev = c.count_dev;
        a.item_base = (uint32_t)i0;
        ChunkSpans sp{c.timed};
        if ((rc = sp.mark(ctx, s, 0, st))) return rc;
        hipLaunchKernelGGL(sw_long_kernel, dim3((n + 63) / 64), dim3(64), 0, st, a);
        HIPCHK(ctx, hipGetLastError());
        if ((rc = sp.mark(ctx, s, 1, st))) return rc;
        TbArgs t = {};
        t.R = 1;
        t.packed = 2;
        t.ltrace = (const uint8_t *)s.trace.p;
        t.lhalf = lhalf;
        t.count_dev = c.count_dev;
        t.item_base = (uint32_t)i0;
        if ((rc = launch_traceback(ctx, s, st, c, i0, n, t))) return rc;
        if ((rc = sp.mark(ctx, s, 2, st))) return rc;
        s.prof_counts[2] += (int64_t)max_lq * lhalf * n;
    }
    return 0;
}

}  // namespace

namespace fadehip::host {

// A stream on CUs [lo, hi) of every XCD (mask bit i is CU i / 8 of XCD i % 8 on MI355X); nullptr where the stack has no CU masks.
hipStream_t xcd_slice_stream(fadehip_ctx *ctx, int lo, int hi) {
    if (ctx->cu_count < 64 || ctx->cu_count % 32) return nullptr;
    std::vector<uint32_t> mask((size_t)ctx->cu_count / 32, 0u);
    for (int i = 0; i < ctx->cu_count; i++)
        if (i / 8 >= lo && i / 8 < hi) mask[(size_t)i / 32] |= 1u << (i % 32);
    hipStream_t q = nullptr;
    if (hipExtStreamCreateWithCUMask(&q, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return q;
}

// streams, events and the pinned counter block of a slot, made when the slot is first used
int ensure_slot(fadehip_ctx *ctx, Slot &s) {
    static_assert(sizeof(uint32_t) * (2 * NUM_LISTS + 4) <= Slot::ZB_C64 - Slot::ZB_COUNTERS, "gate counters overflow their slice");
    static_assert(Slot::ZB_SEL + Slot::ZB_SEL_STRIDE * NUM_CLASSES <= Slot::ZB_STATS, "selection counters overlap the stats");
    static_assert(sizeof(uint32_t) * NUM_BUCKETS <= Slot::ZB_SEL_STRIDE, "selection counters overflow their slice");
    static_assert(sizeof(PlanOut) <= 128, "PlanOut overflows its slice");
    if (s.h_zb) return 0;
    if (!s.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));  // (the file path lends slot 0 the ctx's copy stream)
    HIPCHK(ctx, hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming));
    HIPCHK(ctx, hipHostMalloc((void **)&s.h_zb, Slot::ZB_BYTES));
    memset(s.h_zb, 0, Slot::ZB_BYTES);
    if (ctx->tail_cus_per_xcd > 0 && ctx->cu_count >= 64 && ctx->cu_count % 32 == 0) {
        // Bits 33 k + 8 j, k = 0..7, j < tail CUs per XCD: one CU in each of the 8 XCDs whether the mask counts CUs
        // XCD-interleaved (bit i -> XCD i % 8; what MI355X does: a mask that clears bit 0 of every word instead takes
        // eight CUs from one XCD and costs the score pass 25 %) or XCD by XCD; everything else is enabled.
        std::vector<uint32_t> mask((size_t)ctx->cu_count / 32, 0xffffffffu);
        for (int x = 0; x < 8 && 33 * x < ctx->cu_count; x++)
            for (int j = 0; j < ctx->tail_cus_per_xcd && j < 3; j++) {
                const int bit = 33 * x + 8 * j;
                if (bit < ctx->cu_count) mask[(size_t)bit / 32] &= ~(1u << (bit % 32));
            }
        if (const char *kv = getenv("FADEHIP_CU_MASK")) {  // experiments: comma-separated hex words, lowest CUs first
            size_t w = 0;
            for (const char *q = kv; *q && w < mask.size(); w++) {
                mask[w] = (uint32_t)strtoul(q, nullptr, 16);
                q = strchr(q, ',');
                if (!q) break;
                q++;
            }
        }
        if (hipExtStreamCreateWithCUMask(&s.score_stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            s.score_stream = nullptr;  // no CU masks on this stack: the score pass stays on the slot's stream
        } else {
            s.score_mask = mask;
        }
    }
    return 0;
}

}  // namespace fadehip::host

namespace {

// The tail stream of a slot's early order where pass 2 leaves the slot's stream (FADEHIP_EARLY_TAIL=masked | plain, or a
// slot without a score stream), made when a run first takes that order: on the CUs the score mask leaves free, or a plain
// stream.  One more stream per slot in use, 3 N + 1, which is why the default does without it.
int ensure_tail(fadehip_ctx *ctx, Slot &s) {
    if (s.tail_stream || s.tail_tried) return 0;
    s.tail_tried = true;
    if (ctx->early_tail == 1 && !s.score_mask.empty()) {
        std::vector<uint32_t> mask(s.score_mask.size());
        uint32_t any = 0;
        for (size_t w = 0; w < mask.size(); w++) any |= (mask[w] = ~s.score_mask[w]);
        if (any && hipExtStreamCreateWithCUMask(&s.tail_stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            s.tail_stream = nullptr;
        }
    }
    if (!s.tail_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&s.tail_stream, hipStreamNonBlocking));
    return 0;
}

int check_slot(fadehip_ctx *ctx, int slot) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= FADEHIP_NUM_SLOTS) return set_err(ctx, FADEHIP_E_INVALID, "slot %d out of range", slot);
    return 0;
}

// typed views of the batch in flight, on the host and on the device
template <class T>
const T *d_arr(const Slot &s, int k) { return (const T *)((const uint8_t *)s.in[s.cur].p + s.L.off[k]); }

// anno.d:61 + util.d:37-62 + dhtslib alignedLength over one record's CIGAR, as gate_kernel computes them
struct CigarSummary {
    int n_soft;
    uint32_t clipL, clipR;
    int64_t aligned;
};
inline CigarSummary summarize_cigar(const uint32_t *ops, uint32_t c0, uint32_t c1) {
    CigarSummary r = {0, 0, 0, 0};
    bool first = true;
    for (uint32_t k = c0; k < c1; k++) {
        const uint32_t op = ops[k] & 15u, len = ops[k] >> 4;
        if (op == 4) r.n_soft++;
        if (FADEHIP_OP_CONSUMES_REF(op)) r.aligned += len;
        if (op == 5) continue;
        const bool is_sc = (op == 4);
        if (first && !is_sc) first = false;
        else if (first && is_sc) r.clipL = len;
        else if (is_sc) r.clipR = len;
    }
    return r;
}

}  // namespace

namespace fadehip::host {

// What upload leaves plan_run, for a batch the device packed and counted itself (the file path): n_sent records that carry
// bases, of l_seq_min .. l_seq_max bases, n_long_q of them beyond 512, no alignedLength above span_max.
void bound_counted_batch(Slot &s, uint32_t n_sent, uint32_t l_seq_min, uint32_t l_seq_max, uint32_t n_long_q, int64_t span_max) {
    memset(s.hist, 0, sizeof s.hist);
    s.wide.clear();
    s.wide_all = false;
    s.out_bound = n_sent;
    s.max_lq = 0;
    s.l_seq_lo = 0;  // (the bounds below are counted on the device over these very records)
    s.l_seq_hi = INT32_MAX;
    s.span_bound = 1;
    if (n_sent) {
        const int lmin = (int)std::min<uint32_t>(l_seq_min, (uint32_t)MAX_LONG_QUERY), lmax = (int)std::min<uint32_t>(l_seq_max, (uint32_t)MAX_LONG_QUERY);
        const int c_lo = list_of_len(std::max(lmin, 1)), c_hi = list_of_len(std::max(lmax, 1));
        for (int c = c_lo; c <= c_hi; c++) s.hist[c] = n_sent;  // any of them may be of any length in between
        if (n_long_q) s.hist[LONG_LIST] = n_long_q;  // (the exact number of reads beyond 512 bases)
        s.max_lq = std::max(lmax, 1);
        s.span_bound = std::max<int64_t>(span_max, 1);
        s.wide_all = s.span_bound > WIDE_MIN_SPAN;
    }
}

// Host-side bounds of a run (the launches are sized from these; the device keeps the real counts and checks every bound
// before it writes: a record beyond one is reported at results, never trusted).
int plan_run(fadehip_ctx *ctx, Slot &s) {
    const int64_t w = s.window;
    for (int c = 0; c < NUM_LISTS; c++) s.bound[c] = s.hist[c];
    const int64_t lr_bound = std::min<int64_t>(s.span_bound + 2 * w, ctx->prm.max_ref_len);
    s.wave_lr_bound = (int)std::min<int64_t>(lr_bound, WAVE_MAX_WINDOW);
    s.long_max_lq = s.max_lq;
    s.long_max_lr = (int)std::max<int64_t>(lr_bound, 1);
    if (lr_bound > WAVE_MAX_WINDOW) {
        // Some window may exceed what the wave kernels stage in LDS.  Which records go to the long list depends on the
        // window size, which only the run knows; upload kept the reads whose alignedLength alone is long (spliced reads,
        // large deletions), so the count needs no second look at the caller's arrays (they need not outlive results).
        uint32_t n_long = s.hist[LONG_LIST];  // reads beyond 512 bases
        int64_t max_lr = 1;
        int max_lq = s.hist[LONG_LIST] ? std::min(s.max_lq, MAX_LONG_QUERY) : 1;
        if (2 * w + WIDE_MIN_SPAN > WAVE_MAX_WINDOW || s.wide_all) {
            // with this window size a read of ordinary span may have a long window: any record that carries bases may
            // land on the long list
            n_long = s.out_bound;
            max_lr = lr_bound;
            max_lq = std::min(std::max(s.max_lq, 1), MAX_LONG_QUERY);
        } else {
            for (const auto &wr : s.wide)
                if (wr.first + 2 * w > WAVE_MAX_WINDOW) {
                    if (wr.second <= 16 * class_rows(NUM_CLASSES - 1)) n_long++;  // (longer reads are counted already)
                    max_lq = std::max(max_lq, std::min(wr.second, MAX_LONG_QUERY));
                    max_lr = std::max(max_lr, std::min<int64_t>(wr.first + 2 * w, lr_bound));
                }
            if (s.hist[LONG_LIST]) max_lr = lr_bound;
        }
        s.bound[LONG_LIST] = std::min(n_long, s.out_bound);
        s.long_max_lq = max_lq;
        s.long_max_lr = (int)max_lr;
    }
    return 0;
}

}  // namespace fadehip::host

namespace {

// List c of the slot's level-2 run, at the bounds plan_run left (the caller lowers n_bound where it knows the count).
ClassRun level2_class_run(const fadehip_ctx *ctx, const Slot &s, int c, int64_t budget) {
    ClassRun cr;
    cr.cls = c;
    cr.work = (const Work *)s.work[c].p;
    cr.meta = (const Meta *)s.meta[c].p;
    cr.n_bound = (int)s.bound[c];
    cr.count_dev = s.d_counters() + c;
    cr.max_lr = c == LONG_LIST ? s.long_max_lr : std::max(s.wave_lr_bound, 1);
    cr.q_nib = d_arr<uint8_t>(s, A_SEQ);
    cr.r_nib = (const uint8_t *)ctx->genome.p;
    cr.out = (fadehip_aln *)s.aln.p;
    cr.rs = (uint8_t *)s.rs.p;
    cr.floor_len = s.floor_len;
    cr.gate = 1;
    cr.budget = budget;
    cr.timed = true;
    return cr;
}

}  // namespace

namespace fadehip::host {

// Enqueue one whole run of the slot's uploaded batch on its stream (two-pass path: nothing is read back).
int enqueue_run(fadehip_ctx *ctx, Slot &s) {
    hipStream_t st = s.stream;
    const int n = s.n_reads;
    const int floor_len = s.floor_len;
    s.ev_used = 0;
    s.fwd_spans.clear();
    s.tb_spans.clear();
    s.tickets_used = 0;
    memset(s.prof_counts, 0, sizeof s.prof_counts);
    int rc;
    // (the file path's batches differ a little in size from call to call: its buffers get headroom so that they settle)
    auto rsv = [&](DevBuf &b, size_t bytes) { return s.device_only ? reserve_roomy(ctx, b, bytes) : reserve(ctx, b, bytes); };
    // one result array for all lists: an alignment reports into the entry the gate hands it (Work::out)
    uint32_t total_bound = 0;
    for (int c = 0; c < NUM_LISTS; c++) total_bound += s.bound[c];
    total_bound = std::min(total_bound, s.out_bound);
    s.out_cap = total_bound;
    s.res_aln_off = ((size_t)n + 255) & ~(size_t)255;
    if (s.zblock.cap < 2 * Slot::ZB_STRIDE) s.zb_next_clean = false, s.zoff = 0;  // (a new allocation)
    if ((rc = rsv(s.rs, (size_t)n)) || (rc = rsv(s.aln, sizeof(fadehip_aln) * (size_t)std::max<uint32_t>(total_bound, 1))) ||
        (rc = reserve(ctx, s.zblock, 2 * Slot::ZB_STRIDE)) ||
        (!s.device_only && (rc = reserve_pinned(ctx, s.res, s.res_aln_off + sizeof(fadehip_aln) * (size_t)total_bound))))
        return rc;
    for (int c = 0; c < NUM_LISTS; c++) {
        if (!s.bound[c]) continue;
        if ((rc = rsv(s.work[c], sizeof(Work) * (size_t)s.bound[c])) || (rc = rsv(s.meta[c], sizeof(Meta) * (size_t)s.bound[c])))
            return rc;
    }
    const int64_t budget = ctx->prm.trace_bytes > 0 ? ctx->prm.trace_bytes : ((int64_t)16 << 30);
    // snapshots only when the slot's previous run had many pass-2 candidates (plan_two_pass); FADEHIP_CKPT=0/1 pins it
    s.use_ckpt = s.last_cand * 32 > std::max<int64_t>(s.last_aln, 1);
    if (const char *kv = getenv("FADEHIP_CKPT")) s.use_ckpt = atoi(kv) != 0;
    if (ctx->two_pass) {
        // the scratch of every class of this run, sized once before the first launch (nothing is re-allocated between
        // kernels already queued; the slot is idle here: run waited for its previous results)
        size_t need_ckpt = 0, need_fwd = 0, need_trace = 0, need_cand = 0;
        for (int c = 0; c < NUM_CLASSES; c++) {
            if (!s.bound[c]) continue;
            TwoPassPlan p;
            if ((rc = plan_two_pass(ctx, s, level2_class_run(ctx, s, c, budget), p))) return rc;
            need_ckpt = std::max(need_ckpt, p.ckpt_bytes);
            need_fwd = std::max(need_fwd, p.fwd_bytes);
            need_trace = std::max(need_trace, p.trace_bytes);
            need_cand = std::max(need_cand, p.cand_bytes);
        }
        if ((rc = reserve_run(ctx, s.trash, s.ckpt, need_ckpt)) || (rc = reserve_run(ctx, s.trash, s.fwd, need_fwd)) ||
            (rc = reserve_run(ctx, s.trash, s.trace, need_trace)) || (rc = reserve_run(ctx, s.trash, s.cand, need_cand)))
            return rc;
    }
    // The order of the run's tail.  Late: pass 2 on the slot's stream, then every copy.  Early: the alignment array is
    // copied right behind the score pass, on the score stream, pass 2 runs beside that copy, and the entries it wrote
    // follow in a patch list (run_class_two_pass, finish_run).  Early takes one class list and nothing else to run, results
    // that go to the host, no snapshots (one chunk), and few candidates in the slot's previous run: at most half the patch
    // list's capacity (a slot's first run qualifies; a run whose candidates overflow the list all the same is copied again
    // by finish_run, and the slot's next run is late).
    {
        int n_cls = 0;
        for (int c = 0; c < NUM_CLASSES; c++) n_cls += s.bound[c] ? 1 : 0;
        const char *why = nullptr;
        if (!ctx->early_copy) why = "FADEHIP_EARLY_COPY=0";
        else if (!ctx->two_pass) why = "single-pass kernels";
        else if (s.device_only) why = "results stay on the device";
        else if (n_cls != 1) why = "not exactly one class list";
        else if (s.bound[LONG_LIST]) why = "long list";
        else if (ctx->prm.trace_all) why = "trace_all";
        else if (s.last_cand * 2 > ctx->patch_cap) why = "the previous run's candidates exceed half the patch list";
        else if (s.use_ckpt) why = "snapshots";
        else if (!total_bound) why = "no alignments";
        s.early = why == nullptr;
        if (s.early) {
            s.patch_cap = (uint32_t)ctx->patch_cap;
            s.patch_sent = (uint32_t)std::min<int64_t>(s.patch_cap, 2 * s.last_cand + 64);  // entries copied with the run; finish_run fetches the rest
            const size_t bytes = PATCH_LIST_OFF + sizeof(PatchEntry) * (size_t)std::max<uint32_t>(s.patch_cap, 1);
            if (((ctx->early_tail || !s.score_stream) && (rc = ensure_tail(ctx, s))) || (rc = reserve(ctx, s.patch, bytes)) ||
                (rc = reserve_pinned(ctx, s.h_patch, bytes)))
                return rc;
        }
        if (ctx->debug)
            fprintf(stderr, "[fadehip] copy order: %s (%s)\n", s.early ? "early" : "late",
                    !s.early ? why : !s.tail_stream ? "the copy on the score stream" : ctx->early_tail == 1 && !s.score_mask.empty() ? "pass 2 on the CUs the score mask leaves free" : "pass 2 on a plain stream");
    }
    // every counter of the run: the block the slot's previous run zeroed behind its last copy, or one fill here
    if (s.zb_next_clean) s.zoff ^= Slot::ZB_STRIDE;
    else HIPCHK(ctx, hipMemsetAsync(s.zb(), 0, Slot::ZB_BYTES, st));
    s.zb_next_clean = false;
    for (int c = 0; c < NUM_CLASSES; c++) s.sel_fresh[c] = true;
    if ((rc = record(ctx, s, &s.ev_gate0))) return rc;
    GateArgs g;
    memset(&g, 0, sizeof g);
    g.n_reads = n;
    g.tid = d_arr<int32_t>(s, A_TID);
    g.pos = d_arr<int32_t>(s, A_POS);
    g.l_seq = d_arr<int32_t>(s, A_LSEQ);
    g.flag = d_arr<uint16_t>(s, A_FLAG);
    g.has_sa = d_arr<uint8_t>(s, A_SA);
    g.cigar_off = d_arr<uint32_t>(s, A_CIGOFF);
    g.cigar_ops = d_arr<uint32_t>(s, A_CIG);
    g.seq_off = d_arr<uint32_t>(s, A_SEQOFF);
    g.floor_len = floor_len;
    g.window = s.window;
    g.n_contigs = ctx->n_contigs;
    g.contig_len = (const int64_t *)ctx->contig_len.p;
    g.contig_base = (const uint64_t *)ctx->contig_base.p;
    g.max_ref_len = ctx->prm.max_ref_len;
    g.wave_lr_bound = s.wave_lr_bound;
    g.long_lr_bound = s.long_max_lr;
    g.long_lq_bound = std::max(s.long_max_lq, 1);
    g.l_seq_lo = s.l_seq_lo;
    g.l_seq_hi = s.l_seq_hi;
    g.rs = (uint8_t *)s.rs.p;
    for (int c = 0; c < NUM_LISTS; c++) {
        g.work[c] = (Work *)s.work[c].p;
        g.meta[c] = (Meta *)s.meta[c].p;
        g.list_cap[c] = s.bound[c];
    }
    g.out_cap = s.out_cap;
    g.n_cigar_ops = (uint32_t)(s.L.bytes[A_CIG] / 4);
    g.n_seq_bytes = (uint32_t)s.L.bytes[A_SEQ];
    g.stats = s.d_stats();
    g.counters = s.d_counters();
    g.counters64 = s.d_counters64();
    hipLaunchKernelGGL(gate_kernel, dim3((n + GATE_TILE - 1) / GATE_TILE), dim3(GATE_BLOCK), 0, st, g);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = record(ctx, s, &s.ev_gate1))) return rc;
    uint32_t exact[NUM_LISTS];
    for (int c = 0; c < NUM_LISTS; c++) exact[c] = s.bound[c];
    if (!ctx->two_pass) {
        // single-pass kernels: their launches take the real counts
        HIPCHK(ctx, hipMemcpyAsync(s.h_zb, s.zb(), 128, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int c = 0; c < NUM_LISTS; c++) exact[c] = std::min(s.h_counters()[c], s.bound[c]);
    }
    for (int c = 0; c < NUM_CLASSES; c++) {
        if (!exact[c]) continue;
        ClassRun cr = level2_class_run(ctx, s, c, budget);
        cr.n_bound = (int)exact[c];
        rc = ctx->two_pass ? run_class_two_pass(ctx, s, st, cr) : run_class_single(ctx, s, st, cr);
        if (rc) return rc;
    }
    if (exact[LONG_LIST]) {
        ClassRun cr = level2_class_run(ctx, s, LONG_LIST, budget);
        cr.n_bound = (int)exact[LONG_LIST];
        if ((rc = run_long(ctx, s, st, cr, std::max(s.long_max_lq, 1)))) return rc;
    }
    if ((rc = record(ctx, s, &s.ev_end))) return rc;
    if (s.early) {
        // Early order: the array and rs left behind the score pass, and the gather kernel put the run's counter block in front
        // of the entries pass 2 wrote and zeroed the other counter block: one copy ends the run.
        HIPCHK(ctx, hipMemcpyAsync(s.h_patch.p, s.patch.p, PATCH_LIST_OFF + sizeof(PatchEntry) * (size_t)s.patch_sent, hipMemcpyDeviceToHost, st));
        return 0;
    }
    // results to the slot's pinned block; the counter block tells the host how many entries of each list are live
    HIPCHK(ctx, hipMemcpyAsync(s.h_zb, s.zb(), Slot::ZB_BYTES, hipMemcpyDeviceToHost, st));
    // the next run's counters, zeroed here, off its critical path (the same batch run again takes them as well)
    HIPCHK(ctx, hipMemsetAsync((uint8_t *)s.zblock.p + (s.zoff ^ Slot::ZB_STRIDE), 0, Slot::ZB_BYTES, st));
    s.zb_next_clean = true;
    if (s.device_only) return 0;
    HIPCHK(ctx, hipMemcpyAsync(s.res.p, s.rs.p, (size_t)n, hipMemcpyDeviceToHost, st));  // (pass 2 sets bits in rs: it stays behind it)
    if (total_bound)
        HIPCHK(ctx, hipMemcpyAsync(s.res.p + s.res_aln_off, s.aln.p, sizeof(fadehip_aln) * (size_t)total_bound, hipMemcpyDeviceToHost, st));
    return 0;
}

// Wait for the slot's run and turn the counter block into results (state 2 -> 3).
int finish_run(fadehip_ctx *ctx, Slot &s, int slot) {
    if (s.state == 3) return 0;
    if (s.state != 2) return set_err(ctx, FADEHIP_E_STATE, "slot %d has not been run", slot);
    hipStream_t st = s.stream;
    const int n = s.n_reads;
    if (n == 0) {
        s.n_aln = 0;
        s.n_oversize = 0;
        memset(s.stats, 0, sizeof s.stats);
        s.stats[0] = s.n_skipped;
        s.state = 3;
        return 0;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (void *q : s.trash) (void)hipFree(q);  // scratch outgrown while this run was enqueued
    s.trash.clear();
    if (s.early) memcpy(s.h_zb, s.h_patch.p + PATCH_ZB_OFF, Slot::ZB_BYTES);  // early order: the counter block came in the patch block
    const uint32_t errbits = s.h_counters()[2 * NUM_LISTS];
    if (errbits) {
        s.state = 0;
        if (errbits & 64u) return set_err(ctx, FADEHIP_E_INVALID, "batch has a record whose cigar_off / seq_off are not non-decreasing within the arrays, or l_seq < 0");
        if (errbits & 8u) return set_err(ctx, FADEHIP_E_INVALID, "batch has a mapped soft-clipped record whose seq_packed slice is shorter than its l_seq");
        if (errbits & 16u) return set_err(ctx, FADEHIP_E_INVALID, "batch has a record whose cigar.alignedLength exceeds ref_span_bound=%lld", (long long)s.span_bound);
        if (errbits & 32u) return set_err(ctx, FADEHIP_E_INVALID, "batch has more records to re-align than its bounds said, or a read outside them (n_with_seq too small, or an l_seq outside l_seq_min / l_seq_max?)");
        return set_err(ctx, FADEHIP_E_INVALID, "batch has a mapped soft-clipped read whose tid is not a contig of the uploaded genome");
    }
    if (s.early) {
        // early order: lay the entries pass 2 wrote over the bulk copy, once, before any view is handed out
        s.early = false;
        const PatchHead head = *(const PatchHead *)s.h_patch.p;
        const PatchEntry *const list = (const PatchEntry *)(s.h_patch.p + PATCH_LIST_OFF);
        uint8_t *const h_aln = s.res.p + s.res_aln_off;
        if (head.overflow || head.n > s.patch_cap) {
            // more candidates than the list holds: the whole array again (rare; the slot's next run is late, see last_cand)
            HIPCHK(ctx, hipMemcpyAsync(h_aln, s.aln.p, sizeof(fadehip_aln) * (size_t)s.out_cap, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(s.res.p, s.rs.p, (size_t)n, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
        } else {
            if (head.n > s.patch_sent) {  // more than the run's copy was sized for: the rest of the list
                HIPCHK(ctx, hipMemcpyAsync((void *)(list + s.patch_sent), (const uint8_t *)s.patch.p + PATCH_LIST_OFF + sizeof(PatchEntry) * (size_t)s.patch_sent,
                                           sizeof(PatchEntry) * (size_t)(head.n - s.patch_sent), hipMemcpyDeviceToHost, st));
                HIPCHK(ctx, hipStreamSynchronize(st));
            }
            for (uint32_t k = 0; k < head.n; k++)
                if (list[k].out < s.out_cap) {
                    memcpy(h_aln + sizeof(fadehip_aln) * (size_t)list[k].out, &list[k].e, sizeof(fadehip_aln));
                    if ((uint32_t)list[k].e.read_idx < (uint32_t)n) s.res.p[list[k].e.read_idx] = (uint8_t)list[k].pad;
                }
        }
        if (ctx->debug)
            fprintf(stderr, "[fadehip] slot %d: patch list of %u entries (%u sent with the run)%s\n", slot, head.n, s.patch_sent,
                    head.overflow ? ", overflow: the array was copied again" : "");
    }
    for (int c = 0; c < NUM_CLASSES; c++)  // what pass 2 served: sizes the next run's persistent launch
        if (s.bound[c]) {
            const uint32_t *bn = (const uint32_t *)(s.h_zb + Slot::ZB_SEL + Slot::ZB_SEL_STRIDE * (size_t)c);
            int octs = 0;
            for (int b = 0; b < NUM_BUCKETS; b++) octs += (int)((bn[b] + 7) / 8);
            s.p2_last_octs[c] = octs;
        }
    // all lists report into one result array: its live entries are the ones the gate handed out
    const uint32_t at = std::min(s.h_counters()[2 * NUM_LISTS + 3], s.out_cap);
    s.n_aln = (int)at;
    s.n_oversize = (int)s.h_counters()[2 * NUM_LISTS + 2];
    for (int k = 0; k < 8; k++) {
        s.stats[k] = 0;
        for (int q = 0; q < STAT_PARTS; q++) s.stats[k] += (int64_t)s.h_stats()[8 * q + k];
    }
    s.stats[0] += s.n_skipped;  // records the caller left out (anno.d:61-65: rs = 0) are reads all the same
    const PlanOut *po = s.h_plan();
    s.n_cand = (int64_t)po->cand_total;
    s.n_rerun = (int64_t)po->rerun_total;
    s.last_cand = s.n_cand;
    s.last_aln = (int64_t)at;
    s.prof_counts[0] = at;
    s.prof_counts[1] = (int64_t)s.h_counters64()[0 * C64_STRIDE];
    // algorithmic bytes of the dominant kernel: SURVEY §8(d)'s packed query + packed window + 16 B
    // descriptor + 64 B result slot per alignment
    s.prof_counts[3] = (int64_t)s.h_counters64()[1 * C64_STRIDE] + (int64_t)at * 80;
    s.prof_counts[4] = ctx->two_pass ? (s.use_ckpt ? (int64_t)s.h_counters64()[2 * C64_STRIDE] : 0) : (int64_t)(s.h_counters64()[0 * C64_STRIDE] / 2);
    s.prof_counts[5] = s.n_cand;
    if (ctx->debug)
        fprintf(stderr, "[fadehip] slot %d: %d reads, %u alignments, %lld candidates traced, %lld re-run, trace need %lld B\n", slot, n, at,
                (long long)s.n_cand, (long long)s.n_rerun, (long long)s.prof_counts[2]);
    s.state = 3;
    return 0;
}

}  // namespace fadehip::host

namespace fadehip::host {

// The launches of sw_stats_kernel over a work list that lies class behind class (cls_begin [6]: R = 1, 2, 4, 8 rows per lane
// in one strip, then the multi-strip class), for fadehip_sw_stats_batch and the reports of bam_report.hpp.  Multi-strip
// pairs: a scratch row of long_max_lr entries per wave, at most 256 MB of them.
int sw_stats_long_blocks(size_t n_long, int long_max_lr, size_t *row_bytes) {
    *row_bytes = (size_t)std::max(long_max_lr, 1) * 2 * sizeof(int4);
    if (!n_long) return 0;
    const size_t waves = std::max<size_t>(1, std::min<size_t>({n_long, ((size_t)256 << 20) / *row_bytes, (size_t)2048}));
    return (int)((waves + STATS_WAVES_PER_BLOCK - 1) / STATS_WAVES_PER_BLOCK);
}
int enqueue_sw_stats(fadehip_ctx *ctx, hipStream_t st, const StatsWork *d_work, const size_t cls_begin[6], const uint8_t *d_q,
                     const uint8_t *d_r, fadehip_sw_stats_result *d_out, void *scratch, int long_max_lr, int long_blocks, const StatsScoring &sc) {
    const dim3 blk(64 * STATS_WAVES_PER_BLOCK);
    for (int c = 0; c < 5; c++) {
        const size_t cnt = cls_begin[c + 1] - cls_begin[c];
        if (!cnt) continue;
        const StatsWork *wk = d_work + cls_begin[c];
        if (c == 4) {
            hipLaunchKernelGGL(sw_stats_kernel<STATS_STRIP_R>, dim3((unsigned)long_blocks), blk, 0, st, wk, (int32_t)cnt, d_q, d_r,
                               d_out, (int4 *)scratch, std::max(long_max_lr, 1), sc);
        } else {
            const unsigned g = (unsigned)std::min<size_t>((cnt + STATS_WAVES_PER_BLOCK - 1) / STATS_WAVES_PER_BLOCK, 16384);
            switch (c) {
            case 0: hipLaunchKernelGGL(sw_stats_kernel<1>, dim3(g), blk, 0, st, wk, (int32_t)cnt, d_q, d_r, d_out, (int4 *)nullptr, 0, sc); break;
            case 1: hipLaunchKernelGGL(sw_stats_kernel<2>, dim3(g), blk, 0, st, wk, (int32_t)cnt, d_q, d_r, d_out, (int4 *)nullptr, 0, sc); break;
            case 2: hipLaunchKernelGGL(sw_stats_kernel<4>, dim3(g), blk, 0, st, wk, (int32_t)cnt, d_q, d_r, d_out, (int4 *)nullptr, 0, sc); break;
            default: hipLaunchKernelGGL(sw_stats_kernel<8>, dim3(g), blk, 0, st, wk, (int32_t)cnt, d_q, d_r, d_out, (int4 *)nullptr, 0, sc); break;
            }
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace fadehip::host

extern "C" {

// ------------------------------------------------------------------------------- level 1
int fadehip_sw_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *q, const int64_t *q_off, const uint8_t *r,
                     const int64_t *r_off, fadehip_sw_result *out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!q || !q_off || !r || !r_off || !out))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Slot &s = ctx->slots[0];
    {
        const int erc = ensure_slot(ctx, s);
        if (erc) return erc;
    }
    if (s.state == 2) HIPCHK(ctx, hipStreamSynchronize(s.stream));
    const int64_t q_total = q_off[n], r_total = r_off[n];
    // class-partitioned work lists, built on the host from the offsets (no sequence is touched here)
    std::vector<Work> lists[NUM_LISTS];
    int max_lr[NUM_LISTS] = {0};
    int max_long_lq = 0;
    std::vector<int> degenerate;
    for (int k = 0; k < n; k++) {
        const int64_t lq = q_off[k + 1] - q_off[k], lr = r_off[k + 1] - r_off[k];
        if (lq < 0 || lr < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-decreasing (pair %d)", k);
        if (lq == 0 || lr == 0) { degenerate.push_back(k); continue; }
        const int cls = list_of_len((int)std::min<int64_t>(lq, 1 << 20), lr);
        if (cls < 0) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "query %d has %lld bases (max %d)", k, (long long)lq, FADEHIP_MAX_LONG_QUERY);
        if (cls == LONG_LIST) max_long_lq = std::max(max_long_lq, (int)lq);
        if (lr > ctx->prm.max_ref_len)
            return set_err(ctx, FADEHIP_E_UNSUPPORTED, "reference %d has %lld bases (max_ref_len %d)", k, (long long)lr, ctx->prm.max_ref_len);
        Work w;
        w.r_base = (uint64_t)r_off[k];
        w.q_base = (uint32_t)q_off[k];
        w.lq = (uint32_t)lq;
        w.lr = (uint32_t)lr;
        w.idx = (uint32_t)k;
        w.flags = 0;
        w.out = 0;
        lists[cls].push_back(w);
        max_lr[cls] = std::max(max_lr[cls], (int)lr);
    }
    if (q_total >= (int64_t)1 << 32) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "query bases per batch must stay below 2^32");
    DevBuf &d_q = ctx->l1_q, &d_r = ctx->l1_r, &d_qn = ctx->l1_qn, &d_rn = ctx->l1_rn, &d_bad = ctx->l1_bad,
           &d_work = ctx->l1_work, &d_aln = ctx->l1_aln;
    int rc = 0;
    hipStream_t st = s.stream;
    size_t n_work = 0;
    for (int c = 0; c < NUM_LISTS; c++) n_work += lists[c].size();
    if ((rc = reserve(ctx, d_q, (size_t)q_total + 2)) || (rc = reserve(ctx, d_r, (size_t)r_total + 2)) ||
        (rc = reserve(ctx, d_qn, (size_t)q_total / 2 + 8)) || (rc = reserve(ctx, d_rn, (size_t)r_total / 2 + 8)) ||
        (rc = reserve(ctx, d_bad, 4)) || (rc = reserve(ctx, d_aln, (size_t)n * sizeof(fadehip_aln))) ||
        (rc = reserve(ctx, d_work, std::max<size_t>(1, n_work) * sizeof(Work))) || (rc = reserve(ctx, s.zblock, 2 * Slot::ZB_STRIDE)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_q.p, q, (size_t)q_total, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_r.p, r, (size_t)r_total, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(d_bad.p, 0, 4, st));
    if (q_total > 0)
        hipLaunchKernelGGL(pack_ascii_kernel, dim3((unsigned)((q_total / 2 + 256) / 256)), dim3(256), 0, st,
                           (const uint8_t *)d_q.p, (uint64_t)q_total, (uint64_t)0, (uint8_t *)d_qn.p, 0, (int *)d_bad.p);
    if (r_total > 0)
        hipLaunchKernelGGL(pack_ascii_kernel, dim3((unsigned)((r_total / 2 + 256) / 256)), dim3(256), 0, st,
                           (const uint8_t *)d_r.p, (uint64_t)r_total, (uint64_t)0, (uint8_t *)d_rn.p, 0, (int *)d_bad.p);
    HIPCHK(ctx, hipGetLastError());
    {
        size_t base = 0;
        for (int c = 0; c < NUM_LISTS; c++) {
            if (lists[c].empty()) continue;
            for (size_t k = 0; k < lists[c].size(); k++) lists[c][k].out = (uint32_t)(base + k);  // one result array, list after list
            HIPCHK(ctx, hipMemcpyAsync((Work *)d_work.p + base, lists[c].data(), lists[c].size() * sizeof(Work), hipMemcpyHostToDevice, st));
            base += lists[c].size();
        }
    }
    const int64_t budget = ctx->prm.trace_bytes > 0 ? ctx->prm.trace_bytes : ((int64_t)4 << 30);
    {
        size_t base = 0;
        s.fwd_spans.clear();
        s.tb_spans.clear();
        s.tickets_used = 0;
        s.zoff = 0;  // (slot 0's first counter block, filled here: its level-2 runs start over)
        s.zb_next_clean = false;
        HIPCHK(ctx, hipMemsetAsync(s.zb(), 0, Slot::ZB_BYTES, st));
        for (int c = 0; c < NUM_CLASSES; c++) s.sel_fresh[c] = true;
        // level 1 wants a CIGAR for every pair: whatever the forced-diagonal shortcut leaves goes to pass 2, with snapshots
        s.use_ckpt = true;
        if (const char *kv = getenv("FADEHIP_CKPT")) s.use_ckpt = atoi(kv) != 0;
        s.early = false;  // (the results are read back below, behind everything)
        for (int c = 0; c < NUM_LISTS; c++) {
            if (lists[c].empty()) continue;
            // the lists come from the host here: their counts go where the gate leaves them at level 2
            hipLaunchKernelGGL(set_counts_kernel, dim3(1), dim3(1), 0, st, s.d_counters() + c, (uint32_t)lists[c].size());
            HIPCHK(ctx, hipGetLastError());
            ClassRun cr;  // no meta, no rs, no gate, untimed: the defaults
            cr.cls = c;
            cr.work = (const Work *)d_work.p + base;
            cr.n_bound = (int)lists[c].size();
            cr.count_dev = s.d_counters() + c;
            cr.max_lr = max_lr[c];
            cr.q_nib = (const uint8_t *)d_qn.p;
            cr.r_nib = (const uint8_t *)d_rn.p;
            cr.out = (fadehip_aln *)d_aln.p;
            cr.budget = budget;
            if (c == LONG_LIST) rc = run_long(ctx, s, st, cr, max_long_lq);
            else rc = ctx->two_pass ? run_class_two_pass(ctx, s, st, cr) : run_class_single(ctx, s, st, cr);
            if (rc) {
                (void)hipStreamSynchronize(st);
                return rc;
            }
            base += lists[c].size();
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    s.state = 0;  // slot 0's level-2 buffers were borrowed
    std::vector<fadehip_aln> h_aln(n_work);
    if (n_work) HIPCHK(ctx, hipMemcpy(h_aln.data(), d_aln.p, n_work * sizeof(fadehip_aln), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n_work; k++) out[h_aln[k].read_idx] = h_aln[k].sw;
    // empty query or reference: nothing to align (no DP): all of the query is soft-clipped
    for (int k : degenerate) {
        fadehip_sw_result o;
        memset(&o, 0, sizeof o);
        o.end_query = o.end_ref = -1;
        const int64_t lq = q_off[k + 1] - q_off[k];
        if (lq > 0 && (ctx->sc.rules & FADEHIP_RULE_PAD_SOFTCLIP)) {
            o.n_ops = 1;
            o.ops[0] = ((uint32_t)lq << 4) | 4u;
        }
        out[k] = o;
    }
    return 0;
}

// parasail's stats mode (sw_stats.hpp).  Pairs sorted by (lq, lr) so that neighbouring waves sweep alike; each sorted range
// of a row class is one launch; results go straight to the caller's order.
int fadehip_sw_stats_batch(fadehip_ctx *ctx, const int32_t scoring[4], int32_t n, const uint8_t *q, const int64_t *q_off,
                           const uint8_t *r, const int64_t *r_off, fadehip_sw_stats_result *out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!scoring || n < 0 || (n > 0 && (!q_off || !r_off || !out))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    const int32_t open = scoring[0], ext = scoring[1], match = scoring[2], mismatch = scoring[3];
    const int32_t SC_MAX = 32767;
    if (open < 1 || ext < 1 || match < 1 || mismatch > 0 || open > SC_MAX || ext > SC_MAX || match > SC_MAX || mismatch < -SC_MAX)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED,
                       "stats scoring open %d ext %d match %d mismatch %d outside open, ext, match in [1, %d], mismatch in [-%d, 0]",
                       open, ext, match, mismatch, SC_MAX, SC_MAX);
    if (n == 0) return 0;
    std::vector<uint64_t> keys((size_t)n);
    int64_t q_total = 0, r_total = 0;
    for (int k = 0; k < n; k++) {
        const int64_t lq = q_off[k + 1] - q_off[k], lr = r_off[k + 1] - r_off[k];
        if (q_off[k] < 0 || r_off[k] < 0 || lq < 0 || lr < 0)
            return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (pair %d)", k);
        if (lq > FADEHIP_MAX_LONG_QUERY || lr > FADEHIP_MAX_LONG_QUERY)
            return set_err(ctx, FADEHIP_E_UNSUPPORTED, "pair %d has %lld x %lld bases (max %d each)", k, (long long)lq,
                           (long long)lr, FADEHIP_MAX_LONG_QUERY);
        const uint64_t kq = (lq == 0 || lr == 0) ? 0 : (uint64_t)lq;  // empty pairs sort first (the one-row class)
        keys[(size_t)k] = (kq << 48) | ((uint64_t)lr << 32) | (uint32_t)k;
    }
    q_total = q_off[n];
    r_total = r_off[n];
    if ((q_total > 0 && !q) || (r_total > 0 && !r)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    std::sort(keys.begin(), keys.end());
    std::vector<StatsWork> wl((size_t)n);
    // row classes: R = 1, 2, 4, 8 rows per lane (one strip), then the multi-strip class
    const int cls_max_lq[5] = {64, 128, 256, 512, FADEHIP_MAX_LONG_QUERY};
    size_t cls_begin[6] = {0, 0, 0, 0, 0, 0};
    int long_max_lr = 0;
    {
        int c = 0;
        for (size_t s = 0; s < (size_t)n; s++) {
            const int k = (int)(uint32_t)keys[s];
            StatsWork &w = wl[s];
            w.q_base = (uint64_t)q_off[k];
            w.r_base = (uint64_t)r_off[k];
            w.lq = (int32_t)(q_off[k + 1] - q_off[k]);
            w.lr = (int32_t)(r_off[k + 1] - r_off[k]);
            w.idx = k;
            w.pad = 0;
            const int klq = (int)(keys[s] >> 48);
            while (klq > cls_max_lq[c]) cls_begin[++c] = s;
            if (c == 4) long_max_lr = std::max(long_max_lr, w.lr);
        }
        while (c < 5) cls_begin[++c] = (size_t)n;
    }
    std::lock_guard<std::mutex> lk(ctx->stats_mu);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->stats_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stats_stream, hipStreamNonBlocking));
    hipStream_t st = ctx->stats_stream;
    size_t row_bytes;
    const int long_blocks = sw_stats_long_blocks(cls_begin[5] - cls_begin[4], long_max_lr, &row_bytes);
    int rc = 0;
    if ((rc = reserve(ctx, ctx->st_q, (size_t)q_total + 1)) || (rc = reserve(ctx, ctx->st_r, (size_t)r_total + 1)) ||
        (rc = reserve(ctx, ctx->st_work, (size_t)n * sizeof(StatsWork))) ||
        (rc = reserve(ctx, ctx->st_out, (size_t)n * sizeof(fadehip_sw_stats_result))) ||
        (long_blocks && (rc = reserve(ctx, ctx->st_scratch, (size_t)long_blocks * STATS_WAVES_PER_BLOCK * row_bytes))))
        return rc;
    if (q_total) HIPCHK(ctx, hipMemcpyAsync(ctx->st_q.p, q, (size_t)q_total, hipMemcpyHostToDevice, st));
    if (r_total) HIPCHK(ctx, hipMemcpyAsync(ctx->st_r.p, r, (size_t)r_total, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_work.p, wl.data(), (size_t)n * sizeof(StatsWork), hipMemcpyHostToDevice, st));
    StatsScoring sc;
    sc.open = open;
    sc.ext = ext;
    sc.match = match;
    sc.mismatch = mismatch;
    sc.rules = ctx->sc.rules;
    fadehip_sw_stats_result *d_out = (fadehip_sw_stats_result *)ctx->st_out.p;
    if ((rc = enqueue_sw_stats(ctx, st, (const StatsWork *)ctx->st_work.p, cls_begin, (const uint8_t *)ctx->st_q.p, (const uint8_t *)ctx->st_r.p, d_out,
                               ctx->st_scratch.p, long_max_lr, long_blocks, sc)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(fadehip_sw_stats_result), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------- level 2
// What every genome upload starts with: the contigs' places in the packed genome (each on a 16-base boundary), the buffers,
// the genome cleared (pad bases are 0) and the two contig arrays on the device.  ctx->n_contigs is the caller's to set, last.
static int genome_begin(fadehip_ctx *ctx, int32_t n_contigs, const int64_t *lengths) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->h_contig_len.assign(lengths, lengths + n_contigs);
    ctx->h_contig_base.resize(n_contigs);
    uint64_t total = 0;
    for (int c = 0; c < n_contigs; c++) {
        if (lengths[c] < 0) return set_err(ctx, FADEHIP_E_INVALID, "contig %d has negative length", c);
        ctx->h_contig_base[c] = total;
        total += ((uint64_t)lengths[c] + 15) & ~(uint64_t)15;  // contigs start on 8-byte boundaries
    }
    int rc;
    if ((rc = reserve(ctx, ctx->genome, (size_t)(total / 2 + 16)))) return rc;
    if ((rc = reserve(ctx, ctx->contig_len, sizeof(int64_t) * n_contigs))) return rc;
    if ((rc = reserve(ctx, ctx->contig_base, sizeof(uint64_t) * n_contigs))) return rc;
    hipStream_t st = ctx->copy_stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->genome.p, 0, ctx->genome.cap, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->contig_len.p, lengths, sizeof(int64_t) * n_contigs, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->contig_base.p, ctx->h_contig_base.data(), sizeof(uint64_t) * n_contigs, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));  // (the two host arrays are pageable)
    return 0;
}

int fadehip_genome_upload(fadehip_ctx *ctx, int32_t n_contigs, const int64_t *lengths, const uint8_t *const *seqs) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n_contigs <= 0 || !lengths || !seqs) return set_err(ctx, FADEHIP_E_INVALID, "bad genome arguments");
    int rc;
    if ((rc = genome_begin(ctx, n_contigs, lengths))) return rc;
    hipStream_t st = ctx->copy_stream;
    const size_t CH = (size_t)64 << 20;  // staging chunk, even
    DevBuf stage, bad;
    if ((rc = reserve(ctx, stage, CH)) || (rc = reserve(ctx, bad, 4))) {
        release(stage);
        release(bad);
        return rc;
    }
    hipError_t e = hipMemsetAsync(bad.p, 0, 4, st);
    for (int c = 0; c < n_contigs && e == hipSuccess; c++) {
        for (int64_t off = 0; off < lengths[c] && e == hipSuccess; off += (int64_t)CH) {
            const size_t nb = (size_t)std::min<int64_t>((int64_t)CH, lengths[c] - off);
            e = hipMemcpyAsync(stage.p, seqs[c] + off, nb, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(pack_ascii_kernel, dim3((unsigned)((nb / 2 + 256) / 256)), dim3(256), 0, st,
                               (const uint8_t *)stage.p, (uint64_t)nb, ctx->h_contig_base[c] + (uint64_t)off,
                               (uint8_t *)ctx->genome.p, 1, (int *)bad.p);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(st);  // the staging chunk is reused
        }
    }
    int h_bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    release(stage);
    release(bad);
    if (e != hipSuccess) return set_err(ctx, FADEHIP_E_HIP, "genome upload failed: %s", hipGetErrorString(e));
    if (h_bad) return set_err(ctx, FADEHIP_E_RESIDUE, "FASTA contains '=' which is not a residue this encoding can represent");
    ctx->n_contigs = n_contigs;
    return 0;
}

// ---- fadehip_genome_upload_fasta: the FASTA file through its .fai index, packed on the device
namespace {

// bases of the entry whose byte lies in front of file position x (the byte of base b is offset + b / lb * lw + b % lb)
int64_t fai_bases_before(const fadehip_fai_entry &e, int64_t x) {
    if (e.length == 0 || x <= e.offset) return 0;
    const int64_t d = x - e.offset, full = d / e.line_width, rem = d % e.line_width;
    return std::min<int64_t>(full * e.line_bases + std::min<int64_t>(rem, e.line_bases), e.length);
}
// 16-base groups of the entry whose LAST byte lies in front of x: the groups the ranges in front of x own
int64_t fai_groups_before(const fadehip_fai_entry &e, int64_t x) {
    const int64_t nb = fai_bases_before(e, x);
    return nb >= e.length ? (e.length + FASTA_GROUP - 1) / FASTA_GROUP : nb / FASTA_GROUP;
}
int64_t fai_pos(const fadehip_fai_entry &e, int64_t b) { return e.offset + b / e.line_bases * e.line_width + b % e.line_bases; }

// read fd[off, off + n) into dst: one pread loop per thread, at most four threads (a few MB each at the least)
bool read_range(int fd, uint8_t *dst, size_t n, int64_t off) {
    const int nt = (int)std::max<size_t>(1, std::min<size_t>(4, n >> 22));
    std::vector<char> ok((size_t)nt, 1);
    auto part = [&](int k) {
        size_t a = n * (size_t)k / (size_t)nt;
        const size_t b = n * ((size_t)k + 1) / (size_t)nt;
        while (a < b) {
            const ssize_t r = pread(fd, dst + a, b - a, (off_t)(off + (int64_t)a));
            if (r <= 0) {
                if (r < 0 && errno == EINTR) continue;
                ok[(size_t)k] = 0;
                return;
            }
            a += (size_t)r;
        }
    };
    std::vector<std::thread> th;
    for (int k = 1; k < nt; k++) th.emplace_back(part, k);
    part(0);
    for (auto &t : th) t.join();
    return std::find(ok.begin(), ok.end(), (char)0) == ok.end();
}

struct FastaUpload {  // what one call holds, given back however it ends
    int fd = -1;
    PinBuf chunk[2], pieces[2], tick[2], hblocks[2];
    hipEvent_t copied[2] = {nullptr, nullptr};
    DevBuf stage, d_pieces, flags;
    DevBuf comp[2], blocks[2], status[2], ticket[2], inf[2];  // BGZF: per parity of the call
    ~FastaUpload() {
        if (fd >= 0) close(fd);
        for (int k = 0; k < 2; k++) {
            release(chunk[k]);
            release(pieces[k]);
            release(tick[k]);
            release(hblocks[k]);
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            release(comp[k]);
            release(blocks[k]);
            release(status[k]);
            release(ticket[k]);
            release(inf[k]);
        }
        release(stage);
        release(d_pieces);
        release(flags);
    }
};

// The pieces of the file range [w0, w1) (every group whose last byte lies in it), into `out`; *lo / *hi: the bytes they read.
uint64_t fasta_pieces(const fadehip_ctx *ctx, int32_t n, const fadehip_fai_entry *e, const std::vector<int64_t> &end, int64_t w0, int64_t w1,
                      FastaPiece *out, uint32_t *n_out, int64_t *lo, int64_t *hi) {
    uint64_t groups = 0;
    uint32_t np = 0;
    *lo = INT64_MAX;
    *hi = 0;
    for (int32_t c = 0; c < n; c++) {
        if (e[c].length == 0 || end[(size_t)c] <= w0 || e[c].offset >= w1) continue;
        const int64_t ga = fai_groups_before(e[c], w0), gb = fai_groups_before(e[c], w1);
        if (gb <= ga) continue;
        FastaPiece &p = out[np++];
        p.src = e[c].offset;  // (file position: the caller takes the staged range's origin off)
        p.out_byte = ctx->h_contig_base[(size_t)c] / 2;
        p.length = e[c].length;
        p.g0 = ga;
        p.first = groups;
        p.line_bases = e[c].line_bases;
        p.line_width = e[c].line_width;
        p.contig = c;
        p.pad = 0;
        groups += (uint64_t)(gb - ga);
        *lo = std::min(*lo, fai_pos(e[c], ga * FASTA_GROUP));
        *hi = std::max(*hi, fai_pos(e[c], std::min<int64_t>(gb * FASTA_GROUP, e[c].length) - 1) + 1);
    }
    *n_out = np;
    return groups;
}

int launch_pack_fasta(fadehip_ctx *ctx, hipStream_t st, const uint8_t *in, uint64_t in_bytes, const FastaPiece *d_pieces, uint32_t np, uint64_t groups,
                      int *d_flags) {
    const unsigned grid = (unsigned)std::min<uint64_t>((groups + 255) / 256, (uint64_t)std::max(ctx->cu_count, 1) * 16u);
    hipLaunchKernelGGL(pack_fasta_kernel, dim3(grid), dim3(256), 0, st, in, in_bytes, d_pieces, np, groups, (uint8_t *)ctx->genome.p, d_flags);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

}  // namespace

int fadehip_genome_upload_fasta(fadehip_ctx *ctx, const char *path, int32_t n_contigs, const fadehip_fai_entry *entries) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n_contigs <= 0 || !entries || !path) return set_err(ctx, FADEHIP_E_INVALID, "bad genome arguments");
    size_t CH = (size_t)64 << 20;
    if (const char *v = getenv("FADEHIP_FASTA_CHUNK")) {
        const long long w = atoll(v);
        if (w < 4096) return set_err(ctx, FADEHIP_E_INVALID, "FADEHIP_FASTA_CHUNK=%s: at least 4096 bytes", v);
        CH = (size_t)w;
    }
    FastaUpload u;
    u.fd = open(path, O_RDONLY | O_CLOEXEC);
    struct stat sb;
    if (u.fd < 0 || fstat(u.fd, &sb)) return set_err(ctx, FADEHIP_E_INVALID, "cannot open %s: %s", path, strerror(errno));
    const int64_t file_size = (int64_t)sb.st_size;
    uint8_t magic[18] = {0};
    const ssize_t n_magic = pread(u.fd, magic, sizeof magic, 0);
    const bool gz = n_magic >= 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (gz) {
        bool bc = false;
        if (n_magic == 18 && magic[2] == 8 && (magic[3] & 4)) {
            const size_t xlen = (size_t)magic[10] | ((size_t)magic[11] << 8);
            bc = xlen >= 6 && magic[12] == 'B' && magic[13] == 'C' && magic[14] == 2 && magic[15] == 0;
        }
        if (!bc) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "%s is gzip without BGZF framing (compress it with bgzip)", path);
    }
    // the index: what the kernel divides by and steps with, and where every entry ends (before anything is enqueued)
    std::vector<int64_t> lens((size_t)n_contigs), end((size_t)n_contigs, 0);
    int64_t slack = 0, max_end = 0, min_off = INT64_MAX;
    for (int32_t c = 0; c < n_contigs; c++) {
        const fadehip_fai_entry &e = entries[c];
        lens[(size_t)c] = e.length;
        if (e.length < 0) return set_err(ctx, FADEHIP_E_INVALID, "contig %d has negative length", c);
        if (e.length == 0) continue;
        if (e.offset < 0 || e.line_bases <= 0 || e.line_width < e.line_bases)
            return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: contig %d has offset %lld, %d bases in a line of %d bytes", c,
                           (long long)e.offset, e.line_bases, e.line_width);
        const __int128 last = (__int128)e.offset + (__int128)((e.length - 1) / e.line_bases) * e.line_width + (e.length - 1) % e.line_bases;
        if (!gz && last >= (__int128)file_size)
            return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: contig %d ends beyond the file's %lld bytes", c, (long long)file_size);
        if (last >= ((__int128)1 << 62)) return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: contig %d ends beyond any file", c);
        end[(size_t)c] = (int64_t)last + 1;
        max_end = std::max(max_end, end[(size_t)c]);
        min_off = std::min(min_off, e.offset);
        // a 16-base group crosses at most 1 + 14 / line_bases line ends: the bytes in front of its last one that it reaches back to
        const int64_t gaps = 1 + 14 / e.line_bases;
        slack = std::max<int64_t>(slack, FASTA_GROUP - 1 + gaps * (int64_t)(e.line_width - e.line_bases));
    }
    if (slack > (int64_t)CH / 2)
        return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: line ends of %lld bytes and more do not fit chunks of %zu", (long long)(slack / 15), CH);
    int rc;
    if ((rc = genome_begin(ctx, n_contigs, lens.data()))) return rc;
    hipStream_t st = ctx->copy_stream;
    if (max_end == 0) {  // nothing but empty contigs
        ctx->n_contigs = n_contigs;
        return 0;
    }
    const size_t PAD = ((size_t)slack + 63) & ~(size_t)63;  // bytes staged in front of a range
    if (!gz) CH = std::min(CH, (((size_t)(max_end - min_off) + 4095) & ~(size_t)4095));  // (a small file: small chunks)
    const size_t read_cap = gz ? std::max<size_t>(CH, 65536 + 1024) : CH + PAD;
    for (int k = 0; k < 2; k++) {
        if ((rc = reserve_pinned(ctx, u.chunk[k], read_cap)) || (rc = reserve_pinned(ctx, u.pieces[k], sizeof(FastaPiece) * (size_t)n_contigs)) ||
            (rc = reserve_pinned(ctx, u.tick[k], 64)))
            return rc;
        HIPCHK(ctx, hipEventCreateWithFlags(&u.copied[k], hipEventDisableTiming));
        memset(u.tick[k].p, 0, 64);
    }
    if ((rc = reserve(ctx, u.d_pieces, sizeof(FastaPiece) * (size_t)n_contigs)) || (rc = reserve(ctx, u.flags, 8))) return rc;
    if (!gz && (rc = reserve(ctx, u.stage, read_cap))) return rc;
    HIPCHK(ctx, hipMemsetAsync(u.flags.p, 0, 4, st));
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)((int *)u.flags.p + 1), INT_MAX, 1, st));
    int *d_flags = (int *)u.flags.p;
    uint32_t call = 0;  // chunks that went to the device so far
    if (!gz) {
        for (int64_t w0 = min_off / (int64_t)CH * (int64_t)CH; w0 < max_end;) {
            const int64_t w1 = w0 + (int64_t)CH;
            const int par = (int)(call & 1);
            if (call >= 2) HIPCHK(ctx, hipEventSynchronize(u.copied[par]));  // the chunk's previous bytes have left it
            FastaPiece *hp = (FastaPiece *)u.pieces[par].p;
            uint32_t np = 0;
            int64_t lo, hi;
            const uint64_t groups = fasta_pieces(ctx, n_contigs, entries, end, w0, w1, hp, &np, &lo, &hi);
            if (!groups) {  // a range no contig ends a group in: on to the next one that holds a contig's start
                int64_t next = INT64_MAX;
                for (int32_t c = 0; c < n_contigs; c++)
                    if (end[(size_t)c] > w1) next = std::min(next, std::max(entries[c].offset, w1));
                w0 = next == INT64_MAX ? w1 : std::max(w1, next / (int64_t)CH * (int64_t)CH);
                continue;
            }
            if (hi - lo > (int64_t)read_cap) return set_err(ctx, FADEHIP_E_STATE, "internal: a chunk of %lld bytes", (long long)(hi - lo));
            for (uint32_t k = 0; k < np; k++) hp[k].src -= lo;
            if (!read_range(u.fd, u.chunk[par].p, (size_t)(hi - lo), lo)) return set_err(ctx, FADEHIP_E_INVALID, "cannot read %s: %s", path, strerror(errno));
            HIPCHK(ctx, hipMemcpyAsync(u.stage.p, u.chunk[par].p, (size_t)(hi - lo), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(u.d_pieces.p, hp, sizeof(FastaPiece) * (size_t)np, hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipEventRecord(u.copied[par], st));
            if ((rc = launch_pack_fasta(ctx, st, (const uint8_t *)u.stage.p, (uint64_t)(hi - lo), (const FastaPiece *)u.d_pieces.p, np, groups, d_flags))) return rc;
            call++;
            w0 = w1;
        }
    } else {
        // BGZF: compressed bytes cut at member boundaries, inflated into a device buffer that keeps the PAD bytes in front of
        // the call's range (the end of the call before), the same kernel on the inflated bytes
        int64_t cpos = 0, u0 = 0;  // file position of the next member, uncompressed position of its first byte
        size_t n_prev = 0;         // inflated bytes of the call before
        std::vector<bgzf::InflateBlock> blocks;
        auto check_tick = [&](int par) -> int {  // (after a wait that covers the parity's last call)
            const uint32_t *t = (const uint32_t *)u.tick[par].p;
            if (!t[1]) return 0;
            const uint32_t nb = t[2];
            std::vector<uint32_t> stt(nb);
            HIPCHK(ctx, hipStreamSynchronize(st));
            HIPCHK(ctx, hipMemcpy(stt.data(), u.status[par].p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < nb; k++)
                if (stt[k]) return set_err(ctx, FADEHIP_E_INVALID, "%s: BGZF member %u of a chunk: %s (%u members failed)", path, k, inflate_error_name(stt[k]), t[1]);
            return set_err(ctx, FADEHIP_E_INVALID, "%s: %u BGZF members failed", path, t[1]);
        };
        while (cpos < file_size) {
            const int par = (int)(call & 1);
            if (call >= 2) {
                HIPCHK(ctx, hipEventSynchronize(u.copied[par]));
                if ((rc = check_tick(par))) return rc;
            }
            size_t want = std::min<size_t>(CH, (size_t)(file_size - cpos)), consumed = 0;
            uint64_t total = 0;
            std::string msg;
            for (;;) {
                if (!read_range(u.fd, u.chunk[par].p, want, cpos)) return set_err(ctx, FADEHIP_E_INVALID, "cannot read %s: %s", path, strerror(errno));
                blocks.clear();
                total = 0;
                if (!scan_bgzf_members(u.chunk[par].p, want, blocks, &consumed, &total, msg)) return set_err(ctx, FADEHIP_E_INVALID, "%s: %s", path, msg.c_str());
                if (consumed || want >= std::min<size_t>(65536 + 1024, (size_t)(file_size - cpos))) break;
                want = std::min<size_t>(65536 + 1024, (size_t)(file_size - cpos));  // (a member longer than a small chunk)
            }
            if (!consumed) return set_err(ctx, FADEHIP_E_INVALID, "%s ends inside a BGZF member (at byte %lld)", path, (long long)cpos);
            cpos += (int64_t)consumed;
            if (!total) continue;  // empty members only
            const uint32_t nb = (uint32_t)blocks.size();
            const int64_t u1 = u0 + (int64_t)total;
            FastaPiece *hp = (FastaPiece *)u.pieces[par].p;
            uint32_t np = 0;
            int64_t lo, hi;
            const uint64_t groups = fasta_pieces(ctx, n_contigs, entries, end, u0, u1, hp, &np, &lo, &hi);
            const int64_t origin = u0 - (int64_t)PAD;
            for (uint32_t k = 0; k < np; k++) hp[k].src -= origin;
            if ((rc = reserve(ctx, u.comp[par], consumed + 1024 + 16)) || (rc = reserve(ctx, u.blocks[par], sizeof(bgzf::InflateBlock) * (size_t)nb)) ||
                (rc = reserve(ctx, u.status[par], 4 * (size_t)nb)) || (rc = reserve(ctx, u.ticket[par], 64)) ||
                (rc = reserve_roomy(ctx, u.inf[par], PAD + (size_t)total + 64)) ||
                (rc = reserve_pinned(ctx, u.hblocks[par], sizeof(bgzf::InflateBlock) * (size_t)nb)))
                return rc;
            memcpy(u.hblocks[par].p, blocks.data(), sizeof(bgzf::InflateBlock) * (size_t)nb);
            HIPCHK(ctx, hipMemcpyAsync(u.comp[par].p, u.chunk[par].p, consumed, hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(u.blocks[par].p, u.hblocks[par].p, sizeof(bgzf::InflateBlock) * (size_t)nb, hipMemcpyHostToDevice, st));
            uint8_t *buf = (uint8_t *)u.inf[par].p;
            if (call == 0) HIPCHK(ctx, hipMemsetAsync(buf, 0, PAD, st));
            else HIPCHK(ctx, hipMemcpyAsync(buf, (const uint8_t *)u.inf[par ^ 1].p + n_prev, PAD, hipMemcpyDeviceToDevice, st));
            bgzf::InflateArgs a;
            a.comp = (const uint8_t *)u.comp[par].p;
            a.blocks = (const bgzf::InflateBlock *)u.blocks[par].p;
            a.n_blocks = nb;
            a.out = buf + PAD;
            a.out_shift = nullptr;
            a.status = (uint32_t *)u.status[par].p;
            a.ticket = (uint32_t *)u.ticket[par].p;
            a.check_crc = 1;
            if ((rc = launch_inflate(ctx, st, a))) return rc;
            ((uint32_t *)u.tick[par].p)[2] = nb;
            HIPCHK(ctx, hipMemcpyAsync(u.tick[par].p, u.ticket[par].p, 8, hipMemcpyDeviceToHost, st));
            if (groups) {
                HIPCHK(ctx, hipMemcpyAsync(u.d_pieces.p, hp, sizeof(FastaPiece) * (size_t)np, hipMemcpyHostToDevice, st));
                if ((rc = launch_pack_fasta(ctx, st, buf, (uint64_t)PAD + total, (const FastaPiece *)u.d_pieces.p, np, groups, d_flags))) return rc;
            }
            HIPCHK(ctx, hipEventRecord(u.copied[par], st));
            n_prev = (size_t)total;
            u0 = u1;
            call++;
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int par = 0; par < 2; par++)
            if ((rc = check_tick(par))) return rc;
        if (u0 < max_end) {
            for (int32_t c = 0; c < n_contigs; c++)
                if (end[(size_t)c] > u0)
                    return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: contig %d ends beyond the file's %lld uncompressed bytes", c, (long long)u0);
        }
    }
    int h_flags[2] = {0, INT_MAX};
    HIPCHK(ctx, hipMemcpyAsync(h_flags, u.flags.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (h_flags[1] != INT_MAX)
        return set_err(ctx, FADEHIP_E_INVALID, "index does not match the FASTA: contig %d has a line end, '>' or a control byte where the index puts a base", h_flags[1]);
    if (h_flags[0]) return set_err(ctx, FADEHIP_E_RESIDUE, "FASTA contains '=' which is not a residue this encoding can represent");
    ctx->n_contigs = n_contigs;
    return 0;
}

int fadehip_genome_fetch(fadehip_ctx *ctx, int32_t tid, int64_t start, int64_t n, uint8_t *out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (ctx->n_contigs == 0) return set_err(ctx, FADEHIP_E_STATE, "no genome has been uploaded");
    if (tid < 0 || tid >= ctx->n_contigs || (size_t)tid >= ctx->h_contig_len.size()) return set_err(ctx, FADEHIP_E_INVALID, "contig %d of %d", tid, ctx->n_contigs);
    const int64_t len = ctx->h_contig_len[(size_t)tid];
    if (start < 0 || n < 0 || start > len || n > len - start || (n && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "bases [%lld, %lld + %lld) are not inside contig %d of %lld bases", (long long)start, (long long)start, (long long)n, tid, (long long)len);
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t b0 = ctx->h_contig_base[(size_t)tid] + (uint64_t)start, first = b0 / 2, last = (b0 + (uint64_t)n - 1) / 2;
    std::vector<uint8_t> packed((size_t)(last - first + 1));
    HIPCHK(ctx, hipMemcpy(packed.data(), (const uint8_t *)ctx->genome.p + first, packed.size(), hipMemcpyDeviceToHost));
    static const char letters[] = "=ACMGRSVTWYHKDBN";
    for (int64_t k = 0; k < n; k++) {
        const uint64_t b = b0 + (uint64_t)k;
        const uint8_t v = packed[(size_t)(b / 2 - first)];
        out[k] = (uint8_t)letters[(b & 1) ? (v & 15) : (v >> 4)];
    }
    return 0;
}

int fadehip_annotate_upload(fadehip_ctx *ctx, int slot, const fadehip_read_batch *b) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!b || b->n_reads < 0 || b->n_skipped < 0 || b->ref_span_bound < 0) return set_err(ctx, FADEHIP_E_INVALID, "bad batch");
    if (b->n_reads > ctx->prm.max_batch_reads)
        return set_err(ctx, FADEHIP_E_INVALID, "batch of %d reads exceeds max_batch_reads %d", b->n_reads, ctx->prm.max_batch_reads);
    if (ctx->n_contigs == 0) return set_err(ctx, FADEHIP_E_STATE, "fadehip_genome_upload has not been called");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Slot &s = ctx->slots[slot];
    if ((rc = ensure_slot(ctx, s))) return rc;
    if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));  // (made on first use: the file path never uploads)
    // The batch goes to the input buffer the run in flight (if any) does not use, on the ctx's copy stream: upload never
    // waits for that run, and the run's results stay valid until the slot is RUN again.
    Slot::Pending &nx = s.next;
    if (nx.valid) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));  // an earlier upload that was never run: same buffer
    nx.valid = false;
    const int n = b->n_reads;
    nx.n_reads = n;
    nx.n_skipped = b->n_skipped;
    nx.buf = 1 - s.cur;
    memset(nx.hist, 0, sizeof nx.hist);
    nx.out_bound = 0;
    nx.wide.clear();
    nx.max_lq = 0;
    nx.l_seq_lo = 0;
    nx.l_seq_hi = INT32_MAX;
    nx.span_bound = b->ref_span_bound;
    nx.h_base = nullptr;
    if (n == 0) { nx.valid = true; return 0; }
    if (!b->tid || !b->pos || !b->flag || !b->has_sa || !b->l_seq || !b->cigar_off || !b->seq_off ||
        (b->cigar_off[n] && !b->cigar_ops) || (b->seq_off[n] && !b->seq_packed))
        return set_err(ctx, FADEHIP_E_INVALID, "batch has NULL arrays");
    const size_t n_cig = b->cigar_off[n], n_seq = b->seq_off[n];
    if ((uint64_t)n_seq * 2 >= ((uint64_t)1 << 32)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "packed sequence bytes per batch must stay below 2^31");
    // What the launches of the run are sized from: records that carry bases per read-length class, the longest read, the
    // longest cigar.alignedLength.  A caller that packed the block knows them (ABI 3: n_with_seq, l_seq_min / l_seq_max,
    // ref_span_bound) and upload then touches no record: the offsets the kernels index with are checked by the gate
    // kernel before it reads through them.  Otherwise one pass over the records finds them (and checks the offsets
    // here, as ABI 2 did).  The CIGARs are scanned when the caller gave no span bound, or one so long that a window may
    // exceed what the wave kernels stage (then the few reads concerned are remembered for plan_run).
    const bool hinted = b->n_with_seq > 0 && b->ref_span_bound > 0 && b->ref_span_bound <= WIDE_MIN_SPAN &&
                        b->l_seq_min > 0 && b->l_seq_max >= b->l_seq_min;
    uint32_t hist[NUM_LISTS] = {0};
    int max_lq = 0;
    int64_t span = b->ref_span_bound;
    nx.wide.clear();
    if (hinted) {
        if (b->n_with_seq > n) return set_err(ctx, FADEHIP_E_INVALID, "n_with_seq %d exceeds n_reads %d", b->n_with_seq, n);
        const int c_lo = list_of_len(std::min(b->l_seq_min, MAX_LONG_QUERY)), c_hi = list_of_len(std::min(b->l_seq_max, MAX_LONG_QUERY));
        for (int c = c_lo; c <= c_hi; c++) hist[c] = (uint32_t)b->n_with_seq;  // any of them may be of any length in between
        max_lq = std::min(b->l_seq_max, MAX_LONG_QUERY);
        nx.out_bound = (uint32_t)b->n_with_seq;
        // the row classes and the score kernels are chosen from these bounds: the gate fails the batch for a record with
        // bases outside them (an l_seq_max that is too small but in the same row class raises no list overflow)
        nx.l_seq_lo = b->l_seq_min;
        nx.l_seq_hi = b->l_seq_max;
    } else {
        const bool scan = b->ref_span_bound <= 0, scan_wide = scan || b->ref_span_bound > WIDE_MIN_SPAN;
        uint8_t cls_of[33];  // class of a read of 16 k - 15 .. 16 k bases
        for (int k = 0; k <= 32; k++) cls_of[k] = (uint8_t)list_of_len(std::max(16 * k, 1));
        uint32_t n_out = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t c0 = b->cigar_off[i], c1 = b->cigar_off[i + 1];
            const int lq = b->l_seq[i];
            if (c0 > c1 || c1 > n_cig || b->seq_off[i] > b->seq_off[i + 1] || b->seq_off[i + 1] > n_seq || lq < 0)
                return set_err(ctx, FADEHIP_E_INVALID, "record %d: cigar_off / seq_off must be non-decreasing and l_seq >= 0", i);
            if (b->seq_off[i + 1] == b->seq_off[i]) continue;  // no bases: the record cannot be re-aligned (anno.d:61 settled it)
            if (scan_wide) {
                if (b->flag[i] & 4u) continue;
                const CigarSummary cs = summarize_cigar(b->cigar_ops, c0, c1);
                if (cs.n_soft == 0) continue;
                if (scan) span = std::max(span, cs.aligned);
                if (cs.aligned > WIDE_MIN_SPAN) nx.wide.emplace_back(cs.aligned, lq);
            }
            const int c = lq > 512 ? (lq <= MAX_LONG_QUERY ? LONG_LIST : -1) : (int)cls_of[(std::max(lq, 1) + 15) >> 4];
            if (c >= 0) { hist[c]++; n_out++; }
            max_lq = std::max(max_lq, std::min(lq, MAX_LONG_QUERY));
        }
        nx.out_bound = n_out;
    }
    memcpy(nx.hist, hist, sizeof hist);
    nx.max_lq = max_lq;
    nx.span_bound = std::max<int64_t>(span, 1);
    const Layout L = batch_layout(n, (int64_t)n_cig, (int64_t)n_seq);
    const void *src[N_ARR] = {b->tid, b->pos, b->l_seq, b->cigar_off, b->seq_off, b->flag, b->has_sa, b->cigar_ops, b->seq_packed};
    const uint8_t *base = (const uint8_t *)b->tid;
    bool direct = ((uintptr_t)base & 255u) == 0;
    for (int k = 0; k < N_ARR && direct; k++)
        if (L.bytes[k] && (const uint8_t *)src[k] != base + L.off[k]) direct = false;
    if ((rc = reserve(ctx, s.in[nx.buf], L.total))) return rc;
    if (!direct) {
        // arrays from anywhere: gather them into the pinned staging block of this input buffer (one host copy) for the one DMA
        PinBuf &stage = s.stage[nx.buf];
        if ((rc = reserve_pinned(ctx, stage, L.total))) return rc;
        for (int k = 0; k < N_ARR; k++)
            if (L.bytes[k]) memcpy(stage.p + L.off[k], src[k], L.bytes[k]);
        base = stage.p;
    }
    nx.L = L;
    nx.h_base = base;
    HIPCHK(ctx, hipMemcpyAsync(s.in[nx.buf].p, base, L.off[N_ARR - 1] + L.bytes[N_ARR - 1], hipMemcpyHostToDevice, ctx->copy_stream));
    HIPCHK(ctx, hipEventRecord(s.ev_copied, ctx->copy_stream));
    nx.valid = true;
    return 0;
}

int fadehip_annotate_run(fadehip_ctx *ctx, int slot, int32_t floor_len, int32_t window) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!s.next.valid && !s.have_batch) return set_err(ctx, FADEHIP_E_STATE, "slot %d has no uploaded batch", slot);
    if (window < 0) return set_err(ctx, FADEHIP_E_INVALID, "window must be >= 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (s.state == 2) HIPCHK(ctx, hipStreamSynchronize(s.stream));  // results never fetched: the slot's buffers are still in use
    s.state = 0;
    if (s.next.valid) {
        // the batch uploaded last becomes the batch of this (and any repeated) run; its H2D is awaited on the device
        const Slot::Pending &nx = s.next;
        s.cur = nx.buf;
        s.L = nx.L;
        s.h_base = nx.h_base;
        memcpy(s.hist, nx.hist, sizeof s.hist);
        s.max_lq = nx.max_lq;
        s.l_seq_lo = nx.l_seq_lo;
        s.l_seq_hi = nx.l_seq_hi;
        s.span_bound = nx.span_bound;
        s.out_bound = nx.out_bound;
        s.wide = nx.wide;
        s.n_reads = nx.n_reads;
        s.n_skipped = nx.n_skipped;
        s.have_batch = true;
        s.device_only = false;
        s.wide_all = false;
        s.next.valid = false;
        if (s.n_reads) HIPCHK(ctx, hipStreamWaitEvent(s.stream, s.ev_copied, 0));
    }
    s.floor_len = floor_len;
    s.window = window;
    if (s.n_reads == 0) {
        s.ev_gate0 = s.ev_gate1 = s.ev_end = -1;
        memset(s.prof_counts, 0, sizeof s.prof_counts);
        s.state = 2;
        return 0;
    }
    if ((rc = plan_run(ctx, s))) return rc;
    if ((rc = enqueue_run(ctx, s))) {
        if (s.tail_stream) (void)hipStreamSynchronize(s.tail_stream);
        if (s.score_stream) (void)hipStreamSynchronize(s.score_stream);
        (void)hipStreamSynchronize(s.stream);
        s.state = 0;
        return rc;
    }
    s.state = 2;
    return 0;
}

int fadehip_annotate_submit(fadehip_ctx *ctx, int slot, const fadehip_read_batch *batch, int32_t floor_len, int32_t window) {
    int rc = fadehip_annotate_upload(ctx, slot, batch);
    if (rc) return rc;
    return fadehip_annotate_run(ctx, slot, floor_len, window);
}

int fadehip_annotate_results(fadehip_ctx *ctx, int slot, fadehip_anno_view *out) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "out is NULL");
    Slot &s = ctx->slots[slot];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = finish_run(ctx, s, slot))) return rc;
    out->rs = s.n_reads ? s.res.p : nullptr;
    out->aln = s.n_aln ? (const fadehip_aln *)(s.res.p + s.res_aln_off) : nullptr;
    out->n_reads = s.n_reads;
    out->n_aln = s.n_aln;
    memcpy(out->stats, s.stats, sizeof out->stats);
    out->n_oversize = s.n_oversize;
    out->reserved = 0;
    return 0;
}

int fadehip_annotate_collect(fadehip_ctx *ctx, int slot, fadehip_anno_out *out) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "out is NULL");
    Slot &s = ctx->slots[slot];
    if (s.state < 2) return set_err(ctx, FADEHIP_E_STATE, "slot %d has not been run", slot);
    out->n_aln = 0;
    out->n_oversize = 0;
    out->reserved = 0;
    memset(out->stats, 0, sizeof out->stats);
    if (s.n_reads > 0 && !out->rs) return set_err(ctx, FADEHIP_E_INVALID, "out->rs is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = finish_run(ctx, s, slot))) return rc;
    if (s.n_aln > 0 && (!out->aln || out->aln_cap < s.n_aln))
        return set_err(ctx, FADEHIP_E_INVALID, "out->aln holds %d entries, %d needed", out->aln ? out->aln_cap : 0, s.n_aln);
    if (s.n_reads) memcpy(out->rs, s.res.p, (size_t)s.n_reads);
    if (s.n_aln) memcpy(out->aln, s.res.p + s.res_aln_off, sizeof(fadehip_aln) * (size_t)s.n_aln);
    out->n_aln = s.n_aln;
    out->n_oversize = s.n_oversize;
    memcpy(out->stats, s.stats, sizeof out->stats);
    return 0;
}

int fadehip_last_run_profile(fadehip_ctx *ctx, int slot, float ms[4], int64_t counts[6]) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (s.state != 3) return set_err(ctx, FADEHIP_E_STATE, "slot %d has no collected run", slot);
    if (!ms || !counts) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    for (int k = 0; k < 6; k++) counts[k] = s.prof_counts[k];
    if (s.ev_end < 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(s.ev[s.ev_end]));
    float t = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&t, s.ev[s.ev_gate0], s.ev[s.ev_gate1]));
    ms[0] = t;
    for (auto &p : s.fwd_spans) {
        HIPCHK(ctx, hipEventElapsedTime(&t, s.ev[p.first], s.ev[p.second]));
        ms[1] += t;
    }
    for (auto &p : s.tb_spans) {
        HIPCHK(ctx, hipEventElapsedTime(&t, s.ev[p.first], s.ev[p.second]));
        ms[2] += t;
    }
    HIPCHK(ctx, hipEventElapsedTime(&t, s.ev[s.ev_gate0], s.ev[s.ev_end]));
    ms[3] = t;
    return 0;
}

}  // extern "C"
