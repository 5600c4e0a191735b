// fadehip.hip — C ABI (include/fadehip.h) over the gfx950 kernels in fadehip_kernels.hpp.
// Host side of the drop-in boundary for source/anno.d:44-50 / source/analysis.d:67.
// No CPU fallback lives here: every entry point either runs the HIP path or returns an error.
//
// Level 2 is an asynchronous pipeline: upload is one hipMemcpyAsync of a pinned batch block, run
// enqueues every kernel and the D2H of the results without reading anything back — launches are sized from host-side
// bounds, the real counts stay on the device, persistent waves draw the traced re-computation's work from a table a
// planning kernel builds — and results / collect waits for the slot.
#include "fadehip_kernels.hpp"
#include "bgzf_deflate.hpp"
#include "bgzf_inflate.hpp"
#include "bam_device.hpp"
#include "sw_stats.hpp"
#include <rccl/rccl.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace fadehip;

namespace {

thread_local std::string g_err = "";
thread_local const fadehip_ctx *g_err_ctx = nullptr;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};
struct PinBuf {  // staging memory (pin_alloc)
    uint8_t *p = nullptr;
    size_t cap = 0;
};

// Canonical layout of a batch block (fadehip_batch_bind): nine arrays, 256-byte aligned, in this order.
enum { A_TID, A_POS, A_LSEQ, A_CIGOFF, A_SEQOFF, A_FLAG, A_SA, A_CIG, A_SEQ, N_ARR };
struct Layout {
    size_t off[N_ARR], bytes[N_ARR], total;
};
Layout batch_layout(int64_t n, int64_t n_cig, int64_t n_seq) {
    Layout L;
    const size_t b[N_ARR] = {4 * (size_t)n, 4 * (size_t)n, 4 * (size_t)n, 4 * ((size_t)n + 1), 4 * ((size_t)n + 1),
                             2 * (size_t)n, (size_t)n,     4 * (size_t)n_cig, (size_t)n_seq};
    size_t at = 0;
    for (int k = 0; k < N_ARR; k++) {
        L.off[k] = at;
        L.bytes[k] = b[k];
        at += (b[k] + 8 + 255) & ~(size_t)255;  // + 8: the kernels read packed sequences as aligned dwords
    }
    L.total = at;
    return L;
}

// upload keeps the reads whose cigar.alignedLength exceeds this (spliced reads, large deletions) for plan_run
constexpr int64_t WIDE_MIN_SPAN = 1024;

struct Slot {
    hipStream_t stream = nullptr;
    // The score pass fills every wave slot it may use for ~0.8 ms; the small, latency-bound kernels of the other
    // slots (gate, selection, plan, pass 2, traceback) would wait behind it for a slot each.  So the score pass runs
    // on a stream whose CU mask leaves a few CUs (one per XCD by default) to everything else.
    hipStream_t score_stream = nullptr;
    std::vector<uint32_t> score_mask;  // its CU mask (empty: none)
    // The early order of a run (enqueue_run): the alignment array leaves for the host right behind the score pass, on the
    // score stream, while pass 2 and the gather of the entries it wrote (patch_gather_kernel) run on `stream`; the copy is
    // joined into `stream` before the small copies.  The A/B variants (ctx->early_tail) copy on `stream` and run pass 2 on
    // this stream instead, forked from the score pass's end and joined back; made when a run first takes that order.
    hipStream_t tail_stream = nullptr;
    bool tail_tried = false;
    bool early = false;        // the run in flight took the early order
    DevBuf patch;              // PatchHead | PatchEntry [patch_cap]
    PinBuf h_patch;            // its pinned copy: the head and the first patch_sent entries come with the run
    uint32_t patch_cap = 0, patch_sent = 0;
    // Two input buffers: while a run works on in[cur], the next batch is uploaded into in[1 - cur] on the copy stream
    // (fadehip_annotate_upload never waits for the run in flight, so H2D leaves the slot's critical path).
    DevBuf in[2];                    // device mirrors of a batch block
    int cur = 0;
    bool have_batch = false;         // a batch has been handed to run at least once (it can be run again)
    hipEvent_t ev_copied = nullptr;  // the H2D of the pending batch, recorded on the ctx's copy stream
    Layout L;                        // layout of the batch in flight
    PinBuf stage[2];                 // staging for batches that do not come as one canonical block (one per input buffer)
    const uint8_t *h_base = nullptr; // host block of the batch in flight (the caller's or `stage`)
    struct Pending {                 // the batch uploaded for the NEXT run
        bool valid = false;
        Layout L;
        const uint8_t *h_base = nullptr;
        uint32_t hist[NUM_LISTS] = {};
        int max_lq = 0;
        int l_seq_lo = 0, l_seq_hi = INT32_MAX;  // the caller's l_seq_min / l_seq_max (hinted upload), else no bound
        int64_t span_bound = 0;
        int n_reads = 0, n_skipped = 0;
        int buf = 0;
        uint32_t out_bound = 0;  // alignments the batch can produce at most (records that carry bases)
        // reads whose cigar.alignedLength alone is long (spliced reads, large deletions): (alignedLength, l_seq), so that
        // run can bound the long list for its window size without looking at the caller's arrays again
        std::vector<std::pair<int64_t, int>> wide;
        } next;
    DevBuf rs, fwd, aln, trace;
    DevBuf ckpt, cand;  // two-pass path
    // All small counters of a run live in one block so that one memset clears them and one copy brings them to the host.
    // Counters that different kernels (or different atomics of one kernel) hammer sit in different 128-byte lines:
    // same-line atomics serialise in one L2 channel (the gate kernel took 60 instead of 49 us with them packed).
    //   [0,128) gate counters | [128,512) counters64, one line each | [512 + 48 c, ...) selection counters of class c |
    //   [1024, 1536) stats: STAT_PARTS partial sums of the 8 stats.d counters | [1536, 2560) tickets of the persistent
    //   launches | [2560, ...) PlanOut
    // Two such blocks, used by alternate runs: a run zeroes the OTHER block behind the copy that ends it, so the next run's
    // gate follows its upload directly instead of a fill (zb_next_clean: that fill was enqueued and nothing has touched the
    // block since; otherwise the run fills its own block first, as every run once did).
    DevBuf zblock;
    size_t zoff = 0;             // the block of the run in flight: 0 or ZB_STRIDE
    bool zb_next_clean = false;
    static constexpr size_t ZB_COUNTERS = 0, ZB_C64 = 128, ZB_SEL = 512, ZB_SEL_STRIDE = 48, ZB_STATS = 1024,
                            ZB_TICKETS = 1024 + 8 * 8 * STAT_PARTS, N_TICKETS = 256, ZB_PLAN = ZB_TICKETS + 4 * N_TICKETS,
                            ZB_BYTES = ZB_PLAN + 128, ZB_STRIDE = (ZB_BYTES + 255) & ~(size_t)255;
    uint8_t *zb() const { return (uint8_t *)zblock.p + zoff; }
    unsigned long long *d_counters64() const { return (unsigned long long *)(zb() + ZB_C64); }
    unsigned long long *d_stats() const { return (unsigned long long *)(zb() + ZB_STATS); }
    uint32_t *d_counters() const { return (uint32_t *)(zb() + ZB_COUNTERS); }
    uint32_t *d_sel(int cls) const { return (uint32_t *)(zb() + ZB_SEL + ZB_SEL_STRIDE * (size_t)cls); }
    uint32_t *d_ticket(int k) const { return (uint32_t *)(zb() + ZB_TICKETS) + k; }
    PlanOut *d_plan() const { return (PlanOut *)(zb() + ZB_PLAN); }
    bool sel_fresh[NUM_CLASSES] = {};  // class's selection counters were cleared by the run's memset and not used yet
    int tickets_used = 0;
    DevBuf work[NUM_LISTS], meta[NUM_LISTS];
    DevBuf lrows;  // sw_long_kernel: previous-row H and F-hat
    uint8_t *h_zb = nullptr;  // pinned copy of zblock, filled by the D2H that ends a run
    const uint32_t *h_counters() const { return (const uint32_t *)(h_zb + ZB_COUNTERS); }
    const unsigned long long *h_counters64() const { return (const unsigned long long *)(h_zb + ZB_C64); }
    const unsigned long long *h_stats() const { return (const unsigned long long *)(h_zb + ZB_STATS); }
    const PlanOut *h_plan() const { return (const PlanOut *)(h_zb + ZB_PLAN); }
    PinBuf res;               // pinned result block: rs [n_reads] | aln [sum of the class bounds]
    size_t res_aln_off = 0;
    // host-side bounds of the batch in flight (what the launches are sized from)
    uint32_t bound[NUM_LISTS] = {};     // items per work list, at most
    uint32_t hist[NUM_LISTS] = {};      // upload: records per read-length class (gate-passing ones when the CIGARs were scanned)
    int64_t span_bound = 0;             // upload: max cigar.alignedLength (the caller's bound or the scan's)
    int max_lq = 0;                     // upload: longest read
    int l_seq_lo = 0, l_seq_hi = INT32_MAX;  // upload: l_seq range the caller announced (the gate fails records outside it)
    uint32_t out_bound = 0, out_cap = 0;  // upload: alignments at most; run: entries of the result array
    std::vector<std::pair<int64_t, int>> wide;
    bool use_ckpt = false;              // this run's score passes leave wave snapshots (see run_class_two_pass)
    bool device_only = false;           // the file path: rs and the alignments stay on the device (only the counter block comes back)
    bool wide_all = false;              // the file path: some read's alignedLength is long and which ones is not known on the host
    int wave_lr_bound = 0, long_max_lq = 0, long_max_lr = 0;
    int floor_len = 0, window = 0;
    int n_reads = 0, n_skipped = 0;
    int state = 0;  // 0 nothing run, 2 run enqueued, 3 results on the host
    int n_aln = 0, n_oversize = 0;
    int64_t stats[8] = {};
    std::vector<hipEvent_t> ev;  // event pool
    int ev_used = 0;
    // (start,end) event index pairs of the last run
    std::vector<std::pair<int, int>> fwd_spans, tb_spans;
    int ev_gate0 = -1, ev_gate1 = -1, ev_end = -1;
    int64_t prof_counts[6] = {0, 0, 0, 0, 0, 0};
    int64_t n_cand = 0, n_rerun = 0;  // two-pass: candidates traced / candidates re-run from further back
    int p2_last_octs[NUM_CLASSES];    // octets pass 2 served for this class in the slot's previous run (-1: none yet)
    int64_t last_cand = 0, last_aln = 0;  // previous run of this slot: candidates traced by pass 2 / alignments
    std::vector<void *> trash;        // scratch buffers outgrown while a run was being enqueued (freed after the slot's sync)
};

// One BGZF compression in flight (fadehip_bgzf_deflate_submit / _wait): its own stream, so that the copies of one lane
// run beside the kernels of the other.
struct BgzfLane {
    hipStream_t stream = nullptr;
    DevBuf src, slots, meta, member_off;  // meta: out_size [n] | out_crc [n] | ticket | total (u64)
    PinBuf out;                   // the members, packed: the pack kernel writes them straight into pinned host memory
    uint8_t *h_out = nullptr;     // where the submission in flight packs to (out.p, or a buffer of the caller: the file path's ring)
    hipEvent_t done = nullptr;    // recorded behind the submission's last kernel
    uint64_t *h_total = nullptr;  // pinned
    size_t n_bytes = 0;
    uint32_t n_blocks = 0;
    int geom = 64;  // block geometry of the submission in flight (bgzf_deflate.hpp)
    int state = 0;  // 0 idle, 1 submitted
};

// The synchronous inflate entry (fadehip_bgzf_inflate): buffers kept between calls.
struct InflateLane {
    hipStream_t stream = nullptr;
    DevBuf comp, blocks, out, status, ticket;
    PinBuf h_status;
};

// fadehip_clip_batch, fadehip_extract_batch, fadehip_eject_batch and fadehip_tags_batch: one stream, made when the first of
// them is called, and one set of buffers (kept between calls, grow only); a call of any of them holds mu from its uploads to
// its last wait
struct BatchLane {
    std::mutex mu;
    hipStream_t stream = nullptr;
    DevBuf in, meta, work, out;  // the records | offsets, rs and the call's other arrays | sizes, or eject's group arrays | output bytes
};

}  // namespace

struct fadehip_ctx {
    int device = 0;
    fadehip_params prm;
    ScoreTab sc;
    std::string err;
    std::mutex err_mu;
    Slot slots[FADEHIP_NUM_SLOTS];
    // genome
    DevBuf genome, contig_len, contig_base;
    DevBuf l1_q, l1_r, l1_qn, l1_rn, l1_bad, l1_work, l1_aln;  // level 1 (fadehip_sw_batch): kept between calls, grow only
    // fadehip_sw_stats_batch: its own stream and buffers (kept between calls, grow only), so that it leaves the slots alone
    hipStream_t stats_stream = nullptr;
    DevBuf st_q, st_r, st_work, st_out, st_scratch;
    std::mutex stats_mu;
    BatchLane batch;  // the three record-batch entry points share it: they leave the slots and the stats lane alone, not each other
    int n_contigs = 0;
    std::vector<int64_t> h_contig_len;
    std::vector<uint64_t> h_contig_base;
    int cu_count = 0;
    // One copy stream for the uploads of every slot (they share the DMA engine anyway).  The device multiplexes streams
    // onto few hardware queues and streams that share one run in order: so streams are few and made when first used
    // (a slot that is never used has none), 2 N + 1 for N slots in use.
    hipStream_t copy_stream = nullptr;
    // FADEHIP_KERNEL = twopass (default) | pk (single-pass packed int16) | int32 (single-pass int32): A/B runs
    bool use_packed = true;
    bool two_pass = true;
    int tail_cus_per_xcd = 1;  // FADEHIP_TAIL_CUS: CUs per XCD the score pass leaves alone (0: no CU mask, one stream per slot)
    int score_g8 = 1;            // the score pass on eight-lane groups where the batch's reads fit them (g8_kernel; FADEHIP_SCORE_G8=0: sixteen-lane groups only; 2: the 152-row kernel at two waves per SIMD)
    bool blocking_sync = false;  // FADEHIP_BLOCKING_SYNC=1: waits for the device sleep
    int split_cus = 0;  // FADEHIP_BAM_SPLIT=j: the file path's record kernels get j CUs of every XCD, the compressor the others
    bool score_frame = true;     // the eight-lane score pass in the column-drift frame where the launch fits it (g8_kernel; FADEHIP_SCORE_FRAME=0: never)
    bool score_persist = false;  // FADEHIP_SCORE_PERSIST=1: the score pass as a persistent launch (A/B variant)
    int p2_waves_fixed = 0;    // FADEHIP_P2_WAVES: waves of the persistent pass-2 launch (0: adaptive, see run_class_two_pass)
    bool early_copy = true;    // FADEHIP_EARLY_COPY=0: no run takes the early order (enqueue_run)
    // FADEHIP_EARLY_TAIL: what runs beside what in the early order.  0 "score" (default): the copy rides on the slot's
    // score stream, idle once the score pass has ended, and pass 2 stays on the slot's stream: no stream is added.  1 "masked" /
    // 2 "plain" (A/B variants, both slower: DESIGN.md §6): the copy on the slot's stream, pass 2 on a tail stream of its
    // own, on the CUs the score mask leaves free / without a mask.
    int early_tail = 0;
    int patch_cap = 4096;      // FADEHIP_PATCH_CAP: entries of a slot's patch list (tests)
    int span_slack = 24;  // FADEHIP_SPAN_SLACK overrides (tests: -1 makes almost every path leave its range)
    bool debug = false;
    BgzfLane bgzf[FADEHIP_BGZF_LANES];
    InflateLane inf;
    bool bgzf_ready = false;           // the compressor's LDS size has been declared to the runtime
    int bgzf_geom_fixed = 0;           // FADEHIP_BGZF_GEOM: 32 / 64 (0: by the ratio of the previous call)
    double bgzf_last_ratio = 0;        // compressed / raw bytes of the ctx's previous compression
    std::map<uint64_t, int> resident;  // (class, mode, LDS bytes) -> waves of that kernel the device holds at once
    std::mutex resident_mu;
};

namespace {

int set_err(fadehip_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) {
        std::lock_guard<std::mutex> l(ctx->err_mu);
        ctx->err = buf;
    }
    g_err = buf;
    g_err_ctx = ctx;
    return code;
}

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return set_err(ctx, e_ == hipErrorOutOfMemory ? FADEHIP_E_NOMEM : FADEHIP_E_HIP,      \
                           "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int reserve(fadehip_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return 0;
    if (b.p) {
        HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = std::max<size_t>(bytes, 256);
    want = (want + 255) & ~(size_t)255;
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// Staging memory the device reaches over PCIe.  Large blocks are ordinary 2 MB-aligned host memory handed to
// hipHostRegister: measured on MI355X (bench/setup_costs.hip) 1.5 ms per 32 MB against 4-7 ms for hipHostMalloc, with the
// same 56 GB/s up and down and the same 53 GB/s for a kernel that stores into it; small ones come from hipHostMalloc.
// The registry says which way a pointer came.
constexpr size_t PIN_REGISTER_MIN = (size_t)1 << 20;
std::mutex g_pin_mu;
std::unordered_map<void *, bool> g_pin_registered;  // pointer -> the library owns the memory (free() it)

int pin_alloc(fadehip_ctx *ctx, size_t bytes, void **out) {
    *out = nullptr;
    if (bytes >= PIN_REGISTER_MIN && !getenv("FADEHIP_PIN_HOSTMALLOC")) {
        const size_t al = (size_t)1 << 21, n = (bytes + al - 1) & ~(al - 1);
        void *p = aligned_alloc(al, n);
        if (!p) return set_err(ctx, FADEHIP_E_NOMEM, "out of host memory (%zu bytes of staging memory)", n);
        void *dp = nullptr;
        if (hipHostRegister(p, n, hipHostRegisterDefault) == hipSuccess && hipHostGetDevicePointer(&dp, p, 0) == hipSuccess && dp == p) {
            std::lock_guard<std::mutex> l(g_pin_mu);
            g_pin_registered[p] = true;
            *out = p;
            return 0;
        }
        // (a stack where registered memory has another address on the device: the kernels are given host pointers)
        (void)hipGetLastError();
        (void)hipHostUnregister(p);
        (void)hipGetLastError();
        free(p);
    }
    HIPCHK(ctx, hipHostMalloc(out, bytes ? bytes : 1));
    return 0;
}

int pin_free(fadehip_ctx *ctx, void *p) {
    if (!p) return 0;
    bool registered = false, owned = false;
    {
        std::lock_guard<std::mutex> l(g_pin_mu);
        auto it = g_pin_registered.find(p);
        if (it != g_pin_registered.end()) {
            registered = true;
            owned = it->second;
            g_pin_registered.erase(it);
        }
    }
    if (!registered) {
        HIPCHK(ctx, hipHostFree(p));
        return 0;
    }
    const hipError_t e = hipHostUnregister(p);
    if (owned) free(p);
    if (e != hipSuccess) return set_err(ctx, FADEHIP_E_HIP, "hipHostUnregister failed: %s", hipGetErrorString(e));
    return 0;
}

int reserve_pinned(fadehip_ctx *ctx, PinBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return 0;
    int rc;
    if (b.p) {
        if ((rc = pin_free(ctx, b.p))) return rc;
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = std::max<size_t>(bytes + bytes / 8, 4096);  // some headroom: batches of a stream differ a little in size
    want = (want + 4095) & ~(size_t)4095;
    if ((rc = pin_alloc(ctx, want, (void **)&b.p))) return rc;
    b.cap = want;
    return 0;
}

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

// buffers of a stream whose sizes differ a little from call to call: a quarter of headroom, so that they settle
int reserve_roomy(fadehip_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return 0;
    return reserve(ctx, b, bytes + bytes / 4 + 4096);
}

void release(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}
void release(PinBuf &b) {
    if (b.p) (void)pin_free(nullptr, b.p);
    b.p = nullptr;
    b.cap = 0;
}

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

void fill_ascii_table(uint8_t t[256]) {
    memset(t, 0, 256);
    const char *s = "=ACMGRSVTWYHKDBN";
    for (int k = 1; k < 16; k++) {
        t[(unsigned char)s[k]] = (uint8_t)k;
        t[(unsigned char)(s[k] | 0x20)] = (uint8_t)k;  // analysis.d:63 upper-cases the window
    }
}

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
// the scoring and the kernel's rows); *framed says which was taken.
template <int R8>
const void *g8_pick(const fadehip_ctx *ctx, int steps, bool *framed) {
    const ScoreTab &sc = ctx->sc;
    *framed = ctx->score_frame && frame_fits(std::max(std::max(sc.match, sc.mismatch), 0), sc.open, sc.ext, 8 * R8, steps);
    return *framed ? (const void *)sw_pk_kernel<R8, 1, false, 8, false, 0, true> : (const void *)sw_pk_kernel<R8, 1, false, 8>;
}
const void *g8_kernel(const fadehip_ctx *ctx, int cls, int max_lq, int steps, bool *framed) {
    const int score_g8 = ctx->score_g8, rows16 = 16 * class_rows(cls);
    *framed = false;
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
    bool framed = false;  // (the plan's blocks of four steps cover every window of the class list: what sizes LDS bounds the drift)
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
            if (ctx->debug && o0 == 0) fprintf(stderr, "[fadehip] class of %d rows: score pass on eight-lane groups (longest read of the batch: %d), column-drift frame %s\n", 16 * class_rows(cls), s.max_lq, framed ? "on" : "off");
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
            pa.list = (PatchEntry *)((uint8_t *)s.patch.p + sizeof(PatchHead));
            pa.cap = s.patch_cap;
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
// of up to LONG_WAVE_MAX_WINDOW columns, under the default end-cell and gap-tie rules (the kernel's flags are those rules').
// n_bound / max_lq / max_lr are upper bounds, the live count stays on the device.
constexpr int LONG_WAVE_MAX_QUERY = 4096, LONG_WAVE_MAX_WINDOW = 65000;
int run_long_wave(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c, int max_lq) {
    const int n_items = c.n_bound, max_lr = c.max_lr;
    // rows per lane: the smallest of 12 / 16 / 24 / 32 / 48 / 64 that holds the list's longest read (64: 256 VGPRs + 220 AGPRs, one wave per SIMD)
    const int R = max_lq <= 768 ? 12 : max_lq <= 1024 ? 16 : max_lq <= 1536 ? 24 : max_lq <= 2048 ? 32 : max_lq <= 3072 ? 48 : 64;
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
// windows, the non-default end-cell / gap-tie rules: FADEHIP_LONG_THREAD=1 sends everything to it, for A/B runs).
int run_long(fadehip_ctx *ctx, Slot &s, hipStream_t st, const ClassRun &c, int max_lq) {
    const int n_items = c.n_bound, max_lr = c.max_lr;
    const uint32_t need_rules = FADEHIP_RULE_END_MIN_REF_THEN_QUERY | FADEHIP_RULE_GAP_TIE_EXTENDS;
    if (max_lq <= LONG_WAVE_MAX_QUERY && max_lr <= LONG_WAVE_MAX_WINDOW && (ctx->sc.rules & need_rules) == need_rules && !getenv("FADEHIP_LONG_THREAD"))
        return run_long_wave(ctx, s, st, c, max_lq);
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
            const size_t bytes = sizeof(PatchHead) + sizeof(PatchEntry) * (size_t)std::max<uint32_t>(s.patch_cap, 1);
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
    hipLaunchKernelGGL(gate_kernel, dim3((n + GATE_BLOCK - 1) / GATE_BLOCK), dim3(GATE_BLOCK), 0, st, g);
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
    // results to the slot's pinned block; the counter block tells the host how many entries of each list are live
    HIPCHK(ctx, hipMemcpyAsync(s.h_zb, s.zb(), Slot::ZB_BYTES, hipMemcpyDeviceToHost, st));
    // the next run's counters, zeroed here, off its critical path (the same batch run again takes them as well)
    HIPCHK(ctx, hipMemsetAsync((uint8_t *)s.zblock.p + (s.zoff ^ Slot::ZB_STRIDE), 0, Slot::ZB_BYTES, st));
    s.zb_next_clean = true;
    if (s.device_only) return 0;
    HIPCHK(ctx, hipMemcpyAsync(s.res.p, s.rs.p, (size_t)n, hipMemcpyDeviceToHost, st));  // (pass 2 sets bits in rs: it stays behind it)
    if (s.early)  // the array left behind the score pass: what pass 2 wrote since comes as the patch list
        HIPCHK(ctx, hipMemcpyAsync(s.h_patch.p, s.patch.p, sizeof(PatchHead) + sizeof(PatchEntry) * (size_t)s.patch_sent, hipMemcpyDeviceToHost, st));
    else if (total_bound)
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
        const PatchEntry *const list = (const PatchEntry *)(s.h_patch.p + sizeof(PatchHead));
        uint8_t *const h_aln = s.res.p + s.res_aln_off;
        if (head.overflow || head.n > s.patch_cap) {
            // more candidates than the list holds: the whole array again (rare; the slot's next run is late, see last_cand)
            HIPCHK(ctx, hipMemcpyAsync(h_aln, s.aln.p, sizeof(fadehip_aln) * (size_t)s.out_cap, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
        } else {
            if (head.n > s.patch_sent) {  // more than the run's copy was sized for: the rest of the list
                HIPCHK(ctx, hipMemcpyAsync((void *)(list + s.patch_sent), (const uint8_t *)s.patch.p + sizeof(PatchHead) + sizeof(PatchEntry) * (size_t)s.patch_sent,
                                           sizeof(PatchEntry) * (size_t)(head.n - s.patch_sent), hipMemcpyDeviceToHost, st));
                HIPCHK(ctx, hipStreamSynchronize(st));
            }
            for (uint32_t k = 0; k < head.n; k++)
                if (list[k].out < s.out_cap) memcpy(h_aln + sizeof(fadehip_aln) * (size_t)list[k].out, &list[k].e, sizeof(fadehip_aln));
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


// The BGZF members of p[0, n): where each one's DEFLATE stream lies, its ISIZE and CRC32 (SAM spec 4.1: gzip member with
// FEXTRA and the subfield 'B','C' holding BSIZE = member size - 1).  Stops in front of a member that is not whole
// (*consumed = bytes of whole members); false + msg for bytes that are not a BGZF member.
bool scan_bgzf_members(const uint8_t *p, size_t n, std::vector<bgzf::InflateBlock> &blocks, size_t *consumed, uint64_t *total_out, std::string &msg) {
    size_t at = 0;
    uint64_t out = *total_out;
    while (n - at >= 18) {
        const uint8_t *m = p + at;
        if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || !(m[3] & 4)) {
            msg = "not a BGZF member at byte " + std::to_string(at) + " (gzip magic / FEXTRA missing)";
            return false;
        }
        const size_t xlen = (size_t)m[10] | ((size_t)m[11] << 8);
        if (n - at < 12 + xlen) break;
        size_t bsize = 0;
        for (size_t x = 12; x + 4 <= 12 + xlen;) {
            const size_t slen = (size_t)m[x + 2] | ((size_t)m[x + 3] << 8);
            if (m[x] == 'B' && m[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = ((size_t)m[x + 4] | ((size_t)m[x + 5] << 8)) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 2 + 8) {
            msg = "BGZF member at byte " + std::to_string(at) + " has no BC subfield or an impossible BSIZE";
            return false;
        }
        if (n - at < bsize) break;
        bgzf::InflateBlock b;
        b.src_off = at + 12 + xlen;
        b.src_len = (uint32_t)(bsize - 12 - xlen - 8);
        memcpy(&b.crc, m + bsize - 8, 4);
        memcpy(&b.isize, m + bsize - 4, 4);
        b.dst_off = out;
        b.pad = 0;
        if (b.isize > 65536u) {
            msg = "BGZF member at byte " + std::to_string(at) + " claims ISIZE " + std::to_string(b.isize) + " (at most 65536)";
            return false;
        }
        out += b.isize;
        blocks.push_back(b);
        at += bsize;
    }
    *consumed = at;
    *total_out = out;
    return true;
}

const char *inflate_error_name(uint32_t e) {
    static const char *const nm[] = {"ok", "reserved block type", "stored block LEN/NLEN mismatch", "bad dynamic-Huffman header", "invalid code",
                                     "distance beyond the block's start", "more bytes than ISIZE", "stream runs past the member's end",
                                     "fewer bytes than ISIZE", "CRC32 mismatch"};
    return e < sizeof nm / sizeof nm[0] ? nm[e] : "unknown";
}

// the inflate launch: as many waves as the device holds, each drawing members from the ticket
int launch_inflate(fadehip_ctx *ctx, hipStream_t st, const bgzf::InflateArgs &a) {
    HIPCHK(ctx, hipMemsetAsync(a.ticket, 0, 8, st));
    const unsigned wgs = (a.n_blocks + bgzf::INF_WAVES - 1) / bgzf::INF_WAVES;
    const unsigned grid = std::max(1u, std::min<unsigned>(wgs, (unsigned)std::max(ctx->cu_count, 1) * 8u));
    hipLaunchKernelGGL(bgzf::bgzf_inflate_kernel, dim3(grid), dim3(bgzf::INF_WG), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// ---- the record-batch entry points: fadehip_clip_batch, fadehip_extract_batch, fadehip_eject_batch on ctx->batch
// What their kernels dereference through, checked on the host record by record: block_size against the offsets and the name
// against block_size; with `fields`, n_cigar_op and l_seq as well.  extra(k) is what the caller alone checks of record k.
template <class Extra>
int check_records(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, bool fields, Extra extra) {
    for (int32_t k = 0; k < n; k++) {
        const int64_t len = rec_off[k + 1] - rec_off[k];
        if (len < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record %d)", k);
        const uint8_t *p = recs + rec_off[k];
        uint32_t bs = 0, ncig = 0;
        int32_t lseq = 0;
        if (len >= 36) {
            memcpy(&bs, p, 4);
            memcpy(&lseq, p + 20, 4);
            ncig = (uint32_t)p[16] | ((uint32_t)p[17] << 8);
        }
        const bool whole = len >= 36 && len <= ((int64_t)1 << 29) && (int64_t)bs + 4 == len && p[12] != 0;
        const bool name_fits = whole && 36 + (int64_t)p[12] <= len;
        const bool fields_fit = whole && lseq >= 0 && 36ull + p[12] + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq <= (uint64_t)len;
        if (fields && !fields_fit)
            return set_err(ctx, FADEHIP_E_INVALID, "record %d is malformed (block_size, l_read_name, n_cigar_op and l_seq must fit its %lld bytes)", k, (long long)len);
        if (!fields && !name_fits)
            return set_err(ctx, FADEHIP_E_INVALID, "record %d is malformed (block_size and l_read_name must fit its %lld bytes)", k, (long long)len);
        if (const int rc = extra(k)) return rc;
    }
    return 0;
}

// The lane made ready for a call (whose caller holds its lock): stream, buffers, and on the device the records, their offsets
// from record 0 (`off`, u64 [n + 1], at the start of meta) and rs at meta + m_rs; what lies between is the caller's, copied behind.
int batch_upload(fadehip_ctx *ctx, BatchLane &L, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                 size_t m_rs, size_t meta_bytes, size_t work_bytes, std::vector<uint64_t> &off) {
    const size_t in_bytes = (size_t)(rec_off[n] - rec_off[0]);
    off.resize((size_t)n + 1);
    for (int32_t k = 0; k <= n; k++) off[(size_t)k] = (uint64_t)(rec_off[k] - rec_off[0]);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!L.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    int rc;
    if ((rc = reserve(ctx, L.in, in_bytes + 8)) || (rc = reserve(ctx, L.meta, meta_bytes)) || (rc = reserve(ctx, L.work, work_bytes))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(L.in.p, recs + rec_off[0], in_bytes, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(L.meta.p, off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, L.stream));
    if (rs) HIPCHK(ctx, hipMemcpyAsync((uint8_t *)L.meta.p + m_rs, rs, (size_t)n, hipMemcpyHostToDevice, L.stream));  // (fadehip_tags_batch brings none: it makes them)
    return 0;
}

// Clip and extract behind their uploads: size kernel (a thread per element), the sizes to the host and summed there into
// off [cnt + 1], the out_cap check, the output reserved, the offsets up to a.out_off, write kernel (sixteen lanes per element),
// the bytes to `out`.  out_off gets the offsets — with off_first also when out is too small (clip says what it would have
// taken; extract does not).  No bytes: no second half (extract's rule; clip never gets there, a record leaves with >= 36).
template <class Args>
int size_then_write(fadehip_ctx *ctx, BatchLane &L, Args &a, size_t cnt, void (*size_kernel)(Args), void (*write_kernel)(Args),
                    const char *what, bool off_first, std::vector<uint64_t> &off, uint8_t *out, int64_t out_cap, int64_t *out_off) {
    hipStream_t st = L.stream;
    a.out_size = (uint32_t *)L.work.p;
    a.out = nullptr;
    hipLaunchKernelGGL(size_kernel, dim3(((unsigned)cnt + 255u) / 256u), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    std::vector<uint32_t> sizes(cnt);
    HIPCHK(ctx, hipMemcpyAsync(sizes.data(), a.out_size, 4 * cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    uint64_t run = 0;
    for (size_t q = 0; q < cnt; q++) {
        off[q] = run;
        run += sizes[q];
    }
    off[cnt] = run;
    const size_t out_bytes = (size_t)run;
    const bool fits = (int64_t)out_bytes <= out_cap;
    if (fits || off_first)
        for (size_t q = 0; q <= cnt; q++) out_off[q] = (int64_t)off[q];
    if (!fits) return set_err(ctx, FADEHIP_E_INVALID, "the %s records take %lld bytes, out holds %lld", what, (long long)out_bytes, (long long)out_cap);
    if (!out_bytes) return 0;
    if (const int rc = reserve(ctx, L.out, out_bytes + 8)) return rc;
    HIPCHK(ctx, hipMemcpyAsync((void *)a.out_off, off.data(), 8 * (cnt + 1), hipMemcpyHostToDevice, st));
    a.out = (uint8_t *)L.out.p;
    hipLaunchKernelGGL(write_kernel, dim3(((unsigned)cnt + 15u) / 16u), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, a.out, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The eject kernels on a stream, for fadehip_eject_batch and the file path: with `grouped` the groups' marks cleared, every
// record's group start, the blocks' carries and the marks; then the decision, applied.
int enqueue_eject(fadehip_ctx *ctx, hipStream_t st, bam::EjectArgs &a, uint32_t ntb, bool grouped) {
    if (grouped) {
        HIPCHK(ctx, hipMemsetAsync(a.grp, 0, 4 * (size_t)a.n, st));
        hipLaunchKernelGGL(bam::bam_eject_head_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, st, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_eject_scan_kernel, dim3(1), dim3(1024), 0, st, a, ntb);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_eject_mark_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, st, a);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(bam::bam_eject_apply_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, st, a, grouped ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void fadehip_params_default(fadehip_params *p) {
    if (!p) return;
    p->open = 10;
    p->ext = 2;
    p->match = 2;
    p->mismatch = -3;
    p->max_ref_len = 1 << 20;
    p->max_batch_reads = 1 << 20;
    p->trace_bytes = 0;
    p->trace_all = 0;
    p->rules = FADEHIP_RULES_DEFAULT;
}

int fadehip_abi_version(void) { return FADEHIP_ABI_VERSION; }

const char *fadehip_last_error(const fadehip_ctx *ctx) {
    if (!ctx || g_err_ctx == ctx) return g_err.c_str();
    thread_local std::string copy;
    {
        std::lock_guard<std::mutex> l(const_cast<fadehip_ctx *>(ctx)->err_mu);
        copy = ctx->err;
    }
    return copy.c_str();
}

int fadehip_create(fadehip_ctx **out, int device, const fadehip_params *params) {
    if (!out) return set_err(nullptr, FADEHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return set_err(nullptr, FADEHIP_E_NODEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n_dev) return set_err(nullptr, FADEHIP_E_NODEVICE, "device %d out of range (%d devices)", device, n_dev);
    fadehip_ctx *ctx = new (std::nothrow) fadehip_ctx();
    if (!ctx) return set_err(nullptr, FADEHIP_E_NOMEM, "out of host memory");
    ctx->device = device;
    fadehip_params_default(&ctx->prm);
    if (params) {
        ctx->prm = *params;
        if (ctx->prm.max_ref_len <= 0) ctx->prm.max_ref_len = 1 << 20;
        if (ctx->prm.max_batch_reads <= 0) ctx->prm.max_batch_reads = 1 << 20;
        if (ctx->prm.rules == 0) ctx->prm.rules = FADEHIP_RULES_DEFAULT;
    }
    int rc = 0;
    auto fail = [&](int code) {
        {
            std::lock_guard<std::mutex> l(ctx->err_mu);
            g_err = ctx->err;
        }
        g_err_ctx = nullptr;
        fadehip_destroy(ctx);
        return code;
    };
    if (ctx->prm.max_ref_len > (1 << 20)) {
        set_err(ctx, FADEHIP_E_UNSUPPORTED, "max_ref_len %d exceeds 2^20", ctx->prm.max_ref_len);
        return fail(FADEHIP_E_UNSUPPORTED);
    }
    if (ctx->prm.rules & ~(uint32_t)FADEHIP_RULES_DEFAULT) {
        set_err(ctx, FADEHIP_E_INVALID, "unknown rule bits 0x%x", ctx->prm.rules & ~(uint32_t)FADEHIP_RULES_DEFAULT);
        return fail(FADEHIP_E_INVALID);
    }
    if ((rc = build_score_tab(ctx, ctx->prm, ctx->sc))) return fail(rc);
    // FADEHIP_BLOCKING_SYNC=1 (the `fade` driver's file path sets it): a thread that waits for the device sleeps instead of
    // spinning.  A file-to-file run keeps every host core busy inflating; the two threads that wait for the front and the
    // back half of each call would otherwise burn a core each.  Not the default: a wake-up costs tens of microseconds,
    // which the level-2 pipeline (a result every millisecond) does not have to spare.
    if (const char *kv = getenv("FADEHIP_BLOCKING_SYNC")) {
        if (atoi(kv)) {
            ctx->blocking_sync = true;
            (void)hipSetDevice(device);
            if (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();  // (a device already in use keeps its flags)
        }
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
        set_err(ctx, FADEHIP_E_NODEVICE, "cannot open HIP device %d", device);
        return fail(FADEHIP_E_NODEVICE);
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(ctx, FADEHIP_E_NODEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
        return fail(FADEHIP_E_NODEVICE);
    }
    ctx->cu_count = prop.multiProcessorCount;
    if (const char *kv = getenv("FADEHIP_KERNEL")) {
        ctx->use_packed = strcmp(kv, "int32") != 0;
        ctx->two_pass = strcmp(kv, "twopass") == 0;
    }
    // Value ranges of the packed kernels at the longest query (512): the score pass keeps 16-bit keys of 32 * score
    // (per row pair and below the f16 infinity pattern 0x7c00: 64 * score for the row classes <= 14, i.e. scores <= 448,
    // 32 * score for 16 .. 24, i.e. scores <= 768), DP values are 8 * score in int16 compared as f16 patterns.  FADE's scoring (match 2) fits everything; larger match scores take the path
    // whose ranges still hold: the single-pass packed kernel (32-bit keys) up to match 7, the int32 kernel beyond.
    if (ctx->prm.match > 2) ctx->two_pass = false;
    if (8 * (ctx->prm.match * FADEHIP_MAX_QUERY + ctx->prm.open + std::max(ctx->prm.match, 0)) >= 0x7c00) ctx->use_packed = false;
    if (!ctx->two_pass && ctx->prm.rules != FADEHIP_RULES_DEFAULT) {
        set_err(ctx, FADEHIP_E_UNSUPPORTED, "the rule switches exist on the two-pass path only (match <= 2, FADEHIP_KERNEL unset)");
        return fail(FADEHIP_E_UNSUPPORTED);
    }
    if (const char *kv = getenv("FADEHIP_SPAN_SLACK")) ctx->span_slack = atoi(kv);
    if (const char *kv = getenv("FADEHIP_TAIL_CUS")) ctx->tail_cus_per_xcd = std::max(0, std::min(atoi(kv), 8));
    if (const char *kv = getenv("FADEHIP_BAM_SPLIT")) ctx->split_cus = std::max(0, std::min(atoi(kv), 31));
    if (const char *kv = getenv("FADEHIP_P2_WAVES")) ctx->p2_waves_fixed = std::max(0, atoi(kv));
    if (const char *kv = getenv("FADEHIP_SCORE_PERSIST")) ctx->score_persist = atoi(kv) != 0;
    if (const char *kv = getenv("FADEHIP_SCORE_G8")) ctx->score_g8 = atoi(kv);
    if (const char *kv = getenv("FADEHIP_SCORE_FRAME")) ctx->score_frame = atoi(kv) != 0;
    if (const char *kv = getenv("FADEHIP_EARLY_COPY")) ctx->early_copy = atoi(kv) != 0;
    if (const char *kv = getenv("FADEHIP_EARLY_TAIL")) ctx->early_tail = strcmp(kv, "masked") == 0 ? 1 : strcmp(kv, "plain") == 0 ? 2 : 0;
    if (const char *kv = getenv("FADEHIP_PATCH_CAP")) ctx->patch_cap = std::max(0, std::min(atoi(kv), 1 << 20));
    ctx->debug = getenv("FADEHIP_DEBUG") != nullptr;
    uint8_t table[256];
    fill_ascii_table(table);
    // (everything the library enqueues goes to streams of its own: the null stream would be one more HSA queue, i.e. one
    // more 173 MB context-save area in host memory, for two copies)
    if (hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMemcpyToSymbolAsync(HIP_SYMBOL(c_ascii_code), table, 256, 0, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
        hipStreamSynchronize(ctx->copy_stream) != hipSuccess) {
        set_err(ctx, FADEHIP_E_HIP, "hipMemcpyToSymbol failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(FADEHIP_E_HIP);
    }
    static_assert(sizeof(uint32_t) * (2 * NUM_LISTS + 4) <= Slot::ZB_C64 - Slot::ZB_COUNTERS, "gate counters overflow their slice");
    static_assert(Slot::ZB_SEL + Slot::ZB_SEL_STRIDE * NUM_CLASSES <= Slot::ZB_STATS, "selection counters overlap the stats");
    static_assert(sizeof(uint32_t) * NUM_BUCKETS <= Slot::ZB_SEL_STRIDE, "selection counters overflow their slice");
    static_assert(sizeof(PlanOut) <= 128, "PlanOut overflows its slice");
    for (int k = 0; k < FADEHIP_NUM_SLOTS; k++)
        for (int c = 0; c < NUM_CLASSES; c++) ctx->slots[k].p2_last_octs[c] = -1;
    *out = ctx;
    return 0;
}

void fadehip_destroy(fadehip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < FADEHIP_NUM_SLOTS; k++) {
        Slot &s = ctx->slots[k];
        for (DevBuf *b : {&s.in[0], &s.in[1], &s.rs, &s.fwd, &s.aln, &s.zblock, &s.trace, &s.ckpt, &s.cand, &s.lrows}) release(*b);
        for (void *q : s.trash) (void)hipFree(q);
        s.trash.clear();
        for (int c = 0; c < NUM_LISTS; c++) {
            release(s.work[c]);
            release(s.meta[c]);
        }
        release(s.stage[0]);
        release(s.stage[1]);
        release(s.res);
        release(s.patch);
        release(s.h_patch);
        if (s.tail_stream) (void)hipStreamDestroy(s.tail_stream);
        if (s.ev_copied) (void)hipEventDestroy(s.ev_copied);
        for (hipEvent_t e : s.ev) (void)hipEventDestroy(e);
        if (s.h_zb) (void)hipHostFree(s.h_zb);
        if (s.score_stream) (void)hipStreamDestroy(s.score_stream);
        if (s.stream && s.stream != ctx->copy_stream) (void)hipStreamDestroy(s.stream);
    }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (BgzfLane &l : ctx->bgzf) {
        for (DevBuf *b : {&l.src, &l.slots, &l.meta, &l.member_off}) release(*b);
        if (l.done) (void)hipEventDestroy(l.done);
        release(l.out);
        if (l.h_total) (void)hipHostFree(l.h_total);
        if (l.stream && (&l == &ctx->bgzf[0] || l.stream != ctx->bgzf[0].stream)) (void)hipStreamDestroy(l.stream);
    }
    for (DevBuf *b : {&ctx->inf.comp, &ctx->inf.blocks, &ctx->inf.out, &ctx->inf.status, &ctx->inf.ticket}) release(*b);
    release(ctx->inf.h_status);
    if (ctx->inf.stream) (void)hipStreamDestroy(ctx->inf.stream);
    release(ctx->genome);
    for (DevBuf *b : {&ctx->l1_q, &ctx->l1_r, &ctx->l1_qn, &ctx->l1_rn, &ctx->l1_bad, &ctx->l1_work, &ctx->l1_aln}) release(*b);
    for (DevBuf *b : {&ctx->st_q, &ctx->st_r, &ctx->st_work, &ctx->st_out, &ctx->st_scratch}) release(*b);
    if (ctx->stats_stream) (void)hipStreamDestroy(ctx->stats_stream);
    for (DevBuf *b : {&ctx->batch.in, &ctx->batch.meta, &ctx->batch.work, &ctx->batch.out}) release(*b);
    if (ctx->batch.stream) (void)hipStreamDestroy(ctx->batch.stream);
    release(ctx->contig_len);
    release(ctx->contig_base);
    if (g_err_ctx == ctx) g_err_ctx = nullptr;
    delete ctx;
}

int fadehip_host_alloc(fadehip_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return pin_alloc(ctx, bytes, out);
}

int fadehip_host_free(fadehip_ctx *ctx, void *p) {
    if (!p) return 0;
    return pin_free(ctx, p);
}

int fadehip_host_register(fadehip_ctx *ctx, void *p, size_t bytes) {
    if (!ctx || !p || !bytes) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostRegister(p, bytes, hipHostRegisterDefault));
    std::lock_guard<std::mutex> l(g_pin_mu);
    g_pin_registered[p] = false;  // (the caller's memory: fadehip_host_free only takes the registration back)
    return 0;
}

size_t fadehip_batch_bytes(int32_t n_reads, int64_t n_cigar_ops, int64_t n_seq_bytes) {
    if (n_reads < 0 || n_cigar_ops < 0 || n_seq_bytes < 0) return 0;
    return batch_layout(n_reads, n_cigar_ops, n_seq_bytes).total;
}

int fadehip_batch_bind(void *base, int32_t n_reads, int64_t n_cigar_ops, int64_t n_seq_bytes, fadehip_read_batch *b) {
    if (!base || !b || n_reads < 0 || n_cigar_ops < 0 || n_seq_bytes < 0) return set_err(nullptr, FADEHIP_E_INVALID, "bad batch_bind arguments");
    if ((uintptr_t)base & 255u) return set_err(nullptr, FADEHIP_E_INVALID, "a batch block must be 256-byte aligned (fadehip_host_alloc memory is)");
    const Layout L = batch_layout(n_reads, n_cigar_ops, n_seq_bytes);
    uint8_t *p = (uint8_t *)base;
    b->n_reads = n_reads;
    b->tid = (const int32_t *)(p + L.off[A_TID]);
    b->pos = (const int32_t *)(p + L.off[A_POS]);
    b->l_seq = (const int32_t *)(p + L.off[A_LSEQ]);
    b->cigar_off = (const uint32_t *)(p + L.off[A_CIGOFF]);
    b->seq_off = (const uint32_t *)(p + L.off[A_SEQOFF]);
    b->flag = (const uint16_t *)(p + L.off[A_FLAG]);
    b->has_sa = (const uint8_t *)(p + L.off[A_SA]);
    b->cigar_ops = (const uint32_t *)(p + L.off[A_CIG]);
    b->seq_packed = (const uint8_t *)(p + L.off[A_SEQ]);
    b->n_skipped = 0;
    b->ref_span_bound = 0;
    b->n_with_seq = 0;
    b->l_seq_min = b->l_seq_max = 0;
    b->reserved = 0;
    return 0;
}

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
    // multi-strip pairs: a scratch row of long_max_lr entries per wave, at most 256 MB of them
    const size_t row_bytes = (size_t)std::max(long_max_lr, 1) * 2 * sizeof(int4);
    const size_t n_long = cls_begin[5] - cls_begin[4];
    int long_blocks = 0;
    if (n_long) {
        const size_t waves = std::max<size_t>(1, std::min<size_t>({n_long, ((size_t)256 << 20) / row_bytes, (size_t)2048}));
        long_blocks = (int)((waves + STATS_WAVES_PER_BLOCK - 1) / STATS_WAVES_PER_BLOCK);
    }
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
    const StatsWork *d_work = (const StatsWork *)ctx->st_work.p;
    const uint8_t *d_q = (const uint8_t *)ctx->st_q.p, *d_r = (const uint8_t *)ctx->st_r.p;
    fadehip_sw_stats_result *d_out = (fadehip_sw_stats_result *)ctx->st_out.p;
    const dim3 blk(64 * STATS_WAVES_PER_BLOCK);
    for (int c = 0; c < 5; c++) {
        const size_t cnt = cls_begin[c + 1] - cls_begin[c];
        if (!cnt) continue;
        const StatsWork *wk = d_work + cls_begin[c];
        if (c == 4) {
            hipLaunchKernelGGL(sw_stats_kernel<STATS_STRIP_R>, dim3((unsigned)long_blocks), blk, 0, st, wk, (int32_t)cnt, d_q, d_r,
                               d_out, (int4 *)ctx->st_scratch.p, std::max(long_max_lr, 1), sc);
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
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(fadehip_sw_stats_result), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// filter.d:15-91 over records the caller brings: bam_device.hpp's clip_plan / clip_write_head, the functions of the file
// path under FADEHIP_BAM_CLIP, with the caller's rs and lengths in place of a run's results.
int fadehip_clip_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                       const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap, int64_t *out_off) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || !rec_off || !out_off || (n > 0 && (!recs || !rs || !trim_left || !trim_right)) || out_cap < 0 || (out_cap > 0 && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    out_off[0] = 0;
    if (n == 0) return 0;
    const auto trims = [&](int32_t k) { return trim_left[k] < 0 || trim_right[k] < 0 ? set_err(ctx, FADEHIP_E_INVALID, "record %d: negative trim length", k) : 0; };
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, trims))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | out_off [n + 1] u64 | trim_l [n] u32 | trim_r [n] u32 | rs [n] u8;  work: out_size [n] u32
    const size_t m_out = 8 * ((size_t)n + 1), m_tl = 2 * m_out, m_tr = m_tl + 4 * (size_t)n, m_rs = m_tr + 4 * (size_t)n;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_rs + (size_t)n + 8, 4 * (size_t)n, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tl, trim_left, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tr, trim_right, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    bam::ClipBatchArgs a;
    a.in = (const uint8_t *)L.in.p;
    a.in_off = (const uint64_t *)meta;
    a.rs = meta + m_rs;
    a.trim_l = (const uint32_t *)(meta + m_tl);
    a.trim_r = (const uint32_t *)(meta + m_tr);
    a.n = (uint32_t)n;
    a.out_off = (const uint64_t *)(meta + m_out);
    return size_then_write(ctx, L, a, (size_t)n, bam::clip_batch_size_kernel, bam::clip_batch_write_kernel, "clipped", true, off, out, out_cap, out_off);
}

// filter.d:209-265 over records the caller brings: bam_device.hpp's eject kernels, the ones of the file path under
// FADEHIP_BAM_EJECT / FADEHIP_BAM_EJECT_GROUPS, with the caller's rs in place of a run's results.
int fadehip_eject_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs, int grouped, uint8_t *keep) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || !rec_off || (n > 0 && (!recs || !rs || !keep))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, false, [](int32_t) { return 0; }))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    const uint32_t ntb = ((uint32_t)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    // meta: in_off [n + 1] u64 | rs [n] u8 | keep [n] u8;  work: head_of [n] u32 | grp [n] u32 | blk_head [ntb] | blk_carry [ntb]
    const size_t m_rs = 8 * ((size_t)n + 1), m_keep = m_rs + (size_t)n;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_keep + (size_t)n + 8, 8 * (size_t)n + 8 * (size_t)ntb, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    bam::EjectArgs a;
    memset(&a, 0, sizeof a);
    a.u = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.rs = meta + m_rs;
    a.keep = meta + m_keep;
    a.head_of = (uint32_t *)L.work.p;  // (the group arrays: looked at in grouped mode only)
    a.grp = a.head_of + (size_t)n;
    a.blk_head = a.grp + (size_t)n;
    a.blk_carry = a.blk_head + ntb;
    if ((rc = enqueue_eject(ctx, L.stream, a, ntb, grouped != 0))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(keep, a.keep, (size_t)n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    return 0;
}

// remap.d:11-87 over records the caller brings: bam_device.hpp's extract_write, the function of the file path under
// FADEHIP_BAM_EXTRACT, with the caller's rs, contigs, positions and CIGARs in place of a run's results.
int fadehip_extract_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                          const int32_t *art_tid, const int64_t *art_pos, const int64_t *cig_off, const uint32_t *cig,
                          uint8_t *out, int64_t out_cap, int64_t *out_off) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || n > (1 << 30) || !rec_off || !out_off || (n > 0 && (!recs || !rs || !art_tid || !art_pos || !cig_off)) || out_cap < 0 || (out_cap > 0 && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    out_off[0] = 0;
    if (n == 0) return 0;
    // beside what check_records checks: the CIGAR offsets of the sides that are built
    int64_t cig_end = 0;
    const auto cigars = [&](int32_t k) {
        for (int side = 0; side < 2; side++) {
            if (!(rs[k] & (2u << side))) continue;
            const int64_t c0 = cig_off[2 * (size_t)k + side], c1 = cig_off[2 * (size_t)k + side + 1];
            if (c0 < 0 || c1 < c0) return set_err(ctx, FADEHIP_E_INVALID, "record %d: the CIGAR offsets of its %s side must be non-negative and non-decreasing", k, side ? "right" : "left");
            if (c1 - c0 > 65535) return set_err(ctx, FADEHIP_E_INVALID, "record %d: a BAM record holds at most 65535 CIGAR ops", k);
            if (c1 > c0 && !cig) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
            cig_end = std::max(cig_end, c1);
        }
        return 0;
    };
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, cigars))) return rc;
    const size_t ns = 2 * (size_t)n;
    std::vector<uint64_t> off, soff(ns + 1);
    for (size_t q = 0; q <= ns; q++) soff[q] = (uint64_t)cig_off[q];  // (of a side that is not built: never read on the device)
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | cig_off [2n + 1] u64 | out_off [2n + 1] u64 | pos [2n] i64 | tid [2n] i32 | cig u32 | rs [n] u8;  work: out_size [2n] u32
    const size_t m_coff = 8 * ((size_t)n + 1), m_out = m_coff + 8 * (ns + 1), m_pos = m_out + 8 * (ns + 1), m_tid = m_pos + 8 * ns,
                 m_cig = m_tid + 4 * ns, m_rs = m_cig + 4 * (size_t)cig_end;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_rs + (size_t)n + 8, 4 * ns, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_coff, soff.data(), 8 * (ns + 1), hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_pos, art_pos, 8 * ns, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tid, art_tid, 4 * ns, hipMemcpyHostToDevice, L.stream));
    if (cig_end) HIPCHK(ctx, hipMemcpyAsync(meta + m_cig, cig, 4 * (size_t)cig_end, hipMemcpyHostToDevice, L.stream));
    bam::ExtractBatchArgs a;
    a.in = (const uint8_t *)L.in.p;
    a.in_off = (const uint64_t *)meta;
    a.rs = meta + m_rs;
    a.tid = (const int32_t *)(meta + m_tid);
    a.pos = (const int64_t *)(meta + m_pos);
    a.cig_off = (const uint64_t *)(meta + m_coff);
    a.cig = (const uint32_t *)(meta + m_cig);
    a.n = (uint32_t)n;
    a.out_off = (const uint64_t *)(meta + m_out);
    return size_then_write(ctx, L, a, ns, bam::extract_batch_size_kernel, bam::extract_batch_write_kernel, "extract", false, soff, out, out_cap, out_off);
}

// remap.d:31-50, filter.d:24-25,58-59,190-196 over records the caller brings: bam_device.hpp's read_tags and am_side fill
// the arrays the three calls above take.  Count per side, scan, write: a side's ops are as many as its text holds.
int fadehip_tags_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref, const char *const *ref_names,
                       uint8_t *rs, uint8_t *have, int32_t *trim_left, int32_t *trim_right, int32_t *art_tid, int64_t *art_pos,
                       int64_t *cig_off, uint32_t *cig, int64_t cig_cap) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || n > (1 << 30) || n_ref < 0 || (n_ref > 0 && !ref_names) || !rec_off || !cig_off ||
        (n > 0 && (!recs || !rs || !have || !trim_left || !trim_right || !art_tid || !art_pos)) || cig_cap < 0 || (cig_cap > 0 && !cig))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) {
        cig_off[0] = 0;
        return 0;
    }
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, [](int32_t) { return 0; }))) return rc;
    // the names back to back, and for every contig the first one of its name
    std::vector<uint32_t> noff((size_t)n_ref + 1, 0u);
    std::vector<int32_t> first((size_t)n_ref);
    std::string nbytes;
    {
        std::map<std::string, int32_t> seen;
        for (int32_t c = 0; c < n_ref; c++) {
            if (!ref_names[c]) return set_err(ctx, FADEHIP_E_INVALID, "ref_names[%d] is NULL", c);
            const std::string nm(ref_names[c]);
            if (nbytes.size() + nm.size() > 0x7fffffffu) return set_err(ctx, FADEHIP_E_INVALID, "the contig names take more than 2^31 bytes");
            first[(size_t)c] = seen.emplace(nm, c).first->second;
            nbytes += nm;
            noff[(size_t)c + 1] = (uint32_t)nbytes.size();
        }
    }
    const size_t ns = 2 * (size_t)n, ntb = ((size_t)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | cig_off [2n + 1] u64 | pos [2n] i64 | tid [2n] i32 | trim_l [n] i32 | trim_r [n] i32 |
    //       name_off [n_ref + 1] u32 | first [n_ref] i32 | rs [n] u8 | have [n] u8 | name bytes
    // work: blk_sums [ntb] u64 | blk_base [ntb] u64 | total u64 | bad u32, pad | cnt [2n] u32 | cig_at [2n] u32;  out: the ops
    const size_t m_coff = 8 * ((size_t)n + 1), m_pos = m_coff + 8 * (ns + 1), m_tid = m_pos + 8 * ns, m_tl = m_tid + 4 * ns,
                 m_tr = m_tl + 4 * (size_t)n, m_noff = m_tr + 4 * (size_t)n, m_first = m_noff + 4 * ((size_t)n_ref + 1),
                 m_rs = m_first + 4 * (size_t)n_ref, m_have = m_rs + (size_t)n, m_names = m_have + (size_t)n;
    const size_t w_base = 8 * ntb, w_tot = 16 * ntb, w_bad = w_tot + 8, w_cnt = w_bad + 8, w_at = w_cnt + 4 * ns;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, nullptr, m_rs, m_names + nbytes.size() + 8, w_at + 4 * ns, off))) return rc;
    hipStream_t st = L.stream;
    uint8_t *meta = (uint8_t *)L.meta.p, *work = (uint8_t *)L.work.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_noff, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, st));
    if (n_ref) HIPCHK(ctx, hipMemcpyAsync(meta + m_first, first.data(), 4 * (size_t)n_ref, hipMemcpyHostToDevice, st));
    if (!nbytes.empty()) HIPCHK(ctx, hipMemcpyAsync(meta + m_names, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(work + w_bad, 0xff, 8, st));
    bam::TagsArgs a;
    a.in = (const uint8_t *)L.in.p;
    a.in_off = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.names.bytes = meta + m_names;
    a.names.off = (const uint32_t *)(meta + m_noff);
    a.names.first = (const int32_t *)(meta + m_first);
    a.names.n_ref = n_ref;
    a.rs = meta + m_rs;
    a.have = meta + m_have;
    a.trim_l = (int32_t *)(meta + m_tl);
    a.trim_r = (int32_t *)(meta + m_tr);
    a.tid = (int32_t *)(meta + m_tid);
    a.pos = (int64_t *)(meta + m_pos);
    a.cnt = (uint32_t *)(work + w_cnt);
    a.cig_at = (uint32_t *)(work + w_at);
    a.blk_sums = (uint64_t *)work;
    a.blk_base = (uint64_t *)(work + w_base);
    a.total = (uint64_t *)(work + w_tot);
    a.bad = (uint32_t *)(work + w_bad);
    a.cig_off = (uint64_t *)(meta + m_coff);
    a.cig = nullptr;
    hipLaunchKernelGGL(bam::tags_count_kernel, dim3((unsigned)ntb), dim3(bam::TAG_BLOCK), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::tags_scan_kernel, dim3(1), dim3(1024), 0, st, a, (uint32_t)ntb);
    HIPCHK(ctx, hipGetLastError());
    uint64_t tot_bad[2] = {0, 0};  // total | bad (low word)
    HIPCHK(ctx, hipMemcpyAsync(tot_bad, a.total, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t bad = (uint32_t)tot_bad[1];
    if (bad != 0xffffffffu) return set_err(ctx, FADEHIP_E_INVALID, "record %u is malformed (its aux area is not whole fields)", bad);
    const uint64_t total = tot_bad[0];
    if (total > (uint64_t)cig_cap)
        return set_err(ctx, FADEHIP_E_INVALID, "the am tags hold %llu CIGAR ops, cig holds %lld", (unsigned long long)total, (long long)cig_cap);
    if ((rc = reserve(ctx, L.out, 4 * (size_t)total + 8))) return rc;
    a.cig = (uint32_t *)L.out.p;
    hipLaunchKernelGGL(bam::tags_write_kernel, dim3((unsigned)ntb), dim3(bam::TAG_BLOCK), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(rs, a.rs, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(have, a.have, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(trim_left, a.trim_l, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(trim_right, a.trim_r, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(art_tid, a.tid, 4 * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(art_pos, a.pos, 8 * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(cig_off, a.cig_off, 8 * (ns + 1), hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(ctx, hipMemcpyAsync(cig, a.cig, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
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

int fadehip_sync(fadehip_ctx *ctx) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    for (int k = 0; k < FADEHIP_NUM_SLOTS; k++)
        if (ctx->slots[k].stream) HIPCHK(ctx, hipStreamSynchronize(ctx->slots[k].stream));
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

// ------------------------------------------------------------------------------- BGZF compression
// the compressor's launches for n_bytes at d_src (device memory with 64 readable bytes behind the end) on the lane's stream
static int bgzf_lane_ready(fadehip_ctx *ctx, int lane, bool one_stream = false) {
    BgzfLane &l = ctx->bgzf[lane];
    if (!l.stream) {
        // (every stream is an HSA queue with a 173 MB context-save area to set up and to give back: FADEHIP_BGZF_ONE_STREAM=1
        // lets the lanes share one — their copies then no longer overlap each other's kernels; the file path's back half
        // uses the lanes one after the other anyway)
        if (lane > 0 && (one_stream || getenv("FADEHIP_BGZF_ONE_STREAM")) && ctx->bgzf[0].stream) l.stream = ctx->bgzf[0].stream;
        else if (ctx->split_cus > 0) l.stream = xcd_slice_stream(ctx, ctx->split_cus, ctx->cu_count / 8);
        else if (const char *kv = getenv("FADEHIP_BGZF_CUS")) l.stream = xcd_slice_stream(ctx, 0, std::max(1, std::min(atoi(kv), ctx->cu_count / 8)));  // the compressor alone on fewer CUs
        if (!l.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipHostMalloc((void **)&l.h_total, 64));
        HIPCHK(ctx, hipEventCreateWithFlags(&l.done, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    }
    if (!ctx->bgzf_ready) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)bgzf64::bgzf_deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bgzf64::LDS_BYTES));
        HIPCHK(ctx, hipFuncSetAttribute((const void *)bgzf32::bgzf_deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bgzf32::LDS_BYTES));
        ctx->bgzf_ready = true;
        if (const char *g = getenv("FADEHIP_BGZF_GEOM")) ctx->bgzf_geom_fixed = atoi(g) == 32 ? 32 : 64;  // (A/B runs; default: by the stream's ratio)
        if (getenv("FADEHIP_BGZF_PROF")) {
            int p64 = 0, p32 = 0;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&p64, (const void *)bgzf64::bgzf_deflate_kernel, bgzf64::WG, bgzf64::LDS_BYTES);
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&p32, (const void *)bgzf32::bgzf_deflate_kernel, bgzf32::WG, bgzf32::LDS_BYTES);
            fprintf(stderr, "[fadehip bgzf] compressor workgroups per CU: %d (0xff00-byte blocks, %d B of LDS), %d (0x7f00-byte blocks, %d B)\n", p64, bgzf64::LDS_BYTES, p32, bgzf32::LDS_BYTES);
        }
    }
    if (l.state == 1) HIPCHK(ctx, hipEventSynchronize(l.done));  // never waited for: its buffers are still in use
    l.state = 0;
    return 0;
}
// Which geometry (bgzf_deflate.hpp): small blocks, two per CU, while the stream is mostly incompressible (packed bases,
// uniform qualities: ratio above 0.45, where the smaller blocks cost 0.5 %); htslib's block size where it compresses well
// (runs of qualities: a member shrinks to a few KB and a second header per 64 KB would show).  From the ratio of the ctx's
// previous call; the first call takes the large blocks.
static int bgzf_pick_geom(const fadehip_ctx *ctx) {
    if (ctx->bgzf_geom_fixed) return ctx->bgzf_geom_fixed;
    return ctx->bgzf_last_ratio > 0.45 ? 32 : 64;
}
// The same choice for bytes the host can look at (fadehip_bgzf_deflate_submit): the share of bytes equal to their
// predecessor over 64 windows of 4 KB.  Packed bases and uniform qualities: a few per cent; qualities in runs: a third.
static int bgzf_pick_geom_host(const fadehip_ctx *ctx, const uint8_t *p, size_t n) {
    if (ctx->bgzf_geom_fixed) return ctx->bgzf_geom_fixed;
    const size_t win = 4096, nwin = 64;
    size_t eq = 0, seen = 0;
    for (size_t w = 0; w < nwin; w++) {
        const size_t lo = n > win ? (n - win) / nwin * w : 0, hi = std::min(n, lo + win);
        for (size_t k = lo + 1; k < hi; k++) eq += p[k] == p[k - 1];
        seen += hi > lo ? hi - lo - 1 : 0;
        if (n <= win) break;
    }
    return seen && (double)eq < 0.15 * (double)seen ? 32 : 64;
}
// (host_out: pinned memory the members are packed into — the lane's own buffer when NULL.  A member is at most its block's
// bytes + 5 (stored) + 26 of BGZF framing: the buffer is sized for that, the kernel writes through PCIe, and nothing but
// the 8-byte total has to be copied afterwards.)
static size_t bgzf_block_bytes(int geom) { return geom == 32 ? (size_t)bgzf32::BLOCK : (size_t)bgzf64::BLOCK; }
static size_t bgzf_out_cap(size_t n_bytes, int geom) {
    const size_t block = bgzf_block_bytes(geom);
    return n_bytes + ((n_bytes + block - 1) / block) * 32 + 64;
}
static int bgzf_enqueue(fadehip_ctx *ctx, int lane, const uint8_t *d_src, size_t n_bytes, int geom, PinBuf *host_out = nullptr) {
    BgzfLane &l = ctx->bgzf[lane];
    const size_t block = bgzf_block_bytes(geom);
    const uint32_t nb = (uint32_t)((n_bytes + block - 1) / block);
    int rc;
    PinBuf &ob = host_out ? *host_out : l.out;
    if ((rc = reserve(ctx, l.slots, (size_t)nb * bgzf::SLOT)) || (rc = reserve(ctx, l.meta, (size_t)nb * 8 + 1024)) ||
        (rc = reserve(ctx, l.member_off, (size_t)nb * 8)) || (rc = reserve_pinned(ctx, ob, bgzf_out_cap(n_bytes, geom))))
        return rc;
    l.h_out = ob.p;
    uint32_t *d_size = (uint32_t *)l.meta.p, *d_crc = d_size + nb, *d_ticket = d_crc + nb;
    uint64_t *d_total = (uint64_t *)(((uintptr_t)(d_ticket + 2) + 7) & ~(uintptr_t)7);
    HIPCHK(ctx, hipMemsetAsync(d_ticket, 0, 8, l.stream));
    unsigned long long *prof = nullptr;
    if (getenv("FADEHIP_BGZF_PROF")) {  // shader clocks per phase, printed by wait (development aid)
        prof = (unsigned long long *)(d_total + 1);
        HIPCHK(ctx, hipMemsetAsync(prof, 0, 64 + 8 * 72, l.stream));
    }
    const unsigned cus = (unsigned)std::max(ctx->cu_count, 1);
    bgzf::DeflateArgs a;
    a.src = d_src;
    a.n_bytes = n_bytes;
    a.n_blocks = nb;
    a.slots = (uint8_t *)l.slots.p;
    a.out_size = d_size;
    a.out_crc = d_crc;
    a.ticket = d_ticket;
    a.prof = prof;
    // the geometries differ in the deflate kernel and its launch (a workgroup per CU, or two) ...
    if (geom == 32) hipLaunchKernelGGL(bgzf32::bgzf_deflate_kernel, dim3(std::min<unsigned>(nb, 2u * cus)), dim3(bgzf32::WG), bgzf32::LDS_BYTES, l.stream, a);
    else hipLaunchKernelGGL(bgzf64::bgzf_deflate_kernel, dim3(std::min<unsigned>(nb, cus)), dim3(bgzf64::WG), bgzf64::LDS_BYTES, l.stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bgzf::bgzf_scan_kernel, dim3(1), dim3(1024), 0, l.stream, (const uint32_t *)d_size, nb, (uint64_t *)l.member_off.p, d_total);
    HIPCHK(ctx, hipGetLastError());
    // ... and in the block size the pack kernel writes ISIZE from
    const auto pack = geom == 32 ? bgzf::bgzf_pack_kernel<bgzf32::BLOCK> : bgzf::bgzf_pack_kernel<bgzf64::BLOCK>;
    hipLaunchKernelGGL(pack, dim3(nb), dim3(256), 0, l.stream, (const uint8_t *)l.slots.p, (const uint32_t *)d_size, (const uint32_t *)d_crc,
                       (const uint64_t *)l.member_off.p, (uint64_t)n_bytes, nb, l.h_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(l.h_total, d_total, 8, hipMemcpyDeviceToHost, l.stream));
    HIPCHK(ctx, hipEventRecord(l.done, l.stream));
    l.n_bytes = n_bytes;
    l.n_blocks = nb;
    l.geom = geom;
    l.state = 1;
    return 0;
}

int fadehip_bgzf_deflate_submit(fadehip_ctx *ctx, int lane, const void *src, size_t n_bytes) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (lane < 0 || lane >= FADEHIP_BGZF_LANES) return set_err(ctx, FADEHIP_E_INVALID, "bgzf lane %d out of range", lane);
    if (!src || n_bytes == 0 || n_bytes > ((size_t)1 << 31)) return set_err(ctx, FADEHIP_E_INVALID, "bgzf: 1 .. 2^31 bytes per call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = bgzf_lane_ready(ctx, lane))) return rc;
    BgzfLane &l = ctx->bgzf[lane];
    if ((rc = reserve(ctx, l.src, n_bytes + 64))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(l.src.p, src, n_bytes, hipMemcpyHostToDevice, l.stream));
    return bgzf_enqueue(ctx, lane, (const uint8_t *)l.src.p, n_bytes, bgzf_pick_geom_host(ctx, (const uint8_t *)src, n_bytes));
}

int fadehip_bgzf_deflate_wait(fadehip_ctx *ctx, int lane, const uint8_t **out, size_t *out_bytes) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (lane < 0 || lane >= FADEHIP_BGZF_LANES) return set_err(ctx, FADEHIP_E_INVALID, "bgzf lane %d out of range", lane);
    if (!out || !out_bytes) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    BgzfLane &l = ctx->bgzf[lane];
    if (l.state != 1) return set_err(ctx, FADEHIP_E_STATE, "bgzf lane %d has nothing submitted", lane);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(l.done));
    const uint64_t total = *l.h_total;
    l.state = 0;
    if (getenv("FADEHIP_BGZF_PROF")) {
        unsigned long long pr[8 + 72];
        uint32_t *d_ticket = (uint32_t *)l.meta.p + 2 * (size_t)l.n_blocks;
        uint64_t *d_total = (uint64_t *)(((uintptr_t)(d_ticket + 2) + 7) & ~(uintptr_t)7);
        if (hipMemcpy(pr, d_total + 1, sizeof pr, hipMemcpyDeviceToHost) == hipSuccess) {
            if (pr[8]) {
                fprintf(stderr, "[fadehip bgzf] pipeline timeout: wait 0x%llx (saw %llu, wanted %llu, wave %llu) ticket %llu carry %llu n %llu | cand seq/free:", pr[8], pr[11] >> 32, pr[78], pr[79], pr[9], pr[10], pr[11] & 0xffffffffull);
                for (int k = 0; k < 4; k++) fprintf(stderr, " %llu/%llu", pr[12 + 2 * k], pr[13 + 2 * k]);
                fprintf(stderr, " | lens seq/free:");
                for (int k = 0; k < 24; k++) fprintf(stderr, " %llu/%llu", pr[20 + 2 * k], pr[21 + 2 * k]);
                fprintf(stderr, "\n");
            }
            static const char *nm[7] = {"load", "A match+parse", "B hist", "B codes", "C header+count", "D emit", "CRC"};
            unsigned long long sum = 0;
            for (int k = 0; k < 7; k++) sum += pr[k];
            fprintf(stderr, "[fadehip bgzf] %u blocks, shader clocks per block:", l.n_blocks);
            for (int k = 0; k < 7; k++) fprintf(stderr, " %s %.0f (%.0f%%)", nm[k], (double)pr[k] / l.n_blocks, 100.0 * (double)pr[k] / (double)std::max<unsigned long long>(sum, 1));
            fprintf(stderr, "\n");
            if (pr[41])
                fprintf(stderr, "[fadehip bgzf] B codes, clocks per block: ranks %.0f | merge (one lane) %.0f, depths %.0f, histogram + sums %.0f, leaves %.0f | limit %.0f | the others waited for %.0f | lengths, first codes, codes %.0f\n",
                        (double)pr[40] / l.n_blocks, (double)pr[41] / l.n_blocks, (double)pr[42] / l.n_blocks, (double)pr[43] / l.n_blocks, (double)pr[44] / l.n_blocks, (double)pr[45] / l.n_blocks, (double)pr[46] / l.n_blocks, (double)pr[47] / l.n_blocks);
            if (pr[48])
                fprintf(stderr, "[fadehip bgzf] C header + count, clocks per block: runs of lengths into tokens %.0f | thread 0's bit counts %.0f, then waited for the code-length code %.0f | tokens' bits into the header %.0f\n",
                        (double)pr[48] / l.n_blocks, (double)pr[49] / l.n_blocks, (double)pr[50] / l.n_blocks, (double)pr[51] / l.n_blocks);
            if (pr[56])
                fprintf(stderr, "[fadehip bgzf] A (the first wave's segment), clocks per block: position's bytes, bucket read and written %.0f | candidates' four bytes %.0f | extended %.0f | best picked, who yields, ballot %.0f | the piece's matches taken in turn %.0f | bitmaps, records stored %.0f\n",
                        (double)pr[56] / l.n_blocks, (double)pr[57] / l.n_blocks, (double)pr[58] / l.n_blocks, (double)pr[60] / l.n_blocks, (double)pr[61] / l.n_blocks, (double)pr[62] / l.n_blocks);
            if (pr[52])
                fprintf(stderr, "[fadehip bgzf] D emit, clocks per block: scan of the bit counts, the stream's words cleared %.0f | thread 0's tokens placed %.0f, then waited for the others %.0f | copied out %.0f\n",
                        (double)pr[52] / l.n_blocks, (double)pr[53] / l.n_blocks, (double)pr[54] / l.n_blocks, (double)pr[55] / l.n_blocks);
            fprintf(stderr, "[fadehip bgzf] phase A roles, clocks per block waited / in role: hasher %.0f / %.0f, extenders (sum) %.0f / %.0f, parser %.0f / %.0f\n",
                    (double)pr[60] / l.n_blocks, (double)pr[61] / l.n_blocks, (double)pr[62] / l.n_blocks, (double)pr[63] / l.n_blocks, (double)pr[64] / l.n_blocks, (double)pr[65] / l.n_blocks);
        }
    }
    if (total == 0 || total > (uint64_t)l.n_blocks * bgzf::SLOT) {
        // a block whose pipeline timed out reports size ~0 and, as its CRC, the wait that gave up (role << 28 | piece)
        std::vector<uint32_t> meta(2 * (size_t)l.n_blocks);
        unsigned bad = 0, why = 0;
        if (hipMemcpy(meta.data(), l.meta.p, meta.size() * 4, hipMemcpyDeviceToHost) == hipSuccess)
            for (uint32_t k = 0; k < l.n_blocks; k++)
                if (meta[k] == 0xffffffffu) { if (!bad) why = meta[l.n_blocks + k]; bad++; }
        return set_err(ctx, FADEHIP_E_STATE, "internal: bgzf members add up to %llu bytes (%u blocks timed out, first wait 0x%08x)", (unsigned long long)total, bad, why);
    }
    ctx->bgzf_last_ratio = (double)total / (double)std::max<size_t>(l.n_bytes, 1);
    *out = l.h_out;  // (packed there by the kernel itself)
    *out_bytes = (size_t)total;
    return 0;
}

// ------------------------------------------------------------------------------- BGZF decompression
int fadehip_bgzf_inflate(fadehip_ctx *ctx, const void *members, size_t n_bytes, void *out, size_t out_cap, size_t *out_bytes) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!out_bytes || (n_bytes && !members)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out_bytes = 0;
    if (n_bytes == 0) return 0;
    std::vector<bgzf::InflateBlock> blocks;
    size_t consumed = 0;
    uint64_t total = 0;
    std::string msg;
    if (!scan_bgzf_members((const uint8_t *)members, n_bytes, blocks, &consumed, &total, msg)) return set_err(ctx, FADEHIP_E_INVALID, "bgzf inflate: %s", msg.c_str());
    if (consumed != n_bytes) return set_err(ctx, FADEHIP_E_INVALID, "bgzf inflate: the last member is not whole (%zu of %zu bytes are whole members)", consumed, n_bytes);
    if (total > out_cap || (total && !out)) return set_err(ctx, FADEHIP_E_INVALID, "bgzf inflate: %llu bytes do not fit out_cap %zu", (unsigned long long)total, out_cap);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    InflateLane &l = ctx->inf;
    if (!l.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
    const uint32_t nb = (uint32_t)blocks.size();
    int rc;
    if ((rc = reserve(ctx, l.comp, n_bytes + 16)) || (rc = reserve(ctx, l.blocks, sizeof(bgzf::InflateBlock) * (size_t)nb)) ||
        (rc = reserve(ctx, l.out, (size_t)total + 64)) || (rc = reserve(ctx, l.status, 4 * (size_t)nb)) || (rc = reserve(ctx, l.ticket, 64)) ||
        (rc = reserve_pinned(ctx, l.h_status, 4 * (size_t)nb + 8)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(l.comp.p, members, n_bytes, hipMemcpyHostToDevice, l.stream));
    HIPCHK(ctx, hipMemcpyAsync(l.blocks.p, blocks.data(), sizeof(bgzf::InflateBlock) * (size_t)nb, hipMemcpyHostToDevice, l.stream));
    HIPCHK(ctx, hipStreamSynchronize(l.stream));  // (blocks is a pageable vector about to go out of scope)
    bgzf::InflateArgs a;
    a.comp = (const uint8_t *)l.comp.p;
    a.blocks = (const bgzf::InflateBlock *)l.blocks.p;
    a.n_blocks = nb;
    a.out = (uint8_t *)l.out.p;
    a.out_shift = nullptr;
    a.status = (uint32_t *)l.status.p;
    a.ticket = (uint32_t *)l.ticket.p;
    a.check_crc = 1;
    if ((rc = launch_inflate(ctx, l.stream, a))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(l.h_status.p, l.ticket.p, 8, hipMemcpyDeviceToHost, l.stream));
    HIPCHK(ctx, hipStreamSynchronize(l.stream));
    const uint32_t n_bad = ((const uint32_t *)l.h_status.p)[1];
    if (n_bad) {
        HIPCHK(ctx, hipMemcpy(l.h_status.p, l.status.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        const uint32_t *stt = (const uint32_t *)l.h_status.p;
        for (uint32_t k = 0; k < nb; k++)
            if (stt[k]) return set_err(ctx, FADEHIP_E_INVALID, "bgzf inflate: member %u of %u: %s (%u members failed)", k, nb, inflate_error_name(stt[k]), n_bad);
    }
    if (total) HIPCHK(ctx, hipMemcpy(out, l.out.p, (size_t)total, hipMemcpyDeviceToHost));
    *out_bytes = (size_t)total;
    return 0;
}

// ------------------------------------------------------------------------------- the file path on the device
struct fadehip_bam_stream {
    fadehip_ctx *ctx = nullptr;
    int32_t floor_len = 0, window = 0, n_ref = 0;
    uint32_t first_record = 0, tail_trim = 0;
    bool stored = false;  // uncompressed BGZF out
    bool clip = false;    // FADEHIP_BAM_CLIP: artifact calls leave hard-clipped (the <true> kernels of bam_device.hpp)
    bool no_output = false;  // FADEHIP_BAM_NO_OUTPUT: back gives the call's device bytes back without making BGZF of them
    bool extract = false;    // FADEHIP_BAM_EXTRACT: every call also leaves `fade extract`'s records of its artifact calls
    bool eject = false;      // FADEHIP_BAM_EJECT: artifact calls are not written (the eject kernels of bam_device.hpp) ...
    bool eject_groups = false;  // FADEHIP_BAM_EJECT_GROUPS: ... nor any record of their name group; a group never lies across two calls
    DevBuf names_text, names_off;
    struct Out {
        DevBuf o;
        size_t bytes = 0;
        hipEvent_t ready = nullptr;
        // extract: the call's extract records on the device, their bytes and number, and the event behind their copy to the host
        DevBuf x;
        size_t xbytes = 0;
        int64_t xrecs = 0;
        hipEvent_t xready = nullptr;
        int state = 0;  // 0 free, 1 its call's kernels are enqueued up to the tag sizes (to be finished), 2 finished: waiting for back
    } ring[FADEHIP_BAM_CHUNKS];
    // The front half, two calls in flight.  Call k lives in set k & 1 and on the ctx's slot k & 1 (a stream each):
    //   A  H2D (or H2D + inflate), carry-over of the previous call's cut-off record, framing, which records go to the gate
    //      and their sizes -> the host waits (buffers are sized from what the device found)
    //   B  packing, gate / score pass / pass 2, tag sizes                      -> enqueued, front returns
    //   C  the host reads the sizes (the one other wait), the rewrite kernel   -> "finishing" the call: done by back when it
    //      takes the call (or by front before the set is used again)
    // so that A of call k + 1 runs on the device beside B and C of call k, and no stream idles while the host waits for
    // another.  Order between calls: A(k + 1) needs where call k's last whole record ended (known once front(k) has waited for
    // its A); everything else of two calls is independent.
    struct Set {
        DevBuf comp, blocks, status, ticket;  // members to inflate on the device
        DevBuf u;                             // the call's inflated bytes, the previous call's cut-off record in front
        DevBuf seg, slots, rec_off, info, sent_of, art_of, out_size, blk32, blk64, counts;
        DevBuf ex_size, ex_blk;               // extract: bytes per record, block sums and bases (the tag arrays' counterparts)
        DevBuf ej_head, ej_blk, ej_grp;       // eject: every record's group start, the blocks' last starts and carries, the groups' marks
        bam::TagArgs xa;                      // extract: ta with the extract stream's sizes, sums, counts and output
        PinBuf h_blocks, h_counts;
        uint64_t k = ~0ull;
        uint32_t n_rec = 0, n_sent = 0, ntb = 0;
        bool pending = false;  // B is enqueued, C is not
        bam::PackArgs pa;                     // A fills it (u, rec_off, counts, info, sent_of: what B and the tag arguments start from), B the batch arrays
        bam::TagArgs ta;
        Out *out = nullptr;
        std::mutex mu;  // finishing the set's call (front and back may both come to do it; the OTHER set's call is not held up)
    } set[2];
    uint32_t prev_len = 0, prev_consumed = 0;  // of the previous call's u
    double rec_bytes_avg = 0;                  // bytes per record of the previous call (sizes the next call's record-parallel launch)
    uint64_t k_front = 0, k_back = 0;
    uint64_t k_sub = 0;                     // calls handed to the compressor (back may run one ahead of the call it returns)
    PinBuf outbuf[FADEHIP_BAM_CHUNKS];      // the members of call k, packed by the kernel itself: pinned, k % FADEHIP_BAM_CHUNKS
    // extract: the extract records of call k, pinned, k % (FADEHIP_BAM_CHUNKS + 1) — one more than the ring, because the copy is
    // enqueued when the call is finished, which front may do one back call before the compressor of that ring place starts
    PinBuf xbuf[FADEHIP_BAM_CHUNKS + 1];
    const uint8_t *last_x = nullptr;        // fadehip_bam_back_extract: what the most recent back finished
    size_t last_xbytes = 0;
    int64_t last_xrecs = 0;
    bool have_back = false;
    // the counts of a call as they cross to the host: the call's ChunkCounts and, with extract, the extract stream's behind it
    size_t counts_bytes() const { return sizeof(bam::ChunkCounts) * (extract ? 2u : 1u); }
    std::mutex mu;
    std::condition_variable cv;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n_records = 0, n_oversize = 0, n_redone = 0, n_ejected = 0;
    bool failed = false, ended = false, closing = false;
    double t_inflate = 0, t_frame = 0, t_run = 0, t_tags = 0;
};

namespace {

int bam_fail(fadehip_bam_stream *st, int rc) {
    {
        std::lock_guard<std::mutex> l(st->mu);
        st->failed = true;
    }
    st->cv.notify_all();
    return rc;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// FADEHIP_BAM_TRACE=1: where the first calls of a stream spend their time (buffers, streams and staging memory are made in them)
struct CallTrace {
    bool on;
    const char *who;
    uint64_t k;
    double t;
    CallTrace(const char *w, uint64_t kk) : on(kk < 4 && getenv("FADEHIP_BAM_TRACE")), who(w), k(kk), t(on ? now_s() : 0) {}
    void mark(const char *what) {
        if (!on) return;
        const double n = now_s();
        fprintf(stderr, "[fadehip trace] %s %llu: %-28s %8.3f ms\n", who, (unsigned long long)k, what, (n - t) * 1e3);
        t = n;
    }
};

// FADEHIP_BAM_EXTRACT, C of call k behind the event the compressor waits for: the extract records of the call's artifact
// calls, from the untouched input records, and their copy into the pinned buffer back_extract hands out (the total came
// with the tag sizes)
int bam_finish_extract(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, uint64_t k, hipStream_t q) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *out = S.out;
    int rc;
    out->xbytes = 0;
    out->xrecs = 0;
    if (S.n_rec) {
        const bam::ChunkCounts *xc = (const bam::ChunkCounts *)S.h_counts.p + 1;
        const uint64_t xb = xc->out_bytes;
        if (xb > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu extract bytes in one call (at most 2^31)", (unsigned long long)xb);
        if (xb) {
            PinBuf &xh = st->xbuf[k % (FADEHIP_BAM_CHUNKS + 1)];
            if ((rc = reserve_roomy(ctx, out->x, (size_t)xb + 256)) || (rc = reserve_pinned(ctx, xh, (size_t)xb + (size_t)xb / 4 + 256))) return rc;
            S.xa.o = (uint8_t *)out->x.p;
            hipLaunchKernelGGL(bam::bam_extract_write_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.xa);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(xh.p, out->x.p, (size_t)xb, hipMemcpyDeviceToHost, q));
            out->xbytes = (size_t)xb;
            out->xrecs = (int64_t)xc->n_records;
        }
    }
    if (!out->xready) HIPCHK(ctx, hipEventCreateWithFlags(&out->xready, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    HIPCHK(ctx, hipEventRecord(out->xready, q));
    return 0;
}

// C of call k (see fadehip_bam_stream): waits for the call's run and tag sizes, sizes the output, enqueues the rewrite.
// Idempotent; front and back may both arrive here for the same call.
int bam_finish_call(fadehip_bam_stream *st, uint64_t k) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Set &S = st->set[k & 1];
    std::lock_guard<std::mutex> pl(S.mu);
    if (S.k != k || !S.pending) return 0;
    Slot &s = ctx->slots[k & 1];
    hipStream_t q = s.stream;
    fadehip_bam_stream::Out *out = S.out;
    const double t0 = now_s();
    int rc;
    out->bytes = 0;
    if (S.n_rec) {
        bam::ChunkCounts *h_counts = (bam::ChunkCounts *)S.h_counts.p;
        if (S.n_sent) {
            if ((rc = finish_run(ctx, s, (int)(k & 1)))) return rc;  // waits for the stream: run and sizes
            std::lock_guard<std::mutex> l(st->mu);
            for (int t = 0; t < 8; t++) st->stats[t] += s.stats[t];
            st->n_oversize += s.n_oversize;
        } else {
            HIPCHK(ctx, hipStreamSynchronize(q));
            std::lock_guard<std::mutex> l(st->mu);
            st->stats[0] += S.n_rec;
        }
        const uint64_t out_bytes = h_counts->out_bytes;
        if (out_bytes > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu output bytes in one call (at most 2^31)", (unsigned long long)out_bytes);
        if ((rc = reserve_roomy(ctx, out->o, (size_t)out_bytes + 256))) return rc;
        S.ta.o = (uint8_t *)out->o.p;
        if (st->clip) hipLaunchKernelGGL(bam::bam_rewrite_kernel<true>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.ta);
        else hipLaunchKernelGGL(bam::bam_rewrite_kernel<false>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.ta);
        HIPCHK(ctx, hipGetLastError());
        out->bytes = (size_t)out_bytes;
        std::lock_guard<std::mutex> l(st->mu);
        st->n_records += S.n_rec;
        st->n_ejected += h_counts->n_ejected;
    }
    if (!out->ready) HIPCHK(ctx, hipEventCreateWithFlags(&out->ready, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    HIPCHK(ctx, hipEventRecord(out->ready, q));
    if (st->extract && (rc = bam_finish_extract(st, S, k, q))) return rc;
    S.pending = false;
    st->t_tags += now_s() - t0;
    {
        std::lock_guard<std::mutex> l(st->mu);
        out->state = 2;
    }
    st->cv.notify_all();
    return 0;
}

// A of call k (see fadehip_bam_stream) on the slot's stream q, up to and with the wait and the checks of what came back: the
// call's counts are in S.h_counts then, and S.pa is ready for B
int bam_front_frame(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, CallTrace &tr, const uint8_t *members, size_t n_bytes, int last, bool raw) {
    fadehip_ctx *ctx = st->ctx;
    const uint64_t k = st->k_front;
    hipStream_t q = ctx->slots[k & 1].stream;
    int rc;
    const double t0 = now_s();
    // ---- the members, and where their payloads go
    std::vector<bgzf::InflateBlock> blocks;
    size_t consumed = 0;
    uint64_t total = 0;
    std::string msg;
    if (raw) {
        total = n_bytes;  // the caller has inflated the members: these are their payloads
    } else {
        if (n_bytes && !scan_bgzf_members(members, n_bytes, blocks, &consumed, &total, msg)) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: %s", msg.c_str());
        if (consumed != n_bytes) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: front takes whole BGZF members (%zu of %zu bytes are)", consumed, n_bytes);
    }
    const uint32_t carry = st->prev_len - st->prev_consumed;
    if (st->eject_groups && (uint64_t)carry + total > (uint64_t)bam::MAX_U && total <= (uint64_t)bam::MAX_U)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: a name group is longer than a call can hold (%u bytes carried over, at most %u with the call's own): "
                       "FADE_BAM_DEVICE=0 takes the host pipeline, which holds a group of any length", carry, bam::MAX_U);
    if ((uint64_t)carry + total > (uint64_t)bam::MAX_U) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu inflated bytes in one call (at most %u)", (unsigned long long)total + carry, bam::MAX_U);
    uint32_t u_len = carry + (uint32_t)total;
    if (last && !raw && st->tail_trim) {  // (the bytes behind this stream's last record, in its last member, belong to another reader)
        if ((uint64_t)st->tail_trim > total) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: tail_trim %u exceeds the last call's %llu bytes", st->tail_trim, (unsigned long long)total);
        u_len -= st->tail_trim;
    }
    // (sized from the UNTRIMMED length: the inflate kernel writes the last member's whole ISIZE, tail_trim only shortens
    // what the framing looks at)
    if ((rc = reserve_roomy(ctx, S.u, (size_t)carry + (size_t)total + 256))) return rc;
    uint8_t *u = (uint8_t *)S.u.p;
    // the cut-off record of the previous call: its bytes are final (front waited for that call's framing), and the rewrite
    // that also reads them does not change them
    if (carry) HIPCHK(ctx, hipMemcpyAsync(u, (const uint8_t *)st->set[(k + 1) & 1].u.p + st->prev_consumed, carry, hipMemcpyDeviceToDevice, q));
    const uint32_t nb = (uint32_t)blocks.size();
    if (raw && n_bytes) HIPCHK(ctx, hipMemcpyAsync(u + carry, members, n_bytes, hipMemcpyHostToDevice, q));
    const bool fine = tr.on && k == 0 && getenv("FADEHIP_BAM_TRACE_FINE");
    if (fine) { tr.mark("  copy enqueued"); (void)hipStreamSynchronize(q); tr.mark("  copy waited for"); }
    if (nb) {
        for (auto &b : blocks) b.dst_off += carry;
        if ((rc = reserve_roomy(ctx, S.comp, n_bytes + 16)) || (rc = reserve_roomy(ctx, S.blocks, sizeof(bgzf::InflateBlock) * (size_t)nb)) ||
            (rc = reserve_roomy(ctx, S.status, 4 * (size_t)nb)) || (rc = reserve_roomy(ctx, S.ticket, 64)) ||
            (rc = reserve_pinned(ctx, S.h_blocks, sizeof(bgzf::InflateBlock) * (size_t)nb)))
            return rc;
        memcpy(S.h_blocks.p, blocks.data(), sizeof(bgzf::InflateBlock) * (size_t)nb);
        HIPCHK(ctx, hipMemcpyAsync(S.comp.p, members, n_bytes, hipMemcpyHostToDevice, q));
        HIPCHK(ctx, hipMemcpyAsync(S.blocks.p, S.h_blocks.p, sizeof(bgzf::InflateBlock) * (size_t)nb, hipMemcpyHostToDevice, q));
        bgzf::InflateArgs ia;
        ia.comp = (const uint8_t *)S.comp.p;
        ia.blocks = (const bgzf::InflateBlock *)S.blocks.p;
        ia.n_blocks = nb;
        ia.out = u;
        ia.out_shift = nullptr;
        ia.status = (uint32_t *)S.status.p;
        ia.ticket = (uint32_t *)S.ticket.p;
        ia.check_crc = 1;
        if ((rc = launch_inflate(ctx, q, ia))) return rc;
    }
    // ---- framing
    const uint32_t n_seg = (u_len + bam::SEG - 1) / bam::SEG;
    const uint32_t rec_cap = u_len / 36u + 2u;
    if ((rc = reserve_roomy(ctx, S.seg, 16 * (size_t)std::max(n_seg, 1u))) || (rc = reserve_roomy(ctx, S.slots, 4 * (size_t)bam::SEG_SLOTS * std::max(n_seg, 1u))) ||
        (rc = reserve_roomy(ctx, S.rec_off, 4 * (size_t)rec_cap)) || (rc = reserve_roomy(ctx, S.counts, st->counts_bytes())) ||
        (rc = reserve_pinned(ctx, S.h_counts, st->counts_bytes() + 16)))
        return rc;
    bam::ChunkCounts *d_counts = (bam::ChunkCounts *)S.counts.p;
    bam::ChunkCounts *h_counts = (bam::ChunkCounts *)S.h_counts.p;
    HIPCHK(ctx, hipMemsetAsync(d_counts, 0, st->counts_bytes(), q));
    HIPCHK(ctx, hipMemsetAsync(&d_counts->l_seq_min, 0xff, 4, q));
    bam::FrameArgs fa;
    fa.u = u;
    fa.u_len = u_len;
    fa.first = k == 0 ? st->first_record : 0u;
    fa.n_ref = st->n_ref;
    fa.n_seg_cap = n_seg;
    fa.cand = (uint32_t *)S.seg.p;
    fa.exit_ = fa.cand + std::max(n_seg, 1u);
    fa.cnt = fa.exit_ + std::max(n_seg, 1u);
    fa.base = fa.cnt + std::max(n_seg, 1u);
    fa.slots = (uint32_t *)S.slots.p;
    fa.rec_off = (uint32_t *)S.rec_off.p;
    fa.rec_cap = rec_cap;
    fa.counts = d_counts;
    if (n_seg) {
        hipLaunchKernelGGL(bam::bam_frame_walk_kernel, dim3((n_seg + bam::WALK_SEGS - 1) / bam::WALK_SEGS), dim3(64), 0, q, fa);
        HIPCHK(ctx, hipGetLastError());
    }
    if (fine) { tr.mark("  memsets, walk enqueued"); (void)hipStreamSynchronize(q); tr.mark("  waited for"); }
    hipLaunchKernelGGL(bam::bam_frame_resolve_kernel, dim3(1), dim3(64), 0, q, fa);
    HIPCHK(ctx, hipGetLastError());
    if (fine) { tr.mark("  resolve enqueued"); (void)hipStreamSynchronize(q); tr.mark("  waited for"); }
    hipLaunchKernelGGL(bam::bam_frame_compact_kernel, dim3(std::max(1u, (n_seg + 3) / 4)), dim3(256), 0, q, fa);
    HIPCHK(ctx, hipGetLastError());
    if (st->eject_groups && !last) {  // the call's last name group may go on in the next call: it is given back (and carried over)
        hipLaunchKernelGGL(bam::bam_eject_hold_kernel, dim3(1), dim3(64), 0, q, fa);
        HIPCHK(ctx, hipGetLastError());
    }
    // which records go to the device's gate, their sizes: enqueued behind the framing for as many records as the bytes could
    // hold at most (threads beyond the records that are there return at once), so that ONE wait brings back both counts
    const uint32_t nblk_cap = (rec_cap + bam::PACK_BLOCK - 1) / bam::PACK_BLOCK;
    if ((rc = reserve_roomy(ctx, S.info, 4 * (size_t)rec_cap)) || (rc = reserve_roomy(ctx, S.sent_of, 4 * (size_t)rec_cap)) ||
        (rc = reserve_roomy(ctx, S.out_size, 4 * (size_t)rec_cap)) || (rc = reserve_roomy(ctx, S.blk32, 24 * (size_t)nblk_cap)))
        return rc;
    bam::PackArgs &pa = S.pa;
    memset(&pa, 0, sizeof pa);
    pa.u = u;
    pa.rec_off = fa.rec_off;
    pa.counts_in = d_counts;
    pa.r0 = 0;
    pa.r1_cap = rec_cap;
    pa.info = (uint32_t *)S.info.p;
    pa.blk_sums = (uint32_t *)S.blk32.p;
    pa.blk_base = pa.blk_sums + 3 * (size_t)nblk_cap;
    pa.counts = d_counts;
    pa.sent_of = (int32_t *)S.sent_of.p;
    // (sized from the bytes per record of the calls so far, with a margin; the kernel strides over what is really there)
    const uint32_t nblk_est = st->rec_bytes_avg > 0 ? (uint32_t)((double)u_len / st->rec_bytes_avg * 1.25 / bam::PACK_BLOCK) + 8u : nblk_cap;
    hipLaunchKernelGGL(bam::bam_pack_count_kernel, dim3(std::max(1u, std::min(nblk_cap, nblk_est))), dim3(bam::PACK_BLOCK), 0, q, pa);
    HIPCHK(ctx, hipGetLastError());
    if (fine) { tr.mark("  compact, pack count enqueued"); (void)hipStreamSynchronize(q); tr.mark("  waited for"); }
    hipLaunchKernelGGL(bam::bam_pack_scan_kernel, dim3(1), dim3(1024), 0, q, pa, nblk_cap);
    HIPCHK(ctx, hipGetLastError());
    if (fine) { tr.mark("  pack scan enqueued"); (void)hipStreamSynchronize(q); tr.mark("  waited for"); }
    HIPCHK(ctx, hipMemcpyAsync(h_counts, d_counts, sizeof(bam::ChunkCounts), hipMemcpyDeviceToHost, q));
    uint32_t *h_tick = (uint32_t *)(S.h_counts.p + st->counts_bytes());
    h_tick[0] = h_tick[1] = 0;
    if (nb) HIPCHK(ctx, hipMemcpyAsync(h_tick, S.ticket.p, 8, hipMemcpyDeviceToHost, q));
    const double t1 = now_s();
    tr.mark("A enqueued");
    HIPCHK(ctx, hipStreamSynchronize(q));  // (1) the records of this call and the sizes of their batch
    const double t2 = now_s();
    tr.mark("A waited for");
    st->t_inflate += t1 - t0;
    st->t_frame += t2 - t1;
    if (nb && h_tick[1]) {
        std::vector<uint32_t> stt(nb);
        HIPCHK(ctx, hipMemcpy(stt.data(), S.status.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        for (uint32_t b = 0; b < nb; b++)
            if (stt[b]) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: call %llu, member %u of %u: %s (%u members failed)", (unsigned long long)k, b, nb, inflate_error_name(stt[b]), h_tick[1]);
    }
    if (h_counts->frame_err)
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: call %llu: %s at inflated offset %u", (unsigned long long)k,
                       h_counts->frame_err == 1 ? "a record's block_size is impossible" : "the first record lies beyond the bytes given", h_counts->frame_err_at);
    const uint32_t n_rec = h_counts->n_records, used = h_counts->consumed;
    if (last && used != u_len) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the input ends inside a record (%u bytes behind the last whole one)", u_len - used);
    st->prev_len = u_len;
    st->prev_consumed = used;
    st->n_redone += h_counts->n_redone;
    if (n_rec) st->rec_bytes_avg = (double)used / (double)n_rec;
    return 0;
}

// B's tail, what anno.d:94-107 adds: which alignment is whose, the sizes of the n_rec records as they leave (ntb blocks of
// TAG_BLOCK) and, with the flags, of the extract records and less what eject takes out; their scans; the counts to the host
int bam_enqueue_sizes(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, Slot &s, uint32_t n_rec, uint32_t n_sent, uint32_t ntb) {
    fadehip_ctx *ctx = st->ctx;
    hipStream_t q = s.stream;
    const bam::PackArgs &pa = S.pa;
    bam::ChunkCounts *d_counts = pa.counts;
    int rc;
    if ((rc = reserve_roomy(ctx, S.art_of, 4 * (size_t)std::max(n_sent, 1u)))) return rc;
    if (n_sent) {
        HIPCHK(ctx, hipMemsetAsync(S.art_of.p, 0xff, 4 * (size_t)n_sent, q));
        if (s.out_cap) {
            hipLaunchKernelGGL(bam::bam_art_index_kernel, dim3((s.out_cap + 255) / 256), dim3(256), 0, q, (const fadehip_aln *)s.aln.p,
                               (const uint32_t *)(s.d_counters() + 2 * NUM_LISTS + 3), s.out_cap, (int32_t *)S.art_of.p, n_sent);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    bam::TagArgs &ta = S.ta;
    memset(&ta, 0, sizeof ta);
    ta.u = pa.u;
    ta.rec_off = pa.rec_off;
    ta.counts_in = d_counts;
    ta.r0 = 0;
    ta.r1_cap = n_rec;
    ta.info = pa.info;
    ta.sent_of = pa.sent_of;
    ta.rs = (const uint8_t *)s.rs.p;
    ta.aln = (const fadehip_aln *)s.aln.p;
    ta.art_of = (const int32_t *)S.art_of.p;
    ta.names.text = (const char *)st->names_text.p;
    ta.names.off = (const uint32_t *)st->names_off.p;
    ta.names.n = st->n_ref;
    ta.out_size = (uint32_t *)S.out_size.p;
    ta.blk_sums = (uint64_t *)S.blk64.p;
    ta.blk_base = ta.blk_sums + ntb;
    ta.counts = d_counts;
    ta.out_base = 0;
    if (st->clip) hipLaunchKernelGGL(bam::bam_tag_size_kernel<true>, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ta);
    else hipLaunchKernelGGL(bam::bam_tag_size_kernel<false>, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ta);
    HIPCHK(ctx, hipGetLastError());
    // (eject: the scan comes behind the eject kernels, which come behind the extract sizes — see below)
    if (!st->eject) {
        hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, ta, ntb);
        HIPCHK(ctx, hipGetLastError());
    }
    if (st->extract) {
        // the extract records' sizes into the same scan, their total into the ChunkCounts behind the call's own: it crosses
        // to the host in the copy below, which back reads anyway
        if ((rc = reserve_roomy(ctx, S.ex_size, 4 * (size_t)n_rec)) || (rc = reserve_roomy(ctx, S.ex_blk, 16 * (size_t)ntb))) return rc;
        bam::TagArgs &xa = S.xa;
        xa = ta;
        xa.out_size = (uint32_t *)S.ex_size.p;
        xa.blk_sums = (uint64_t *)S.ex_blk.p;
        xa.blk_base = xa.blk_sums + ntb;
        xa.counts = d_counts + 1;
        xa.o = nullptr;
        hipLaunchKernelGGL(bam::bam_extract_size_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, xa);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, xa, ntb);
        HIPCHK(ctx, hipGetLastError());
    }
    if (st->eject) {
        // which records leave: out_size 0 and INFO_BAD for them, the blocks' sums again, and only then the scan of the
        // sums.  Behind the extract sizes, which are taken of every artifact call and look at `info`.
        bam::EjectArgs ea;
        memset(&ea, 0, sizeof ea);
        ea.u = pa.u;
        ea.off32 = pa.rec_off;
        ea.n = n_rec;
        ea.sent_of = pa.sent_of;
        ea.rs = (const uint8_t *)s.rs.p;
        ea.out_size = ta.out_size;
        ea.info = pa.info;
        ea.blk_sums = ta.blk_sums;
        ea.counts = d_counts;
        if (st->eject_groups) {
            if ((rc = reserve_roomy(ctx, S.ej_head, 4 * (size_t)n_rec)) || (rc = reserve_roomy(ctx, S.ej_blk, 8 * (size_t)ntb)) ||
                (rc = reserve_roomy(ctx, S.ej_grp, 4 * (size_t)n_rec)))
                return rc;
            ea.head_of = (uint32_t *)S.ej_head.p;
            ea.blk_head = (uint32_t *)S.ej_blk.p;
            ea.blk_carry = ea.blk_head + ntb;
            ea.grp = (uint32_t *)S.ej_grp.p;
        }
        if ((rc = enqueue_eject(ctx, q, ea, ntb, st->eject_groups))) return rc;
        hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, ta, ntb);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(S.h_counts.p, d_counts, st->counts_bytes(), hipMemcpyDeviceToHost, q));
    return 0;
}

// B of call k: the records that go to the gate packed into the slot's batch arrays, annotateTask on the device (level 2's
// kernels, results left there), then the sizes
int bam_front_run(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, Slot &s, CallTrace &tr, uint32_t n_rec) {
    fadehip_ctx *ctx = st->ctx;
    hipStream_t q = s.stream;
    bam::PackArgs &pa = S.pa;
    const bam::ChunkCounts *h_counts = (const bam::ChunkCounts *)S.h_counts.p;
    int rc;
    const uint32_t nblk = (n_rec + bam::PACK_BLOCK - 1) / bam::PACK_BLOCK, ntb = (n_rec + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    if ((rc = reserve_roomy(ctx, S.blk64, 16 * (size_t)ntb))) return rc;
    if (h_counts->n_bad_layout)
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: call %llu: %u records whose fields do not fit their block_size or whose tags are not whole fields (corrupt BAM)", (unsigned long long)st->k_front, h_counts->n_bad_layout);
    const uint32_t n_sent = h_counts->n_sent;
    if ((uint64_t)h_counts->n_seq * 2 >= ((uint64_t)1 << 32)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: packed sequence bytes per call must stay below 2^31");
    if (s.state == 2) HIPCHK(ctx, hipStreamSynchronize(s.stream));
    s.state = 0;
    s.device_only = true;
    s.next.valid = false;
    s.have_batch = false;
    s.cur = 0;
    s.L = batch_layout(n_sent, h_counts->n_cig, h_counts->n_seq);
    if ((rc = reserve_roomy(ctx, s.in[0], s.L.total))) return rc;
    uint8_t *ib = (uint8_t *)s.in[0].p;
    pa.tid = (int32_t *)(ib + s.L.off[A_TID]);
    pa.pos = (int32_t *)(ib + s.L.off[A_POS]);
    pa.lseq = (int32_t *)(ib + s.L.off[A_LSEQ]);
    pa.cigar_off = (uint32_t *)(ib + s.L.off[A_CIGOFF]);
    pa.seq_off = (uint32_t *)(ib + s.L.off[A_SEQOFF]);
    pa.flag = (uint16_t *)(ib + s.L.off[A_FLAG]);
    pa.has_sa = ib + s.L.off[A_SA];
    pa.cigar_ops = (uint32_t *)(ib + s.L.off[A_CIG]);
    pa.seq = ib + s.L.off[A_SEQ];
    hipLaunchKernelGGL(bam::bam_pack_write_kernel, dim3(nblk), dim3(bam::PACK_BLOCK), 0, q, pa);
    HIPCHK(ctx, hipGetLastError());
    tr.mark("pack enqueued");
    // ---- annotateTask on the device (level 2's kernels), results left there
    s.n_reads = (int)n_sent;
    s.n_skipped = (int)(n_rec - n_sent);
    s.floor_len = st->floor_len;
    s.window = st->window;
    memset(s.hist, 0, sizeof s.hist);
    s.wide.clear();
    s.wide_all = false;
    s.out_bound = n_sent;
    s.max_lq = 0;
    s.l_seq_lo = 0;  // (the bounds below are counted on the device over these very records)
    s.l_seq_hi = INT32_MAX;
    s.span_bound = 1;
    if (n_sent) {
        const int lmin = (int)std::min<uint32_t>(h_counts->l_seq_min, (uint32_t)MAX_LONG_QUERY), lmax = (int)std::min<uint32_t>(h_counts->l_seq_max, (uint32_t)MAX_LONG_QUERY);
        const int c_lo = list_of_len(std::max(lmin, 1)), c_hi = list_of_len(std::max(lmax, 1));
        for (int c = c_lo; c <= c_hi; c++) s.hist[c] = n_sent;  // any of them may be of any length in between
        if (h_counts->n_long_q) s.hist[LONG_LIST] = h_counts->n_long_q;  // (the exact number of reads beyond 512 bases)
        s.max_lq = std::max(lmax, 1);
        s.span_bound = std::max<int64_t>(h_counts->span_max, 1);
        s.wide_all = s.span_bound > WIDE_MIN_SPAN;
    }
    if (n_sent) {
        if ((rc = plan_run(ctx, s)) || (rc = enqueue_run(ctx, s))) {
            (void)hipStreamSynchronize(q);
            return rc;
        }
        s.state = 2;
    }
    tr.mark("run planned and enqueued");
    if ((rc = bam_enqueue_sizes(st, S, s, n_rec, n_sent, ntb))) return rc;
    S.n_sent = n_sent;
    S.ntb = ntb;
    return 0;
}

int bam_front_impl(fadehip_bam_stream *st, const uint8_t *members, size_t n_bytes, int last, bool raw) {
    fadehip_ctx *ctx = st->ctx;
    const uint64_t k = st->k_front;
    fadehip_bam_stream::Set &S = st->set[k & 1];
    Slot &s = ctx->slots[k & 1];
    int rc;
    // the set's previous call must have been finished (back has usually done that long ago)
    CallTrace tr("front", k);
    if (ctx->n_contigs == 0) return set_err(ctx, FADEHIP_E_STATE, "fadehip_genome_upload has not been called");
    if (k >= 2 && (rc = bam_finish_call(st, k - 2))) return rc;
    tr.mark("finish call k - 2");
    // every stream is an HSA queue to set up and to give back (tens of ms each): slot 0 works on the ctx's copy stream, which
    // exists anyway and which the file path does not use otherwise; slot 1 gets a stream of its own when the second call comes
    if (ctx->split_cus > 0 && !s.stream && !s.h_zb) {
        ctx->tail_cus_per_xcd = 0;  // (no third set of CUs)
        s.stream = xcd_slice_stream(ctx, 0, ctx->split_cus);
    }
    if (!s.stream && !s.h_zb && (k & 1) == 0 && ctx->copy_stream) s.stream = ctx->copy_stream;
    if ((rc = ensure_slot(ctx, s))) return rc;
    tr.mark("slot (stream, events)");
    if ((rc = bam_front_frame(st, S, tr, members, n_bytes, last, raw))) return rc;
    const double t2 = now_s();
    const uint32_t n_rec = ((const bam::ChunkCounts *)S.h_counts.p)->n_records;
    // ---- a place in the ring
    fadehip_bam_stream::Out *out = &st->ring[k % FADEHIP_BAM_CHUNKS];
    {
        std::unique_lock<std::mutex> l(st->mu);
        st->cv.wait(l, [&] { return out->state == 0 || st->failed || st->closing; });
        if (st->failed || st->closing) return set_err(ctx, FADEHIP_E_STATE, "bam stream: stopped");
    }
    tr.mark("place in the ring");
    out->bytes = 0;
    S.k = k;
    S.n_rec = n_rec;
    S.n_sent = 0;
    S.ntb = 0;
    S.out = out;
    if (n_rec && (rc = bam_front_run(st, S, s, tr, n_rec))) return rc;
    S.pending = true;
    tr.mark("tag sizes enqueued");
    st->t_run += now_s() - t2;
    // the inflated bytes of this call are read by the next call's carry copy and by this call's rewrite, which change nothing;
    // the set's buffers are written again by call k + 2, whose front finishes this call first.
    {
        std::lock_guard<std::mutex> l(st->mu);
        out->state = 1;
        st->k_front = k + 1;
        if (last) st->ended = true;
    }
    st->cv.notify_all();
    return 0;
}

}  // namespace

int fadehip_bam_open(fadehip_ctx *ctx, const fadehip_bam_config *cfg, fadehip_bam_stream **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!cfg || !out || cfg->n_ref < 0 || (cfg->n_ref && !cfg->ref_names) || cfg->window < 0 || (cfg->flags & ~(FADEHIP_BAM_STORED | FADEHIP_BAM_NO_OUTPUT | FADEHIP_BAM_CLIP | FADEHIP_BAM_EXTRACT | FADEHIP_BAM_EJECT | FADEHIP_BAM_EJECT_GROUPS)))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: bad configuration");
    if ((cfg->flags & FADEHIP_BAM_CLIP) && (cfg->flags & (FADEHIP_BAM_EJECT | FADEHIP_BAM_EJECT_GROUPS)))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_CLIP and FADEHIP_BAM_EJECT exclude each other (`fade out` clips an artifact or ejects it)");
    if (!ctx->two_pass) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: needs the default kernels (FADEHIP_KERNEL unset)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fadehip_bam_stream *st = new (std::nothrow) fadehip_bam_stream;
    if (!st) return set_err(ctx, FADEHIP_E_NOMEM, "out of memory");
    st->ctx = ctx;
    st->floor_len = cfg->floor_len;
    st->window = cfg->window;
    st->n_ref = cfg->n_ref;
    st->first_record = cfg->first_record;
    st->tail_trim = cfg->tail_trim;
    st->stored = (cfg->flags & FADEHIP_BAM_STORED) != 0;
    st->no_output = (cfg->flags & FADEHIP_BAM_NO_OUTPUT) != 0;
    st->clip = (cfg->flags & FADEHIP_BAM_CLIP) != 0;
    st->extract = (cfg->flags & FADEHIP_BAM_EXTRACT) != 0;
    st->eject_groups = (cfg->flags & FADEHIP_BAM_EJECT_GROUPS) != 0;
    st->eject = st->eject_groups || (cfg->flags & FADEHIP_BAM_EJECT) != 0;
    std::string text;
    std::vector<uint32_t> off((size_t)cfg->n_ref + 1, 0);
    for (int k = 0; k < cfg->n_ref; k++) {
        if (!cfg->ref_names[k]) { delete st; return set_err(ctx, FADEHIP_E_INVALID, "bam stream: ref_names[%d] is NULL", k); }
        off[(size_t)k] = (uint32_t)text.size();
        text += cfg->ref_names[k];
    }
    off[(size_t)cfg->n_ref] = (uint32_t)text.size();
    int rc;
    if ((rc = reserve(ctx, st->names_text, text.size() + 1)) || (rc = reserve(ctx, st->names_off, 4 * off.size()))) { fadehip_bam_close(st); return rc; }
    // (on the ctx's copy stream: a synchronous hipMemcpy would bring up the null stream, one more queue to set up and to give back)
    if (hipMemcpyAsync(st->names_text.p, text.data(), text.size(), hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
        hipMemcpyAsync(st->names_off.p, off.data(), 4 * off.size(), hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
        hipStreamSynchronize(ctx->copy_stream) != hipSuccess) {
        fadehip_bam_close(st);
        return set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the contig names failed");
    }
    *out = st;
    return 0;
}

// What the first calls of a stream would otherwise make one after the other, each in its turn holding up the thread that
// came to it — the second slot's stream and the compressor lanes' streams (HSA queues: 7-10 ms each, and a launch on
// another thread waits meanwhile), the three staging buffers of the members, the inflated bytes' buffers — made here side by
// side; then one copy up, one down and one wait per stream (the first of each costs milliseconds).  Optional, and meant
// for a thread of its own beside the caller's own start-up (reading the FASTA, the input's first members).
int fadehip_bam_prepare(fadehip_bam_stream *st, size_t call_bytes) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (call_bytes == 0 || call_bytes > (size_t)bam::MAX_U) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: prepare takes the inflated bytes of a call (1 .. %u)", bam::MAX_U);
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: prepare comes before the first front call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double t0 = now_s();
    static const bool one_stream = getenv("FADEHIP_BAM_BACK_STREAMS") && atoi(getenv("FADEHIP_BAM_BACK_STREAMS")) == 1;
    int rcs[4] = {0, 0, 0, 0};
    std::string errs[4];
    const bool with_out = !st->no_output;
    // lane 0 first on this thread when the lanes share a stream (lane 1 borrows it); the function attributes are set once, there
    if (with_out && (rcs[0] = bgzf_lane_ready(ctx, 0, one_stream))) return rcs[0];
    const double t_lane0 = now_s();
    std::vector<std::thread> th;
    auto side = [&](int slot_no, auto fn) {
        th.emplace_back([&, slot_no, fn] {
            if (hipSetDevice(ctx->device) != hipSuccess) { rcs[slot_no] = FADEHIP_E_HIP; errs[slot_no] = "hipSetDevice failed"; return; }
            if ((rcs[slot_no] = fn())) errs[slot_no] = fadehip_last_error(ctx);
        });
    };
    side(1, [&]() -> int {  // the second slot: a stream of its own
        Slot &s = ctx->slots[1];
        if (ctx->split_cus > 0 && !s.stream && !s.h_zb) s.stream = xcd_slice_stream(ctx, 0, ctx->split_cus);
        return ensure_slot(ctx, s);
    });
    if (with_out) side(2, [&]() -> int { return bgzf_lane_ready(ctx, 1, one_stream); });
    // this thread: the first slot (on the ctx's copy stream), the buffers
    int rc = 0;
    {
        Slot &s = ctx->slots[0];
        if (ctx->split_cus > 0 && !s.stream && !s.h_zb) {
            ctx->tail_cus_per_xcd = 0;
            s.stream = xcd_slice_stream(ctx, 0, ctx->split_cus);
        }
        if (!s.stream && !s.h_zb && ctx->copy_stream) s.stream = ctx->copy_stream;
        rc = ensure_slot(ctx, s);
    }
    const size_t carry_room = 65536;
    for (int q = 0; q < 2 && !rc; q++) {
        fadehip_bam_stream::Set &S = st->set[q];
        if (!(rc = reserve_roomy(ctx, S.u, call_bytes + carry_room + 256))) rc = reserve_pinned(ctx, S.h_counts, st->counts_bytes() + 16);
        if (!rc) rc = reserve_roomy(ctx, S.counts, st->counts_bytes());
    }
    // (annotated records are a few per cent longer than the call's; the members' bound is the compressor's own)
    const size_t out_est = call_bytes + call_bytes / 8;
    for (int q = 0; q < FADEHIP_BAM_CHUNKS && !rc && with_out; q++)
        rc = reserve_pinned(ctx, st->outbuf[q], st->stored ? (out_est / bgzf::STORE_BLOCK + 2) * bgzf::STORE_MEMBER : bgzf_out_cap(out_est, 32));
    const double t_mine = now_s();
    for (auto &t : th) t.join();
    if (getenv("FADEHIP_BAM_TRACE")) fprintf(stderr, "[fadehip trace] prepare: lane 0 %.3f ms, own part (slot 0, buffers) %.3f ms, the side threads %.3f ms more\n", (t_lane0 - t0) * 1e3, (t_mine - t_lane0) * 1e3, (now_s() - t_mine) * 1e3);
    if (rc) return rc;
    for (int q = 1; q < 4; q++)
        if (rcs[q]) return set_err(ctx, rcs[q], "bam stream: prepare: %s", errs[q].c_str());
    // the first copy, the first wait of every stream
    const double t1 = now_s();
    if (with_out && st->outbuf[0].p) {
        for (int q = 0; q < 2; q++) {
            fadehip_bam_stream::Set &S = st->set[q];
            hipStream_t sq = ctx->slots[q].stream;
            const size_t n = std::min(call_bytes, st->outbuf[q].cap);
            HIPCHK(ctx, hipMemcpyAsync(S.u.p, st->outbuf[q].p, n, hipMemcpyHostToDevice, sq));
            HIPCHK(ctx, hipMemsetAsync(S.counts.p, 0, sizeof(bam::ChunkCounts), sq));
            HIPCHK(ctx, hipMemcpyAsync(S.h_counts.p, S.counts.p, sizeof(bam::ChunkCounts), hipMemcpyDeviceToHost, sq));
        }
        for (int q = 0; q < 2; q++) HIPCHK(ctx, hipStreamSynchronize(ctx->slots[q].stream));
        for (int q = 0; q < 2; q++) {
            BgzfLane &l = ctx->bgzf[q];
            HIPCHK(ctx, hipMemcpyAsync(l.h_total, st->set[0].counts.p, 8, hipMemcpyDeviceToHost, l.stream));
            HIPCHK(ctx, hipEventRecord(l.done, l.stream));
            HIPCHK(ctx, hipEventSynchronize(l.done));
        }
    }
    if (getenv("FADEHIP_BAM_TRACE")) fprintf(stderr, "[fadehip trace] prepare: streams and buffers %.3f ms, first copies and waits %.3f ms\n", (t1 - t0) * 1e3, (now_s() - t1) * 1e3);
    return 0;
}

int fadehip_bam_front(fadehip_bam_stream *st, const void *members, size_t n_bytes, int last) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (n_bytes && !members) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (st->failed) return set_err(ctx, FADEHIP_E_STATE, "bam stream: an earlier call failed");
    if (st->ended) return set_err(ctx, FADEHIP_E_STATE, "bam stream: front after the last call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = bam_front_impl(st, (const uint8_t *)members, n_bytes, last, false);
    if (rc) {
        for (int q = 0; q < 2; q++)
            if (ctx->slots[q].stream) (void)hipStreamSynchronize(ctx->slots[q].stream);
        return bam_fail(st, rc);
    }
    return 0;
}

int fadehip_bam_front_raw(fadehip_bam_stream *st, const void *payload, size_t n_bytes, int last) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (n_bytes && !payload) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (st->failed) return set_err(ctx, FADEHIP_E_STATE, "bam stream: an earlier call failed");
    if (st->ended) return set_err(ctx, FADEHIP_E_STATE, "bam stream: front after the last call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = bam_front_impl(st, (const uint8_t *)payload, n_bytes, last, true);
    if (rc) {
        for (int q = 0; q < 2; q++)
            if (ctx->slots[q].stream) (void)hipStreamSynchronize(ctx->slots[q].stream);
        return bam_fail(st, rc);
    }
    return 0;
}

// the back half's first step for call k: the call is finished (sizes read, rewrite enqueued) and its bytes go to the
// compressor on lane k & 1, the members packed into the stream's pinned buffer k % FADEHIP_BAM_CHUNKS
static int bam_submit_back(fadehip_bam_stream *st, uint64_t k) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *o = &st->ring[k % FADEHIP_BAM_CHUNKS];
    int rc;
    CallTrace tr("back", k);
    if ((rc = bam_finish_call(st, k))) return rc;
    tr.mark("finish call");
    st->k_sub = k + 1;
    if (!o->bytes || st->no_output) return 0;
    const int lane = (int)(k & 1);
    // (FADEHIP_BAM_BACK_STREAMS=1: both lanes on one stream — one HSA queue fewer, but call k's members then cross PCIe
    // before call k + 1's compressor starts instead of beside it)
    static const bool one_stream = getenv("FADEHIP_BAM_BACK_STREAMS") && atoi(getenv("FADEHIP_BAM_BACK_STREAMS")) == 1;
    if ((rc = bgzf_lane_ready(ctx, lane, one_stream))) return rc;
    tr.mark("lane (stream)");
    BgzfLane &l = ctx->bgzf[lane];
    if (hipStreamWaitEvent(l.stream, o->ready, 0) != hipSuccess) return set_err(ctx, FADEHIP_E_HIP, "bam stream: hipStreamWaitEvent failed");
    PinBuf &ob = st->outbuf[k % FADEHIP_BAM_CHUNKS];
    if (st->stored) {
        // uncompressed BGZF: the members' sizes are known here; the kernel stores them straight into the pinned buffer
        const uint32_t nb = (uint32_t)((o->bytes + bgzf::STORE_BLOCK - 1) / bgzf::STORE_BLOCK);
        const size_t total = o->bytes + (size_t)nb * (bgzf::STORE_MEMBER - bgzf::STORE_BLOCK);
        if ((rc = reserve_pinned(ctx, ob, (size_t)nb * bgzf::STORE_MEMBER))) return rc;
        hipLaunchKernelGGL(bgzf::bgzf_store_kernel, dim3(nb), dim3(bgzf::STORE_WG), 0, l.stream, (const uint8_t *)o->o.p, (uint64_t)o->bytes, nb, ob.p);
        if (hipGetLastError() != hipSuccess || hipEventRecord(l.done, l.stream) != hipSuccess) return set_err(ctx, FADEHIP_E_HIP, "bam stream: storing the members failed");
        l.h_out = ob.p;
        *l.h_total = total;
        l.n_bytes = o->bytes;
        l.state = 1;
        return 0;
    }
    rc = bgzf_enqueue(ctx, lane, (const uint8_t *)o->o.p, o->bytes, bgzf_pick_geom(ctx), &ob);
    tr.mark("compressor enqueued");
    return rc;
}

int fadehip_bam_back(fadehip_bam_stream *st, const uint8_t **out, size_t *out_bytes) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!out || !out_bytes) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    *out_bytes = 0;
    const uint64_t k = st->k_back;
    fadehip_bam_stream::Out *o = &st->ring[k % FADEHIP_BAM_CHUNKS];
    bool next_waiting = false;
    {
        std::unique_lock<std::mutex> l(st->mu);
        if ((o->state == 0 && st->k_sub <= k) || st->failed) return set_err(ctx, FADEHIP_E_STATE, st->failed ? "bam stream: an earlier call failed" : "bam stream: no front call is waiting for back");
        next_waiting = st->k_front > k + 1 && st->ring[(k + 1) % FADEHIP_BAM_CHUNKS].state != 0;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = 0;
    // the call's last step (sizes read, rewrite enqueued) is taken here, beside the front half's work on the next call
    if (st->k_sub <= k && (rc = bam_submit_back(st, k))) return bam_fail(st, rc);
    // The call after this one, if its front half is through on the device: its compressor is enqueued now, so that it
    // starts the moment this call's has left the CUs — while this call's members cross PCIe and the caller gets them.
    if (next_waiting && st->k_sub == k + 1) {
        bool through;
        {
            fadehip_bam_stream::Set &S = st->set[(k + 1) & 1];
            std::lock_guard<std::mutex> pl(S.mu);
            through = S.k != k + 1 || !S.pending || hipStreamQuery(ctx->slots[(k + 1) & 1].stream) == hipSuccess;
        }
        if (through && (rc = bam_submit_back(st, k + 1))) return bam_fail(st, rc);
    }
    if (o->bytes && !st->no_output) {
        const int lane = (int)(k & 1);
        BgzfLane &l = ctx->bgzf[lane];
        if (st->stored) {
            if (hipEventSynchronize(l.done) != hipSuccess) return bam_fail(st, set_err(ctx, FADEHIP_E_HIP, "bam stream: storing the members failed"));
            l.state = 0;
            *out = l.h_out;
            *out_bytes = (size_t)*l.h_total;
        } else if ((rc = fadehip_bgzf_deflate_wait(ctx, lane, out, out_bytes))) return bam_fail(st, rc);
    } else if (o->ready) {
        (void)hipEventSynchronize(o->ready);
    }
    if (st->extract) {
        if (o->xready && hipEventSynchronize(o->xready) != hipSuccess) return bam_fail(st, set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the extract records failed"));
        st->last_x = o->xbytes ? st->xbuf[k % (FADEHIP_BAM_CHUNKS + 1)].p : nullptr;
        st->last_xbytes = o->xbytes;
        st->last_xrecs = o->xrecs;
        st->have_back = true;
    }
    {
        std::lock_guard<std::mutex> l(st->mu);
        o->state = 0;
        st->k_back++;
    }
    st->cv.notify_all();
    return 0;
}

int fadehip_bam_back_extract(fadehip_bam_stream *st, const uint8_t **recs, size_t *n_bytes, int64_t *n_records) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!recs || !n_bytes || !n_records) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *recs = nullptr;
    *n_bytes = 0;
    *n_records = 0;
    if (!st->extract) return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened without FADEHIP_BAM_EXTRACT");
    if (!st->have_back) return set_err(ctx, FADEHIP_E_STATE, "bam stream: back_extract comes after a back call");
    *recs = st->last_x;
    *n_bytes = st->last_xbytes;
    *n_records = st->last_xrecs;
    return 0;
}

int fadehip_bam_totals(fadehip_bam_stream *st, int64_t stats[8], int64_t *n_records, int64_t *n_oversize) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    std::lock_guard<std::mutex> l(st->mu);
    if (stats) memcpy(stats, st->stats, sizeof st->stats);
    if (n_records) *n_records = st->n_records;
    if (n_oversize) *n_oversize = st->n_oversize;
    return 0;
}

int fadehip_bam_ejected(fadehip_bam_stream *st, int64_t *n_ejected) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    if (!n_ejected) return set_err(st->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> l(st->mu);
    *n_ejected = st->n_ejected;
    return 0;
}

void fadehip_bam_close(fadehip_bam_stream *st) {
    if (!st) return;
    {
        std::lock_guard<std::mutex> l(st->mu);
        st->closing = true;
    }
    st->cv.notify_all();
    fadehip_ctx *ctx = st->ctx;
    if (getenv("FADEHIP_BAM_PROF"))
        fprintf(stderr, "[fadehip bam] %llu front calls: A enqueue (copy / inflate, frame, pack count) %.3f s, wait for A %.3f | B enqueue (pack, run, tag sizes) %.3f | "
                        "C (wait for B, rewrite enqueued; taken by back or front) %.3f | segments walked again %lld\n", (unsigned long long)st->k_front, st->t_inflate, st->t_frame, st->t_run, st->t_tags,
                (long long)st->n_redone);
    (void)hipSetDevice(ctx->device);
    for (int q = 0; q < 2; q++) {
        if (ctx->slots[q].stream) (void)hipStreamSynchronize(ctx->slots[q].stream);
        ctx->slots[q].device_only = false;
        ctx->slots[q].wide_all = false;
        if (ctx->slots[q].state == 2) ctx->slots[q].state = 0;  // (a call that was never finished: nothing of it is handed out)
    }
    for (BgzfLane &l : ctx->bgzf)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    release(st->names_text);
    release(st->names_off);
    for (auto &S : st->set) {
        for (DevBuf *b : {&S.comp, &S.blocks, &S.status, &S.ticket, &S.u, &S.seg, &S.slots, &S.rec_off, &S.info, &S.sent_of, &S.art_of, &S.out_size, &S.blk32,
                          &S.blk64, &S.counts, &S.ex_size, &S.ex_blk, &S.ej_head, &S.ej_blk, &S.ej_grp})
            release(*b);
        release(S.h_blocks);
        release(S.h_counts);
    }
    for (auto &ob : st->outbuf) release(ob);
    for (auto &xb : st->xbuf) release(xb);
    for (auto &o : st->ring) {
        release(o.o);
        release(o.x);
        if (o.xready) (void)hipEventDestroy(o.xready);
        if (o.ready) (void)hipEventDestroy(o.ready);
    }
    delete st;
}

int fadehip_stats_allreduce(fadehip_ctx *const *ctxs, int n_ctx, int64_t *counters, int count) {
    if (!ctxs || n_ctx <= 0 || !counters || count <= 0) return set_err(nullptr, FADEHIP_E_INVALID, "bad arguments");
    fadehip_ctx *c0 = ctxs[0];
    std::vector<int> devs(n_ctx);
    for (int k = 0; k < n_ctx; k++) {
        if (!ctxs[k]) return set_err(c0, FADEHIP_E_INVALID, "ctx %d is NULL", k);
        devs[k] = ctxs[k]->device;
    }
    std::vector<ncclComm_t> comms(n_ctx);
    ncclResult_t nr = ncclCommInitAll(comms.data(), n_ctx, devs.data());
    if (nr != ncclSuccess) return set_err(c0, FADEHIP_E_RCCL, "ncclCommInitAll failed: %s", ncclGetErrorString(nr));
    std::vector<void *> bufs(n_ctx, nullptr);
    int rc = 0;
    for (int k = 0; k < n_ctx && !rc; k++) {
        if (hipSetDevice(devs[k]) != hipSuccess || hipMalloc(&bufs[k], sizeof(int64_t) * count) != hipSuccess ||
            hipMemcpy(bufs[k], counters + (size_t)k * count, sizeof(int64_t) * count, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c0, FADEHIP_E_HIP, "staging counters on device %d failed", devs[k]);
    }
    if (!rc) {
        ncclGroupStart();
        for (int k = 0; k < n_ctx; k++) {
            (void)hipSetDevice(devs[k]);
            nr = ncclAllReduce(bufs[k], bufs[k], count, ncclInt64, ncclSum, comms[k], ctxs[k]->slots[0].stream);
            if (nr != ncclSuccess) rc = set_err(c0, FADEHIP_E_RCCL, "ncclAllReduce failed: %s", ncclGetErrorString(nr));
        }
        nr = ncclGroupEnd();
        if (nr != ncclSuccess && !rc) rc = set_err(c0, FADEHIP_E_RCCL, "ncclGroupEnd failed: %s", ncclGetErrorString(nr));
    }
    for (int k = 0; k < n_ctx; k++) {
        (void)hipSetDevice(devs[k]);
        if (!rc) {
            if (hipStreamSynchronize(ctxs[k]->slots[0].stream) != hipSuccess ||
                hipMemcpy(counters + (size_t)k * count, bufs[k], sizeof(int64_t) * count, hipMemcpyDeviceToHost) != hipSuccess)
                rc = set_err(c0, FADEHIP_E_HIP, "reading reduced counters from device %d failed", devs[k]);
        }
        if (bufs[k]) (void)hipFree(bufs[k]);
        ncclCommDestroy(comms[k]);
    }
    return rc;
}

int fadehip_stats_allreduce_rank(fadehip_ctx *ctx, int rank, int n_ranks, const char *id_path, int64_t *counters, int count) {
    if (!ctx || !id_path || !counters || count <= 0 || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return set_err(ctx, FADEHIP_E_INVALID, "bad arguments");
    if (n_ranks == 1) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    if (rank == 0) {
        ncclResult_t nr = ncclGetUniqueId(&id);
        if (nr != ncclSuccess) return set_err(ctx, FADEHIP_E_RCCL, "ncclGetUniqueId failed: %s", ncclGetErrorString(nr));
        const std::string tmp = std::string(id_path) + ".tmp";
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(&id, 1, sizeof id, f) != sizeof id) { if (f) fclose(f); return set_err(ctx, FADEHIP_E_INVALID, "cannot write %s", tmp.c_str()); }
        fclose(f);
        if (rename(tmp.c_str(), id_path) != 0) return set_err(ctx, FADEHIP_E_INVALID, "cannot rename %s", tmp.c_str());
    } else {
        bool got = false;
        for (int tries = 0; tries < 60000 && !got; tries++) {
            if (FILE *f = fopen(id_path, "rb")) {
                got = fread(&id, 1, sizeof id, f) == sizeof id;
                fclose(f);
            }
            if (!got) {
                struct timespec ts = {0, 1000000};
                nanosleep(&ts, nullptr);
            }
        }
        if (!got) return set_err(ctx, FADEHIP_E_RCCL, "rank %d: no ncclUniqueId appeared in %s", rank, id_path);
    }
    ncclComm_t comm;
    ncclResult_t nr = ncclCommInitRank(&comm, n_ranks, id, rank);
    if (nr != ncclSuccess) return set_err(ctx, FADEHIP_E_RCCL, "ncclCommInitRank failed: %s", ncclGetErrorString(nr));
    void *buf = nullptr;
    int rc = 0;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipMalloc(&buf, sizeof(int64_t) * count) != hipSuccess ||
        hipMemcpy(buf, counters, sizeof(int64_t) * count, hipMemcpyHostToDevice) != hipSuccess)
        rc = set_err(ctx, FADEHIP_E_HIP, "staging counters failed");
    if (!rc) {
        nr = ncclAllReduce(buf, buf, count, ncclInt64, ncclSum, comm, st);
        if (nr != ncclSuccess) rc = set_err(ctx, FADEHIP_E_RCCL, "ncclAllReduce failed: %s", ncclGetErrorString(nr));
    }
    if (!rc && (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(counters, buf, sizeof(int64_t) * count, hipMemcpyDeviceToHost) != hipSuccess))
        rc = set_err(ctx, FADEHIP_E_HIP, "reading the reduced counters failed");
    if (buf) (void)hipFree(buf);
    ncclCommDestroy(comm);
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

}  // extern "C"
