// fadehip_host.hpp — what the host units of libfadehip.so share (internal; declarations only, no kernel).
// The context with its slots and lanes, the buffer types, HIPCHK, and the helpers of one unit that another one calls:
// everything in namespace fadehip::host, which has hidden visibility, so that none of it shows in the library's symbol
// table.  A unit reaches into another through this header and in no other way ("Translation units").
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/fadehip.h"
#include "fadehip_types.hpp"

namespace fadehip {
struct StatsWork;     // sw_stats.hpp
struct StatsScoring;
namespace host __attribute__((visibility("hidden"))) {

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

// upload keeps the reads whose cigar.alignedLength exceeds this (spliced reads, large deletions) for plan_run
constexpr int64_t WIDE_MIN_SPAN = 1024;

struct Slot {
    hipStream_t stream = nullptr;
    // The score pass fills every wave slot it may use for ~0.8 ms; the small, latency-bound kernels of the other
    // slots (gate, selection, plan, pass 2, traceback) would wait behind it for a slot each.  So the score pass runs
    // on a stream whose CU mask leaves a few CUs (one per XCD by default) to everything else.
    hipStream_t score_stream = nullptr;
    std::vector<uint32_t> score_mask;  // its CU mask (empty: none)
    // The early order of a run (enqueue_run): the alignment array and rs leave for the host right behind the score pass, on
    // the score stream, while pass 2 and the gather of the entries it wrote (patch_gather_kernel) run on `stream`; the copies
    // are joined into `stream` before the one copy that ends the run (the patch block, which carries the counter block too).  The A/B variants (ctx->early_tail) copy on `stream` and run pass 2 on
    // this stream instead, forked from the score pass's end and joined back; made when a run first takes that order.
    hipStream_t tail_stream = nullptr;
    bool tail_tried = false;
    bool early = false;        // the run in flight took the early order
    DevBuf patch;              // PatchHead | the run's counter block (ZB_STRIDE) | PatchEntry [patch_cap]
    PinBuf h_patch;            // its pinned copy: the head, the counters and the first patch_sent entries come with the run
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
    // Two such blocks, used by alternate runs: a run zeroes the OTHER block (behind the copy that ends it; in the early order
    // in its gather kernel), so the next run's gate follows its upload directly instead of a fill (zb_next_clean: that fill was enqueued and nothing has touched the
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
    uint8_t *h_zb = nullptr;  // pinned copy of zblock, filled by the D2H that ends a run (early order: by finish_run, from h_patch)
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
    DevBuf scratch;              // fadehip_report_batch: sw_stats_kernel's rows of its multi-strip pairs
    std::vector<uint8_t> index_host;  // fadehip_index_batch: the arrays *out points into, until the lane's next call
};

}  // namespace host
}  // namespace fadehip

struct fadehip_ctx {
    int device = 0;
    fadehip_params prm;
    fadehip::ScoreTab sc;
    std::string err;
    std::mutex err_mu;
    fadehip::host::Slot slots[FADEHIP_NUM_SLOTS];
    // genome
    fadehip::host::DevBuf genome, contig_len, contig_base;
    fadehip::host::DevBuf l1_q, l1_r, l1_qn, l1_rn, l1_bad, l1_work, l1_aln;  // level 1 (fadehip_sw_batch): kept between calls, grow only
    // fadehip_sw_stats_batch: its own stream and buffers (kept between calls, grow only), so that it leaves the slots alone
    hipStream_t stats_stream = nullptr;
    fadehip::host::DevBuf st_q, st_r, st_work, st_out, st_scratch;
    std::mutex stats_mu;
    fadehip::host::BatchLane batch;  // the three record-batch entry points share it: they leave the slots and the stats lane alone, not each other
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
    bool score_diag = true;      // ... with the drift following the row too where that frame's own bound holds (g8_pick; FADEHIP_SCORE_DIAG=0: never)
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
    fadehip::host::BgzfLane bgzf[FADEHIP_BGZF_LANES];
    fadehip::host::InflateLane inf;
    bool bgzf_ready = false;           // the compressor's LDS size has been declared to the runtime
    int bgzf_geom_fixed = 0;           // FADEHIP_BGZF_GEOM: 32 / 64 (0: by the ratio of the previous call)
    double bgzf_last_ratio = 0;        // compressed / raw bytes of the ctx's previous compression
    std::map<uint64_t, int> resident;  // (class, mode, LDS bytes) -> waves of that kernel the device holds at once
    std::mutex resident_mu;
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fadehip::host::set_err(ctx, e_ == hipErrorOutOfMemory ? FADEHIP_E_NOMEM : FADEHIP_E_HIP,      \
                           "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace fadehip {
namespace host __attribute__((visibility("hidden"))) {

// ---- fadehip_ctx.hip: the error channel and memory
int set_err(fadehip_ctx *ctx, int code, const char *fmt, ...);
Layout batch_layout(int64_t n, int64_t n_cig, int64_t n_seq);
int reserve(fadehip_ctx *ctx, DevBuf &b, size_t bytes);
int reserve_pinned(fadehip_ctx *ctx, PinBuf &b, size_t bytes);
int reserve_roomy(fadehip_ctx *ctx, DevBuf &b, size_t bytes);
void release(DevBuf &b);
void release(PinBuf &b);

// ---- fadehip.hip: the alignment engine
int build_score_tab(fadehip_ctx *ctx, const fadehip_params &p, ScoreTab &sc);
hipError_t upload_ascii_code(hipStream_t st);
hipStream_t xcd_slice_stream(fadehip_ctx *ctx, int lo, int hi);
int ensure_slot(fadehip_ctx *ctx, Slot &s);
void bound_counted_batch(Slot &s, uint32_t n_sent, uint32_t l_seq_min, uint32_t l_seq_max, uint32_t n_long_q, int64_t span_max);
int plan_run(fadehip_ctx *ctx, Slot &s);
int enqueue_run(fadehip_ctx *ctx, Slot &s);
int finish_run(fadehip_ctx *ctx, Slot &s, int slot);
int sw_stats_long_blocks(size_t n_long, int long_max_lr, size_t *row_bytes);
int enqueue_sw_stats(fadehip_ctx *ctx, hipStream_t st, const StatsWork *d_work, const size_t cls_begin[6], const uint8_t *d_q, const uint8_t *d_r,
                     fadehip_sw_stats_result *d_out, void *scratch, int long_max_lr, int long_blocks, const StatsScoring &sc);

// ---- fadehip_bgzf.hip: the inflater and the compressor lanes
bool scan_bgzf_members(const uint8_t *p, size_t n, std::vector<bgzf::InflateBlock> &blocks, size_t *consumed, uint64_t *total_out, std::string &msg);
const char *inflate_error_name(uint32_t e);
int launch_inflate(fadehip_ctx *ctx, hipStream_t st, const bgzf::InflateArgs &a);
int bgzf_lane_ready(fadehip_ctx *ctx, int lane, bool one_stream = false);
int bgzf_pick_geom(const fadehip_ctx *ctx);
size_t bgzf_out_cap(size_t n_bytes, int geom);
int bgzf_enqueue(fadehip_ctx *ctx, int lane, const uint8_t *d_src, size_t n_bytes, int geom, PinBuf *host_out = nullptr);
size_t bgzf_store_cap(size_t n_bytes);
int bgzf_store_enqueue(fadehip_ctx *ctx, int lane, const uint8_t *d_src, size_t n_bytes, PinBuf &ob);
struct BgzfGeometry {
    uint32_t block = 0;                    // uncompressed bytes per member (the last may hold fewer)
    const uint64_t *member_off = nullptr;  // device: member k's offset among the call's members; nullptr: k * member_stride
    const uint64_t *behind_ptr = nullptr;  // device: the members' total; nullptr: `behind`
    uint64_t member_stride = 0, behind = 0;
};
BgzfGeometry bgzf_lane_geometry(const fadehip_ctx *ctx, int lane, bool stored);

}  // namespace host
}  // namespace fadehip
