// fadehip_ctx.hip — C ABI (include/fadehip.h): the context, its memory and the error channel.
// fadehip_create / _destroy / _sync, the staging-memory and batch-block calls, the reserve / release helpers every unit
// uses, and the two stats all-reduces (the only use of RCCL).  No kernel header is included here, so an edit here compiles
// no kernel: they are launched by fadehip.hip, fadehip_bgzf.hip and fadehip_bam.hip, reached through fadehip_host.hpp.
// No CPU fallback lives here: every entry point either runs the HIP path or returns an error.
#include "fadehip_host.hpp"
#include <rccl/rccl.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>
#include <unordered_map>

using namespace fadehip;
using namespace fadehip::host;

namespace {

thread_local std::string g_err = "";
thread_local const fadehip_ctx *g_err_ctx = nullptr;

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

}  // namespace

namespace fadehip::host {

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

}  // namespace fadehip::host

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
    if (const char *kv = getenv("FADEHIP_SCORE_DIAG")) ctx->score_diag = atoi(kv) != 0;
    if (const char *kv = getenv("FADEHIP_EARLY_COPY")) ctx->early_copy = atoi(kv) != 0;
    if (const char *kv = getenv("FADEHIP_EARLY_TAIL")) ctx->early_tail = strcmp(kv, "masked") == 0 ? 1 : strcmp(kv, "plain") == 0 ? 2 : 0;
    if (const char *kv = getenv("FADEHIP_PATCH_CAP")) ctx->patch_cap = std::max(0, std::min(atoi(kv), 1 << 20));
    ctx->debug = getenv("FADEHIP_DEBUG") != nullptr;
    // (everything the library enqueues goes to streams of its own: the null stream would be one more HSA queue, i.e. one
    // more 173 MB context-save area in host memory, for two copies)
    if (hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        upload_ascii_code(ctx->copy_stream) != hipSuccess) {
        set_err(ctx, FADEHIP_E_HIP, "hipMemcpyToSymbol failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(FADEHIP_E_HIP);
    }
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
    for (DevBuf *b : {&ctx->batch.in, &ctx->batch.meta, &ctx->batch.work, &ctx->batch.out, &ctx->batch.scratch}) release(*b);
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

int fadehip_sync(fadehip_ctx *ctx) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    for (int k = 0; k < FADEHIP_NUM_SLOTS; k++)
        if (ctx->slots[k].stream) HIPCHK(ctx, hipStreamSynchronize(ctx->slots[k].stream));
    return 0;
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
