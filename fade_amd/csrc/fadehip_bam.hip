// fadehip_bam.hip — BAM records on the device: host side of bam_device.hpp.
// The record-batch lane (fadehip_clip_batch, fadehip_eject_batch, fadehip_extract_batch, fadehip_tags_batch) and the file
// path, struct fadehip_bam_stream with every fadehip_bam_* call.  The file path drives a slot's run and the BGZF lanes
// through fadehip_host.hpp.
#include "fadehip_host.hpp"
#include "bam_device.hpp"
#include "bam_from_tags.hpp"
#include "bam_names.hpp"
#include "bam_mates.hpp"
#include "bam_calmd.hpp"
#include "bam_report.hpp"
#include "bam_resort.hpp"
#include "bam_index.hpp"
#include "bam_recstore.hpp"
#include "bam_sortwin.hpp"
#include "bam_intervals.hpp"
#include "host/bai_build.hpp"
#include "host/csi_build.hpp"
#include "host/recstore_host.hpp"
#include "host/bed_lite.hpp"
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>

using namespace fadehip;
using namespace fadehip::host;

// A CSI geometry as the calls take it (fadehip_index_batch_csi, fadehip_bam_index_geometry, fadehip_recstore_index_geometry);
// depth 0 stands for "none": BAI's tree, limit and message.
struct IndexGeometry {
    int32_t min_shift = 0, depth = 0;
    uint64_t limit() const { return 1ull << (min_shift + 3 * depth); }
    static bool valid(int32_t min_shift, int32_t depth) { return min_shift >= 4 && depth >= 1 && depth <= 8 && min_shift + 3 * depth <= 32; }
};

// A set of read names on the device (bam_names.hpp).  The host's part: the buffers, bounds on what the kernels in flight may
// have added (exact values as of the last wait, plus the bounds of every launch since), and growth.  Every launch that names
// the set's buffers is enqueued under `mu`, and growth — under `mu` too — begins with a wait for the whole device: so a
// rehash, or the arena's move to a larger buffer, never runs beside an insert or a look-up of the same set, on whichever
// stream those were enqueued (the two slots' streams of a file path, the record-batch lane).
struct fadehip_nameset {
    fadehip_ctx *ctx = nullptr;
    std::mutex mu;
    DevBuf table, arena, ctrl;
    uint64_t slots = 0;
    uint64_t count_ub = 0, used_ub = 0;  // bounds on ctrl[NS_COUNT], ctrl[NS_USED] once everything enqueued has run
    uint32_t hash_bits = 64;
    PinBuf h_ctrl;
    // a name set; the mate map (bam_mates.hpp) is the same buffers with one more key byte and a fourth counter
    uint32_t key_extra = 0;
    const char *what = "nameset";
};

// The mate map of fadehip_mateset_* / fadehip_mates_fix_batch: the name set's host part as it is, over bam_mates.hpp's entries.
struct fadehip_mateset {
    fadehip_nameset core;
};

// A store of records on the device (bam_recstore.hpp).  The host's part: the arena and the item arrays with what has been
// handed out of them — exact numbers, since every call's byte range and item range are reserved here, in call order, before
// anything of the call is launched — growth, the sort's arrays, and the drain's cursor and buffers.  As with the name set,
// every launch that names the store's buffers is enqueued under `mu`, and growth begins with a wait for the whole device.
struct fadehip_recstore {
    fadehip_ctx *ctx = nullptr;
    std::mutex mu;
    DevBuf arena, key, off, size;
    uint64_t first_bytes = 0;         // FADEHIP_RECSTORE_BYTES: the first arena
    uint64_t used = 0, n_items = 0;   // arena bytes and items handed out
    uint64_t item_cap = 0;
    bool sorted = false;              // fadehip_recstore_sort has run: nothing is added any more
    DevBuf sort_arr;                  // the sort's arrays (recstore_sort_layout) and its ctl
    bam::ResortArgs ra;
    std::vector<uint64_t> h_dst;      // [n_items + 1] the records' offsets in final order
    uint64_t cursor = 0;              // records drained so far
    DevBuf stage, at, app;            // a drain's bytes and offsets; add_batch's sizes, bases and counts
    DevBuf ix_work, ix_ctl, ix_out;
    IndexGeometry ix_geo;             // fadehip_recstore_index_geometry: the drains' entries are a CSI's (depth 0: a BAI's)
    bool drained = false;             // a drain has handed out records: the geometry stays
    bam::IndexCtl ixc;                // a drain's index ctl as it crosses (a member: the copy may outlive a call that fails)
    PinBuf h_out;                     // what a drain hands out: the raw records or the members
    std::vector<uint8_t> h_ix;        // the arrays *idx points into, until the next drain
    // the sorted main output (bam_sortwin.hpp): none of it is set on a store that only collects extract records
    bool budget_set = false;          // fadehip_recstore_set_budget has been called
    uint64_t budget = 0;              // the most cost(used, n_items) may be
    bool measuring = false, over = false;  // fadehip_recstore_measure .. _reset; a call took the cost over the budget meanwhile
    recstore::BucketLayout lay;       // measure's buckets
    bool have_table = false;
    DevBuf table, lay_dev;            // bytes [n_buckets] | records [n_buckets]; first [n_ref] | nb [n_ref]
    uint64_t win_lo = 0, win_hi = ~(uint64_t)0;  // fadehip_recstore_set_window
    uint64_t n_reset = 0;             // reset records (written zero-filled, keyed as unmapped) among what STORE_OUTPUT streams wrote or measured since create / reset
};

// A set of intervals on the device (bam_intervals.hpp).  The host's part: the contigs' names and their ids, the raw items
// as add brought them (exact numbers: a call's items count only once its key kernel has found no bad interval), growth, and
// behind seal the three sealed arrays and the names on the device — from then on nothing of the set changes, so the kernels
// that read it (the overlap query, the report's on any stream) take no lock.
struct fadehip_intervals {
    fadehip_ctx *ctx = nullptr;
    std::mutex mu;
    std::vector<std::string> names;
    std::map<std::string, int32_t> ids;
    DevBuf key, end32, idx;            // the raw items
    uint64_t first_cap = 0, cap = 0, n = 0;  // FADEHIP_INTERVALS_CAP; items the arrays hold; items added
    bool sealed = false;
    DevBuf start, maxend, chrom_first;  // sealed
    DevBuf name_bytes, name_off;        // sealed: the names as report_repeats_kernel looks them up
    DevBuf stage;                       // a call's arrays on the device (add, overlap_batch)
};

namespace {

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
// the bytes to `out`; size_per_block 16: the size kernel, too, takes sixteen lanes per element.  out_off gets the offsets — with off_first also when out is too small (clip says what it would have
// taken; extract does not).  No bytes: no second half (extract's rule; clip never gets there, a record leaves with >= 36).
template <class Args>
int size_then_write(fadehip_ctx *ctx, BatchLane &L, Args &a, size_t cnt, void (*size_kernel)(Args), void (*write_kernel)(Args),
                    const char *what, bool off_first, std::vector<uint64_t> &off, uint8_t *out, int64_t out_cap, int64_t *out_off, unsigned size_per_block = 256u) {
    hipStream_t st = L.stream;
    a.out_size = (uint32_t *)L.work.p;
    a.out = nullptr;
    hipLaunchKernelGGL(size_kernel, dim3(((unsigned)cnt + size_per_block - 1u) / size_per_block), dim3(256), 0, st, a);
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

// the genome on the device as bam_calmd.hpp's kernels take it
bam::GenomeRef genome_ref(const fadehip_ctx *ctx) {
    bam::GenomeRef g;
    g.nib = (const uint8_t *)ctx->genome.p;
    g.contig_len = (const int64_t *)ctx->contig_len.p;
    g.contig_base = (const uint64_t *)ctx->contig_base.p;
    g.n_contigs = ctx->n_contigs;
    return g;
}

bam::CalmdWriteArgs calmd_write_args(const fadehip_ctx *ctx, const DevBuf &fix) {
    bam::CalmdWriteArgs w;
    w.gen = genome_ref(ctx);
    w.cfix = (const bam::CalmdFix *)fix.p;
    return w;
}

// ---- the name set (bam_names.hpp): what a launch names of it, its growth
bam::NameSetRef nameset_ref(const fadehip_nameset *s) {
    bam::NameSetRef r;
    r.table = (unsigned long long *)s->table.p;
    r.mask = s->slots - 1;
    r.arena = (uint8_t *)s->arena.p;
    r.arena_cap = s->arena.cap;
    r.ctrl = (unsigned long long *)s->ctrl.p;
    r.hash_bits = s->hash_bits;
    return r;
}

// What the set's kernels have left in ctrl, once nothing of the set runs any more (the caller holds s->mu): waits for the
// whole device, since the set's kernels may be on any of the ctx's streams.  A raised error flag fails the call.
int nameset_settle(fadehip_nameset *s, hipStream_t q) {
    fadehip_ctx *ctx = s->ctx;
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpyAsync(s->h_ctrl.p, s->ctrl.p, 32, hipMemcpyDeviceToHost, q));
    HIPCHK(ctx, hipStreamSynchronize(q));
    const unsigned long long *c = (const unsigned long long *)s->h_ctrl.p;
    if (c[bam::NS_ERR]) return set_err(ctx, FADEHIP_E_STATE, "%s: the %s was full during an insert (names may be missing: the set cannot be used)", s->what, (c[bam::NS_ERR] & bam::NS_ERR_ARENA) ? "arena" : "table");
    s->used_ub = c[bam::NS_USED];
    s->count_ub = c[bam::NS_COUNT];
    return 0;
}

// Room for a launch that adds at most n_new names of at most bytes_new arena bytes, made before it is enqueued on q (the
// caller holds s->mu).  The bounds of the launches so far usually say that there is room; when they do not, the device is
// waited for, the true numbers are read, and only if those do not leave room either the set grows — to `ahead` launches of
// this size, so that a file path does not come here with every call.  The insert kernel thus never finds the table (load
// at most 1/2 after the add) or the arena full.
int nameset_room(fadehip_nameset *s, hipStream_t q, uint64_t n_new, uint64_t bytes_new, uint64_t ahead) {
    fadehip_ctx *ctx = s->ctx;
    const auto fits = [&] { return 2 * (s->count_ub + n_new) <= s->slots && s->used_ub + bytes_new <= (uint64_t)s->arena.cap; };
    int rc;
    if (!fits()) {
        if ((rc = nameset_settle(s, q))) return rc;
        if (s->used_ub + bytes_new > (uint64_t)s->arena.cap) {  // the arena moves: offsets stay what they are
            const uint64_t want = s->used_ub + ahead * bytes_new;
            if (want > bam::NS_OFF_MASK) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "%s: more than 2^40 bytes of names", s->what);
            DevBuf nb;
            if ((rc = reserve(ctx, nb, (size_t)want))) return rc;
            if (s->used_ub && (hipMemcpyAsync(nb.p, s->arena.p, (size_t)s->used_ub, hipMemcpyDeviceToDevice, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)) {
                release(nb);
                return set_err(ctx, FADEHIP_E_HIP, "%s: moving the arena failed", s->what);
            }
            release(s->arena);
            s->arena = nb;
        }
        if (2 * (s->count_ub + n_new) > s->slots) {  // the table is hashed again into a larger one
            uint64_t slots = s->slots;
            while (slots < 2 * (s->count_ub + ahead * n_new)) slots <<= 1;
            if (slots > ((uint64_t)1 << 36)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "%s: more than 2^35 names", s->what);
            DevBuf nt;
            if ((rc = reserve(ctx, nt, 8 * (size_t)slots))) return rc;
            bam::NameRehashArgs ra;
            ra.old_table = (const unsigned long long *)s->table.p;
            ra.old_slots = s->slots;
            const DevBuf old = s->table;
            s->table = nt;
            s->slots = slots;
            ra.s = nameset_ref(s);
            ra.key_extra = s->key_extra;
            hipError_t e = hipMemsetAsync(nt.p, 0, 8 * (size_t)slots, q);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(bam::bam_names_rehash_kernel, dim3((unsigned)((ra.old_slots + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK)), dim3(bam::TAG_BLOCK), 0, q, ra);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(s->h_ctrl.p, s->ctrl.p, 24, hipMemcpyDeviceToHost, q);
            if (e == hipSuccess) e = hipStreamSynchronize(q);
            if (e != hipSuccess || ((const unsigned long long *)s->h_ctrl.p)[bam::NS_ERR]) {
                (void)hipStreamSynchronize(q);
                s->table = old;  // (the old table is whole: the rehash only read it)
                s->slots = ra.old_slots;
                release(nt);
                return set_err(ctx, FADEHIP_E_HIP, "%s: hashing the table again failed%s%s", s->what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
            }
            DevBuf o2 = old;
            release(o2);
        }
    }
    s->count_ub += n_new;
    s->used_ub += bytes_new;
    return 0;
}

// A new set's buffers, cleared.  env_slots: the first table's size (at least 16, rounded up to a power of two); env_bits:
// 0 .. 64, the hash is cut to its low bits (0: every key collides with every other).
int nameset_init(fadehip_ctx *ctx, fadehip_nameset *s, const char *env_slots, const char *env_bits) {
    s->ctx = ctx;
    uint64_t want = 65536;
    if (const char *e = getenv(env_slots)) want = (uint64_t)std::max<long long>(16, std::min<long long>(atoll(e), 1ll << 32));
    s->slots = 16;
    while (s->slots < want) s->slots <<= 1;
    if (const char *e = getenv(env_bits)) s->hash_bits = (uint32_t)std::max(0, std::min(64, atoi(e)));
    int rc;
    if ((rc = reserve(ctx, s->table, 8 * (size_t)s->slots)) || (rc = reserve(ctx, s->arena, 65536)) || (rc = reserve(ctx, s->ctrl, 256)) ||
        (rc = reserve_pinned(ctx, s->h_ctrl, 64)))
        return rc;
    // (on the ctx's copy stream: the null stream would be one more queue to set up and to give back)
    if (hipMemsetAsync(s->table.p, 0, 8 * (size_t)s->slots, ctx->copy_stream) != hipSuccess || hipMemsetAsync(s->ctrl.p, 0, 256, ctx->copy_stream) != hipSuccess ||
        hipStreamSynchronize(ctx->copy_stream) != hipSuccess)
        return set_err(ctx, FADEHIP_E_HIP, "%s: clearing the table failed", s->what);
    return 0;
}

void nameset_release(fadehip_nameset *s) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    release(s->table);
    release(s->arena);
    release(s->ctrl);
    release(s->h_ctrl);
}

// the arguments the set's kernels take of a record-batch call behind batch_upload
bam::NameArgs nameset_batch_args(const fadehip_nameset *s, BatchLane &L, int32_t n) {
    bam::NameArgs a;
    memset(&a, 0, sizeof a);
    a.s = nameset_ref(s);
    a.u = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)L.meta.p;
    a.n = (uint32_t)n;
    return a;
}

}  // namespace

extern "C" {

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

// fadehip_clip_batch, then NM and MD of the records that leave hard-clipped recomputed against the uploaded genome
// (bam_calmd.hpp): the plan kernel in the place of the size kernel, the write kernel replacing what it planned.
int fadehip_calmd_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                        const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap, int64_t *out_off, uint8_t *updated) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || !rec_off || !out_off || (n > 0 && (!recs || !rs || !trim_left || !trim_right || !updated)) || out_cap < 0 || (out_cap > 0 && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (ctx->n_contigs == 0) return set_err(ctx, FADEHIP_E_STATE, "fadehip_genome_upload has not been called");
    if (n == 0) {
        out_off[0] = 0;
        return 0;
    }
    const auto trims = [&](int32_t k) { return trim_left[k] < 0 || trim_right[k] < 0 ? set_err(ctx, FADEHIP_E_INVALID, "record %d: negative trim length", k) : 0; };
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, trims))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | out_off [n + 1] u64 | fix [n] CalmdFix | trim_l [n] u32 | trim_r [n] u32 | rs [n] u8;  work: out_size [n] u32
    static_assert(sizeof(bam::CalmdFix) % 8 == 0, "the fix array keeps what lies behind it aligned");
    const size_t m_out = 8 * ((size_t)n + 1), m_fix = 2 * m_out, m_tl = m_fix + sizeof(bam::CalmdFix) * (size_t)n, m_tr = m_tl + 4 * (size_t)n, m_rs = m_tr + 4 * (size_t)n;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_rs + (size_t)n + 8, 4 * (size_t)n, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tl, trim_left, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tr, trim_right, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    bam::CalmdArgs a;
    memset(&a, 0, sizeof a);
    a.g = genome_ref(ctx);
    a.u = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.rs = meta + m_rs;
    a.trim_l = (const uint32_t *)(meta + m_tl);
    a.trim_r = (const uint32_t *)(meta + m_tr);
    a.fix = (bam::CalmdFix *)(meta + m_fix);
    a.out_off = (const uint64_t *)(meta + m_out);
    std::vector<int64_t> ooff((size_t)n + 1);
    if ((rc = size_then_write(ctx, L, a, (size_t)n, bam::calmd_batch_plan_kernel, bam::calmd_batch_write_kernel, "clipped", false, off, out, out_cap, ooff.data(), 16u))) return rc;
    std::vector<bam::CalmdFix> fix((size_t)n);
    HIPCHK(ctx, hipMemcpyAsync(fix.data(), a.fix, sizeof(bam::CalmdFix) * (size_t)n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    for (int32_t k = 0; k < n; k++) updated[k] = (uint8_t)fix[(size_t)k].state;
    for (int32_t k = 0; k <= n; k++) out_off[k] = ooff[(size_t)k];
    return 0;
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

// ---- `fade stats` / `fade stats-clip` over records the caller brings (bam_report.hpp)
namespace {

// what a failed report call says of the record the stage named (RepCtl::bad)
int report_bad(fadehip_ctx *ctx, unsigned long long bad, long long first_record) {
    const long long rec = first_record + (long long)(0xffffffffu - (uint32_t)(bad >> 8));
    const uint32_t kind = (uint32_t)(bad & 0xffu);
    if (kind == bam::RP_BAD_LONG)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "report: record %lld: a piece of as / ar is longer than %d bytes", rec, FADEHIP_MAX_LONG_QUERY);
    const char *what = kind == bam::RP_BAD_AUX         ? "its aux area is not whole fields"
                       : kind == bam::RP_BAD_SIDE      ? "rs names a side of am that is not name,pos,cigar with pos in int32"
                       : kind == bam::RP_BAD_ART_TAGS  ? "as, ar or ab is absent or not of type Z"
                       : kind == bam::RP_BAD_PIECE     ? "as or ar has no piece for the side rs names, or the as piece is empty"
                       : kind == bam::RP_BAD_AB        ? "ab is shorter than the side's piece of as"
                       : kind == bam::RP_BAD_NO_S      ? "an artifact record without a soft clip"
                       : kind == bam::RP_BAD_TID       ? "an artifact record whose refID is outside the header"
                       : kind == bam::RP_BAD_CLIP_EMPTY ? "a soft-clipped record without bases (l_seq 0)"
                                                        : "a soft clip longer than the read";
    return set_err(ctx, FADEHIP_E_INVALID, "report: record %lld: %s", rec, what);
}

// The arrays of a call's reports (`which`: RP_* bits) over n records, one behind the other from `base` (nullptr: only their
// size is wanted): ctl | per report: row_off [2n + 1] u64 | size [2n] u64 | the rows' descriptors [2n] | (stats) work [2n] | res [2n] |
// kind [2n] u8, padded; with `rpm` (a set of intervals attached) the stats report's repeat bits [2n] u8 behind its kind
size_t report_layout(bam::RepArgs &a, uint8_t *base, size_t n, uint32_t which, uint8_t **rpm = nullptr) {
    const size_t ns = 2 * n;
    size_t at = 128;
    auto take = [&](size_t bytes) {
        uint8_t *p = base ? base + at : nullptr;
        at += (bytes + 7) & ~(size_t)7;
        return p;
    };
    a.ctl = (bam::RepCtl *)base;
    for (uint32_t w = 0; w < 2u; w++) {
        if (!(which & (1u << w))) continue;
        a.row_off[w] = (uint64_t *)take(8 * (ns + 1));
        a.size[w] = (uint64_t *)take(8 * ns);
        if (w == 0u) {
            a.srow = (bam::StatsRow *)take(ns * sizeof(bam::StatsRow));
            a.work = (StatsWork *)take(ns * sizeof(StatsWork));
            a.res = (fadehip_sw_stats_result *)take(ns * sizeof(fadehip_sw_stats_result));
        } else {
            a.crow = (bam::ClipRow *)take(ns * sizeof(bam::ClipRow));
        }
        a.kind[w] = take(ns);
        if (w == 0u && rpm) *rpm = take(ns);
    }
    return at + 8;
}

// The kernels of one report (w: 0 stats, 1 clip) behind the stage, whose ctl `c` is on the host: the stats sides' pairs and
// their alignments class by class, the rows' sizes, the scan.  `scratch` holds the multi-strip pairs' rows.  With rpm (the
// repeat bits report_repeats_kernel left) the stats rows are sized with their two more columns.
int enqueue_report_sizes(fadehip_ctx *ctx, hipStream_t st, bam::RepArgs &a, uint32_t w, const bam::RepCtl &c, DevBuf &scratch, const uint8_t *rpm = nullptr) {
    const size_t ns = 2 * (size_t)a.n;
    if (w == 0u) {
        size_t cls_begin[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 5; k++) cls_begin[k + 1] = cls_begin[k] + c.cls[k];
        if (cls_begin[5]) {
            size_t row_bytes;
            const int long_blocks = sw_stats_long_blocks(c.cls[4], (int)c.long_max_lr, &row_bytes);
            int rc;
            if (long_blocks && (rc = reserve(ctx, scratch, (size_t)long_blocks * STATS_WAVES_PER_BLOCK * row_bytes))) return rc;
            hipLaunchKernelGGL(bam::report_bucket_kernel, dim3((unsigned)((ns + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK)), dim3(bam::TAG_BLOCK), 0, st, a);
            HIPCHK(ctx, hipGetLastError());
            StatsScoring sc;  // stats.d:87
            sc.open = 3;
            sc.ext = 8;
            sc.match = 10;
            sc.mismatch = -5;
            sc.rules = ctx->sc.rules;
            if ((rc = enqueue_sw_stats(ctx, st, a.work, cls_begin, a.base, a.base, a.res, scratch.p, (int)c.long_max_lr, long_blocks, sc))) return rc;
        }
    }
    if (rpm && w == 0u) hipLaunchKernelGGL((bam::report_size_kernel<true>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, st, a, w, rpm);
    else hipLaunchKernelGGL((bam::report_size_kernel<false>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, st, a, w, (const uint8_t *)nullptr);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::report_scan_kernel, dim3(1), dim3(1024), 0, st, a, w);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// the sealed set as the kernels read it
bam::IvSetRef intervals_ref(const fadehip_intervals *s) {
    bam::IvSetRef r;
    r.start = (const uint32_t *)s->start.p;
    r.maxend = (const uint64_t *)s->maxend.p;
    r.chrom_first = (const uint32_t *)s->chrom_first.p;
    r.n = (uint32_t)s->n;
    r.n_chrom = (int32_t)s->names.size();
    return r;
}

// ref_chrom: for every contig of a header the set's chrom id of that name, by its bytes, or -1
std::vector<int32_t> intervals_ref_chrom(const fadehip_intervals *s, int32_t n_ref, const char *const *ref_names) {
    std::vector<int32_t> rc((size_t)n_ref + 1, -1);
    for (int32_t c = 0; c < n_ref; c++) {
        const auto it = s->ids.find(ref_names[c]);
        if (it != s->ids.end()) rc[(size_t)c] = it->second;
    }
    return rc;
}

// report_repeats_kernel behind the stage: the two bits of every slot into rpm
int enqueue_report_repeats(fadehip_ctx *ctx, hipStream_t st, const bam::RepArgs &a, const fadehip_intervals *iv, const int32_t *d_ref_chrom, uint8_t *rpm) {
    bam::RepeatArgs q;
    q.s = intervals_ref(iv);
    q.ref_chrom = d_ref_chrom;
    q.name_bytes = (const uint8_t *)iv->name_bytes.p;
    q.name_off = (const uint32_t *)iv->name_off.p;
    q.rpm = rpm;
    const size_t ns = 2 * (size_t)a.n;
    hipLaunchKernelGGL(bam::report_repeats_kernel, dim3((unsigned)((ns + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK)), dim3(bam::TAG_BLOCK), 0, st, a, q);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// fadehip_report_batch, and with a set of intervals fadehip_report_batch_repeats
int report_batch_impl(fadehip_ctx *ctx, int32_t which, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref, const char *const *ref_names,
                      fadehip_intervals *iv, uint8_t *out, int64_t out_cap, int64_t *row_off) {
    if (which != FADEHIP_BAM_REPORT_STATS && which != FADEHIP_BAM_REPORT_CLIP)
        return set_err(ctx, FADEHIP_E_INVALID, "which must be FADEHIP_BAM_REPORT_STATS or FADEHIP_BAM_REPORT_CLIP");
    if (n < 0 || n > (1 << 30) || n_ref < 0 || (n_ref > 0 && !ref_names) || !rec_off || !row_off || (n > 0 && !recs) || out_cap < 0 || (out_cap > 0 && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) {
        row_off[0] = 0;
        return 0;
    }
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, [](int32_t) { return 0; }))) return rc;
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
    const uint32_t w = which == FADEHIP_BAM_REPORT_STATS ? 0u : 1u;
    const size_t ns = 2 * (size_t)n, ntb = ((size_t)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | name_off [n_ref + 1] u32 | first [n_ref] i32 | name bytes;  work: report_layout
    // (with a set: ref_chrom [n_ref] i32 behind the name bytes, and the repeat bits in work)
    const size_t m_noff = 8 * ((size_t)n + 1), m_first = m_noff + 4 * ((size_t)n_ref + 1), m_names = m_first + 4 * (size_t)n_ref;
    const size_t m_refc = (m_names + nbytes.size() + 7) & ~(size_t)7, m_end = iv ? m_refc + 4 * ((size_t)n_ref + 1) : m_names + nbytes.size();
    bam::RepArgs a;
    memset(&a, 0, sizeof a);
    a.which = w == 0u ? bam::RP_STATS : bam::RP_CLIP;
    uint8_t *rpm = nullptr;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, nullptr, 0, m_end + 8, report_layout(a, nullptr, (size_t)n, a.which, iv ? &rpm : nullptr), off))) return rc;
    hipStream_t st = L.stream;
    uint8_t *meta = (uint8_t *)L.meta.p, *work = (uint8_t *)L.work.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_noff, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, st));
    if (n_ref) HIPCHK(ctx, hipMemcpyAsync(meta + m_first, first.data(), 4 * (size_t)n_ref, hipMemcpyHostToDevice, st));
    if (!nbytes.empty()) HIPCHK(ctx, hipMemcpyAsync(meta + m_names, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(work, 0, 128, st));
    report_layout(a, work, (size_t)n, a.which, iv ? &rpm : nullptr);
    a.base = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.names.bytes = meta + m_names;
    a.names.off = (const uint32_t *)(meta + m_noff);
    a.names.first = (const int32_t *)(meta + m_first);
    a.names.n_ref = n_ref;
    hipLaunchKernelGGL(bam::report_stage_kernel, dim3((unsigned)ntb), dim3(bam::TAG_BLOCK), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    std::vector<int32_t> refc;  // (lives to the first wait)
    if (iv) {
        refc = intervals_ref_chrom(iv, n_ref, ref_names);
        HIPCHK(ctx, hipMemcpyAsync(meta + m_refc, refc.data(), 4 * refc.size(), hipMemcpyHostToDevice, st));
        if ((rc = enqueue_report_repeats(ctx, st, a, iv, (const int32_t *)(meta + m_refc), rpm))) return rc;
    }
    bam::RepCtl c;
    HIPCHK(ctx, hipMemcpyAsync(&c, a.ctl, sizeof c, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));  // wait 1: what fails the call, the stats sides per class
    if (c.bad) return report_bad(ctx, c.bad, 0);
    if ((rc = enqueue_report_sizes(ctx, st, a, w, c, L.scratch, rpm))) return rc;
    std::vector<uint64_t> roff(ns + 1);
    HIPCHK(ctx, hipMemcpyAsync(roff.data(), a.row_off[w], 8 * (ns + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));  // wait 2: the rows' offsets
    const uint64_t total = roff[ns];
    if (total > (uint64_t)out_cap)
        return set_err(ctx, FADEHIP_E_INVALID, "the report's rows take %llu bytes, out holds %lld", (unsigned long long)total, (long long)out_cap);
    for (size_t q = 0; q <= ns; q++) row_off[q] = (int64_t)roff[q];
    if (!total) return 0;
    if ((rc = reserve(ctx, L.out, (size_t)total + 8))) return rc;
    a.out[w] = (uint8_t *)L.out.p;
    if (rpm) hipLaunchKernelGGL((bam::report_write_kernel<true>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, st, a, w, (const uint8_t *)rpm);
    else hipLaunchKernelGGL((bam::report_write_kernel<false>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, st, a, w, (const uint8_t *)nullptr);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, a.out[w], (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));  // wait 3: the rows
    return 0;
}

}  // namespace

int fadehip_report_batch(fadehip_ctx *ctx, int32_t which, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref,
                         const char *const *ref_names, uint8_t *out, int64_t out_cap, int64_t *row_off) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    return report_batch_impl(ctx, which, n, recs, rec_off, n_ref, ref_names, nullptr, out, out_cap, row_off);
}

int fadehip_report_batch_repeats(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref, const char *const *ref_names,
                                 fadehip_intervals *iv, uint8_t *out, int64_t out_cap, int64_t *row_off) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!iv) return set_err(ctx, FADEHIP_E_INVALID, "intervals is NULL");
    if (iv->ctx != ctx) return set_err(ctx, FADEHIP_E_INVALID, "report: the set of intervals belongs to another ctx");
    if (!iv->sealed) return set_err(ctx, FADEHIP_E_INVALID, "report: the set of intervals has not been sealed (fadehip_intervals_seal)");
    return report_batch_impl(ctx, FADEHIP_BAM_REPORT_STATS, n, recs, rec_off, n_ref, ref_names, iv, out, out_cap, row_off);
}

// ---- the name set over records the caller brings: bam_names.hpp's kernels, the ones of the file path under
// FADEHIP_BAM_COLLECT_NAMES / FADEHIP_BAM_EJECT_NAMED
int fadehip_nameset_create(fadehip_ctx *ctx, fadehip_nameset **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fadehip_nameset *s = new (std::nothrow) fadehip_nameset;
    if (!s) return set_err(ctx, FADEHIP_E_NOMEM, "out of memory");
    if (const int rc = nameset_init(ctx, s, "FADEHIP_NAMESET_SLOTS", "FADEHIP_NAMESET_HASH_BITS")) {
        fadehip_nameset_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

int fadehip_nameset_add_batch(fadehip_nameset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *pick) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "nameset is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || !rec_off || (n > 0 && !recs)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, false, [](int32_t) { return 0; }))) return rc;
    uint64_t n_pick = 0, b_pick = 0;  // the call's bounds: its picked records, and the bytes their entries take at most
    for (int32_t k = 0; k < n; k++)
        if (!pick || pick[k]) {
            n_pick++;
            b_pick += std::min<uint64_t>(256, (uint64_t)(rec_off[k + 1] - rec_off[k]));
        }
    if (!n_pick) return 0;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | pick [n] u8
    const size_t m_pick = 8 * ((size_t)n + 1);
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, pick, m_pick, m_pick + (size_t)n + 8, 8, off))) return rc;
    std::lock_guard<std::mutex> sl(s->mu);
    if ((rc = nameset_room(s, L.stream, n_pick, b_pick, 1))) return rc;
    bam::NameArgs a = nameset_batch_args(s, L, n);
    a.pick = pick ? (const uint8_t *)L.meta.p + m_pick : nullptr;
    a.pick_mask = 0xffu;
    hipLaunchKernelGGL(bam::bam_names_insert_kernel, dim3(((unsigned)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK), dim3(bam::TAG_BLOCK), 0, L.stream, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(s->h_ctrl.p, s->ctrl.p, 24, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    if (((const unsigned long long *)s->h_ctrl.p)[bam::NS_ERR]) return set_err(ctx, FADEHIP_E_STATE, "nameset: the table or the arena was full during an insert (names may be missing: the set cannot be used)");
    return 0;
}

int fadehip_nameset_contains_batch(fadehip_nameset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, uint8_t *hit) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "nameset is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || !rec_off || (n > 0 && (!recs || !hit))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, false, [](int32_t) { return 0; }))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | hit [n] u8
    const size_t m_hit = 8 * ((size_t)n + 1);
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, nullptr, m_hit, m_hit + (size_t)n + 8, 8, off))) return rc;
    {
        std::lock_guard<std::mutex> sl(s->mu);
        bam::NameArgs a = nameset_batch_args(s, L, n);
        a.hit = (uint8_t *)L.meta.p + m_hit;
        hipLaunchKernelGGL(bam::bam_names_lookup_kernel, dim3(((unsigned)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK), dim3(bam::TAG_BLOCK), 0, L.stream, a);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(hit, (const uint8_t *)L.meta.p + m_hit, (size_t)n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    return 0;
}

int fadehip_nameset_count(fadehip_nameset *s, int64_t *n_names) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "nameset is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (!n_names) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> sl(s->mu);
    if (const int rc = nameset_settle(s, ctx->copy_stream)) return rc;
    *n_names = (int64_t)s->count_ub;
    return 0;
}

void fadehip_nameset_destroy(fadehip_nameset *s) {
    if (!s) return;
    nameset_release(s);
    delete s;
}

// ---- the mate map over records the caller brings (bam_mates.hpp): placements in, mate fields out
int fadehip_mateset_create(fadehip_ctx *ctx, fadehip_mateset **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fadehip_mateset *m = new (std::nothrow) fadehip_mateset;
    if (!m) return set_err(ctx, FADEHIP_E_NOMEM, "out of memory");
    m->core.key_extra = 1;
    m->core.what = "mateset";
    if (const int rc = nameset_init(ctx, &m->core, "FADEHIP_MATESET_SLOTS", "FADEHIP_MATESET_HASH_BITS")) {
        fadehip_mateset_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

int fadehip_mateset_add_batch(fadehip_mateset *m, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                              const int32_t *trim_left, const int32_t *trim_right, const uint8_t *pick) {
    if (!m) return set_err(nullptr, FADEHIP_E_INVALID, "mateset is NULL");
    fadehip_nameset *s = &m->core;
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || !rec_off || (n > 0 && (!recs || !rs || !trim_left || !trim_right))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    // the call's bounds: the records that insert, and the bytes their entries take at most (bam_mates.hpp's header)
    uint64_t n_pick = 0, b_pick = 0;
    const auto bounds = [&](int32_t k) {
        if (trim_left[k] < 0 || trim_right[k] < 0) return set_err(ctx, FADEHIP_E_INVALID, "record %d: negative trim length", k);
        const uint8_t *p = recs + rec_off[k];
        const uint32_t flag = (uint32_t)p[18] | ((uint32_t)p[19] << 8), ncig = (uint32_t)p[16] | ((uint32_t)p[17] << 8), seg = flag & 0xC0u;
        if ((pick && !pick[k]) || !(flag & 1u) || (seg != 0x40u && seg != 0x80u) || (flag & 0x900u)) return 0;
        n_pick++;
        b_pick += bam::MATE_KEY_BYTES_MAX + 4ull * bam::MV_DWORDS + 11ull * (ncig + 2ull) + 3ull;
        return 0;
    };
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, bounds))) return rc;
    if (!n_pick) return 0;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | trim_l [n] u32 | trim_r [n] u32 | rs [n] u8 | pick [n] u8
    const size_t m_tl = 8 * ((size_t)n + 1), m_tr = m_tl + 4 * (size_t)n, m_rs = m_tr + 4 * (size_t)n, m_pick = m_rs + (size_t)n;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_pick + (size_t)n + 8, 8, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tl, trim_left, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tr, trim_right, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    if (pick) HIPCHK(ctx, hipMemcpyAsync(meta + m_pick, pick, (size_t)n, hipMemcpyHostToDevice, L.stream));
    std::lock_guard<std::mutex> sl(s->mu);
    if ((rc = nameset_room(s, L.stream, n_pick, b_pick, 1))) return rc;
    bam::MateArgs a;
    memset(&a, 0, sizeof a);
    a.s = nameset_ref(s);
    a.u = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.rs = meta + m_rs;
    a.trim_l = (const uint32_t *)(meta + m_tl);
    a.trim_r = (const uint32_t *)(meta + m_tr);
    a.pick = pick ? meta + m_pick : nullptr;
    hipLaunchKernelGGL(bam::bam_mates_insert_kernel, dim3(((unsigned)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK), dim3(bam::TAG_BLOCK), 0, L.stream, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(s->h_ctrl.p, s->ctrl.p, 32, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    if (((const unsigned long long *)s->h_ctrl.p)[bam::NS_ERR]) return set_err(ctx, FADEHIP_E_STATE, "mateset: the table or the arena was full during an insert (placements may be missing: the set cannot be used)");
    return 0;
}

// fadehip_clip_batch, then the rule: the plan kernel in the place of the size kernel, the write kernel patching what it planned.
int fadehip_mates_fix_batch(fadehip_mateset *m, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                            const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap, int64_t *out_off, uint8_t *fixed) {
    if (!m) return set_err(nullptr, FADEHIP_E_INVALID, "mateset is NULL");
    fadehip_nameset *s = &m->core;
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || !rec_off || !out_off || (n > 0 && (!recs || !rs || !trim_left || !trim_right || !fixed)) || out_cap < 0 || (out_cap > 0 && !out))
        return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) {
        out_off[0] = 0;
        return 0;
    }
    const auto trims = [&](int32_t k) { return trim_left[k] < 0 || trim_right[k] < 0 ? set_err(ctx, FADEHIP_E_INVALID, "record %d: negative trim length", k) : 0; };
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, trims))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | out_off [n + 1] u64 | fix [n] MateFix | trim_l [n] u32 | trim_r [n] u32 | rs [n] u8;  work: out_size [n] u32
    static_assert(sizeof(bam::MateFix) % 8 == 0, "the fix array keeps what lies behind it aligned");
    const size_t m_out = 8 * ((size_t)n + 1), m_fix = 2 * m_out, m_tl = m_fix + sizeof(bam::MateFix) * (size_t)n, m_tr = m_tl + 4 * (size_t)n, m_rs = m_tr + 4 * (size_t)n;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, rs, m_rs, m_rs + (size_t)n + 8, 4 * (size_t)n, off))) return rc;
    uint8_t *meta = (uint8_t *)L.meta.p;
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tl, trim_left, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(meta + m_tr, trim_right, 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    // (the set's lock is held to the end of the call: its buffers must not move under the two kernels)
    std::lock_guard<std::mutex> sl(s->mu);
    bam::MateArgs a;
    memset(&a, 0, sizeof a);
    a.s = nameset_ref(s);
    a.u = (const uint8_t *)L.in.p;
    a.off64 = (const uint64_t *)meta;
    a.n = (uint32_t)n;
    a.rs = meta + m_rs;
    a.trim_l = (const uint32_t *)(meta + m_tl);
    a.trim_r = (const uint32_t *)(meta + m_tr);
    a.fix = (bam::MateFix *)(meta + m_fix);
    a.out_off = (const uint64_t *)(meta + m_out);
    std::vector<int64_t> ooff((size_t)n + 1);
    if ((rc = size_then_write(ctx, L, a, (size_t)n, bam::mates_batch_plan_kernel, bam::mates_batch_write_kernel, "fixed", false, off, out, out_cap, ooff.data()))) return rc;
    std::vector<bam::MateFix> fix((size_t)n);
    HIPCHK(ctx, hipMemcpyAsync(fix.data(), a.fix, sizeof(bam::MateFix) * (size_t)n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(s->h_ctrl.p, s->ctrl.p, 32, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    if (((const unsigned long long *)s->h_ctrl.p)[bam::NS_ERR]) return set_err(ctx, FADEHIP_E_STATE, "mateset: a look-up came round the whole table (the set cannot be used)");
    for (int32_t k = 0; k < n; k++) fixed[k] = (uint8_t)fix[(size_t)k].state;
    for (int32_t k = 0; k <= n; k++) out_off[k] = ooff[(size_t)k];
    return 0;
}

int fadehip_mateset_count(fadehip_mateset *m, int64_t *n_entries, int64_t *n_ambiguous) {
    if (!m) return set_err(nullptr, FADEHIP_E_INVALID, "mateset is NULL");
    fadehip_nameset *s = &m->core;
    fadehip_ctx *ctx = s->ctx;
    if (!n_entries || !n_ambiguous) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> sl(s->mu);
    if (const int rc = nameset_settle(s, ctx->copy_stream)) return rc;
    *n_entries = (int64_t)s->count_ub;
    *n_ambiguous = (int64_t)((const unsigned long long *)s->h_ctrl.p)[bam::MS_AMBIG];
    return 0;
}

void fadehip_mateset_destroy(fadehip_mateset *m) {
    if (!m) return;
    nameset_release(&m->core);
    delete m;
}

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
    bool from_tags = false;     // FADEHIP_BAM_FROM_TAGS: rs and am come out of the records (bam_from_tags.hpp), nothing is aligned
    bool collect_names = false;  // FADEHIP_BAM_COLLECT_NAMES: from_tags, and every record with rs & 6 adds its name to `names` (bam_names.hpp)
    bool eject_named = false;    // FADEHIP_BAM_EJECT_NAMED: from_tags, and a record is written exactly when its name is not in `names`
    bool keep_sorted = false;    // FADEHIP_BAM_KEEP_SORTED: clip, and the records leave in coordinate order (bam_resort.hpp)
    uint32_t report = 0;         // FADEHIP_BAM_REPORT_STATS / _CLIP as bam::RP_*: from_tags, and every call leaves the reports' rows (bam_report.hpp)
    bool index = false;          // FADEHIP_BAM_INDEX: every call leaves the .bai entries of the records it wrote (bam_index.hpp)
    IndexGeometry ix_geo;        // fadehip_bam_index_geometry: ... the entries of a CSI of that geometry instead (depth 0: none)
    bool collect_mates = false;  // FADEHIP_BAM_COLLECT_MATES: from_tags and clip, and every primary paired-end record whose name is in `names` stores its placement in `mates` (bam_mates.hpp)
    bool fix_mates = false;      // FADEHIP_BAM_FIX_MATES: from_tags and clip, and every record's mate fields follow the placement `mates` holds for its mate
    bool calmd = false;          // FADEHIP_BAM_CALMD: from_tags and clip, and NM and MD of every record that leaves hard-clipped are recomputed against the genome (bam_calmd.hpp)
    fadehip_nameset *names = nullptr;  // fadehip_bam_use_nameset
    fadehip_mateset *mates = nullptr;  // fadehip_bam_use_mateset
    bool store_extract = false;  // FADEHIP_BAM_STORE_EXTRACT: extract, and the calls' extract records stay on the device, in `recstore` (bam_recstore.hpp)
    bool store_output = false;   // FADEHIP_BAM_STORE_OUTPUT: the calls' OUTPUT records stay on the device, in `recstore` (bam_sortwin.hpp); back hands out nothing
    fadehip_recstore *recstore = nullptr;  // fadehip_bam_use_recstore
    bool repeats = false;        // FADEHIP_BAM_REPORT_REPEATS: the stats rows gain read_rpm and art_rpm (bam_intervals.hpp)
    fadehip_intervals *intervals = nullptr;  // fadehip_bam_use_intervals
    std::vector<std::string> ref_names_h;    // the header's contigs as the caller named them (ref_chrom is made of them)
    DevBuf ref_chrom;            // repeats: the set's chrom id of every contig of the header
    DevBuf names_text, names_off;
    DevBuf names_first;         // from_tags: for every contig the first one of its name (fadehip_tags_batch's rule)
    struct Out {
        DevBuf o;
        size_t bytes = 0;
        hipEvent_t ready = nullptr;
        // extract: the call's extract records on the device, their bytes and number, and the event behind their copy to the host
        DevBuf x;
        size_t xbytes = 0;
        int64_t xrecs = 0;
        hipEvent_t xready = nullptr;
        // report: the call's rows on the device per report (stats, clip), their bytes and number, and the event behind their copies
        DevBuf r[2];
        size_t rbytes[2] = {0, 0};
        int64_t rrows[2] = {0, 0};
        hipEvent_t rready = nullptr;
        // index (bam_index.hpp): where the call's records lie in o (made when the call is finished, on its slot's stream), the
        // stage's arrays and ctl, its arguments (the arrays it writes are pinned memory of the stream), the records it was
        // launched for at most (0: no stage — the call wrote nothing), and the event behind it
        DevBuf ix_at, ix_work, ix_ctl;
        bam::IndexArgs ixa;
        uint32_t ix_n_cap = 0;
        hipEvent_t iready = nullptr;
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
        DevBuf rx_cnt;                        // store_extract, store_output: the append kernels' item counts per block, and their bases
        DevBuf sw_key;                        // store_output with clip: the keys the records leave with (bam_sortwin.hpp)
        DevBuf ej_head, ej_blk, ej_grp;       // eject: every record's group start, the blocks' last starts and carries, the groups' marks
        // from_tags: the stage's per-record arrays (rs byte, trims), per-side arrays (contig, position, ops, text), the ops'
        // block sums and bases, where a record's ops start, and the ops themselves (sized in back, when their total is known)
        DevBuf ft_rec, ft_side, ft_ops_blk, ft_ops_at, ft_ops;
        bam::FromTagsArgs fa;
        DevBuf rp, rp_scratch;                // report: the arrays of report_layout; sw_stats_kernel's rows of its multi-strip pairs
        PinBuf h_rp;                          // the RepCtl behind the stage, then behind the scans
        bam::RepArgs rpa;
        uint8_t *rpm = nullptr;               // report with a set of intervals attached: the stats slots' repeat bits (in rp)
        bam::TagArgs xa;                      // extract: ta with the extract stream's sizes, sums, counts and output
        PinBuf h_blocks, h_counts;
        PinBuf h_ns;                          // collect_names / eject_named: the set's ctrl words behind the call's kernels; the mate map's at + 32
        DevBuf mt_hit, mt_fix;                // collect_mates: the name look-up's byte per record; fix_mates: the plan per record
        DevBuf cm_fix;                        // calmd: the plan per record
        // keep_sorted (bam_resort.hpp).  Call k reads what call k - 1 left in the OTHER set — its ctl and final-order arrays in
        // its front half (behind rs_meta), the bytes of its hold in its back half (behind rs_moved) — and writes only its own
        // set's, so a call never writes what the call in front of it still reads.
        DevBuf rs_ctl, rs_arr;                // the call's ResortCtl; the stage's arrays (resort_layout)
        DevBuf rs_stage, rs_hold;             // the call's records in input order (what the rewrite writes); the records held behind it
        PinBuf h_rs;                          // the ctl behind the stage
        hipEvent_t rs_meta = nullptr, rs_moved = nullptr;
        bam::ResortArgs ra;
        uint32_t rs_n_rec = 0;                // records of the set's call
        uint64_t rs_held = 0;                 // records held behind it (known once the call is finished)
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
    PinBuf rbuf[2][FADEHIP_BAM_CHUNKS + 1];  // report: the rows of call k per report, pinned, as xbuf
    const uint8_t *last_r[2] = {nullptr, nullptr};  // fadehip_bam_back_report: what the most recent back finished
    size_t last_rbytes[2] = {0, 0};
    int64_t last_rrows[2] = {0, 0};
    const uint8_t *last_x = nullptr;        // fadehip_bam_back_extract: what the most recent back finished
    size_t last_xbytes = 0;
    int64_t last_xrecs = 0;
    bool have_back = false;
    // index: the entries of call k, pinned, k % FADEHIP_BAM_CHUNKS (the write kernel stores them there itself; they are good as
    // long as the call's members); what fadehip_bam_back_index hands out; the records and the last key of the calls so far
    PinBuf ixbuf[FADEHIP_BAM_CHUNKS];
    fadehip_index_call last_ix = {};
    bool have_ix = false, ix_have_key = false;
    int64_t ix_records = 0;
    uint64_t ix_last_key = 0;
    // the counts of a call as they cross to the host: the call's ChunkCounts, with extract the extract stream's behind it,
    // with from_tags the stage's StageCounts behind those
    size_t stage_counts_at() const { return sizeof(bam::ChunkCounts) * (extract ? 2u : 1u); }
    size_t counts_bytes() const { return stage_counts_at() + (from_tags ? sizeof(bam::StageCounts) : 0u); }
    std::mutex mu;
    std::condition_variable cv;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n_records = 0, n_oversize = 0, n_redone = 0, n_ejected = 0;
    int64_t n_fixed = 0, n_mate_ambiguous = 0;  // fix_mates
    int64_t n_calmd_updated = 0, n_calmd_skipped = 0;  // calmd
    int64_t held_recs = 0, held_bytes = 0;  // keep_sorted: behind the most recent finished call
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

// ---- FADEHIP_BAM_KEEP_SORTED and fadehip_coord_order_batch (bam_resort.hpp)
// The stage's arrays for at most m_cap items, one behind the other from `base` (nullptr: only their size is wanted)
size_t resort_layout(bam::ResortArgs &a, uint8_t *base, size_t m_cap) {
    const size_t m = std::max<size_t>(m_cap, 1), tiles = (m + bam::RS_TILE - 1) / bam::RS_TILE, ntb = (m + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        uint8_t *p = base + at;
        at += (bytes + 7) & ~(size_t)7;
        return p;
    };
    a.key0 = (uint64_t *)take(8 * m);
    a.key1 = (uint64_t *)take(8 * m);
    a.isrc = (uint64_t *)take(8 * m);
    a.msrc = (uint64_t *)take(8 * m);
    a.dst = (uint64_t *)take(8 * (m + 1));
    a.sblk = (uint64_t *)take(16 * ntb);
    a.idx0 = (uint32_t *)take(4 * m);
    a.idx1 = (uint32_t *)take(4 * m);
    a.isize = (uint32_t *)take(4 * m);
    a.msize = (uint32_t *)take(4 * m);
    a.hist = (uint32_t *)take(4 * 256 * tiles);
    a.hist_base = (uint32_t *)take(4 * 256 * tiles);
    return at;
}

// the eight passes over at most m_cap items (the kernels take the true number from a.ctl): side 0 holds the final order
int enqueue_resort_sort(fadehip_ctx *ctx, hipStream_t q, const bam::ResortArgs &a, size_t m_cap) {
    const unsigned tiles = (unsigned)((std::max<size_t>(m_cap, 1) + bam::RS_TILE - 1) / bam::RS_TILE);
    for (uint32_t pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(bam::bam_resort_hist_kernel, dim3(tiles), dim3(256), 0, q, a, pass);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_resort_scan_kernel, dim3(1), dim3(1024), 0, q, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_resort_scatter_kernel, dim3(tiles), dim3(256), 0, q, a, pass);
        HIPCHK(ctx, hipGetLastError());
    }
    return 0;
}

// ---- FADEHIP_BAM_INDEX and fadehip_index_batch (bam_index.hpp)
// The stage's arrays for at most n_cap records, one behind the other from `base` (nullptr: only their size is wanted)
size_t index_layout(bam::IndexArgs &a, uint8_t *base, size_t n_cap) {
    const size_t n = std::max<size_t>(n_cap, 1), nb = (n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        uint8_t *p = base + at;
        at += (bytes + 7) & ~(size_t)7;
        return p;
    };
    a.uo = (uint64_t *)take(8 * (n + 1));
    a.blk_max = (uint64_t *)take(8 * nb);
    a.blk_carry = (uint64_t *)take(8 * nb);
    a.blk_sums = (uint64_t *)take(32 * nb);
    a.blk_base = (uint64_t *)take(32 * nb);
    a.cum = (uint64_t *)take(16 * n);
    a.rec = (bam::IndexRec *)take(sizeof(bam::IndexRec) * n);
    return at;
}

// where the three arrays the stage writes lie in one block from `base`: n_cap chunks, n_cap reference runs, cap_linear entries
size_t index_out_layout(bam::IndexArgs &a, uint8_t *base, size_t n_cap, size_t cap_linear) {
    a.chunks = (fadehip_index_chunk *)base;
    a.refs = (fadehip_index_ref *)(base + sizeof(fadehip_index_chunk) * n_cap);
    a.linear = (fadehip_index_linear *)(base + (sizeof(fadehip_index_chunk) + sizeof(fadehip_index_ref)) * n_cap);
    a.cap_linear = (uint32_t)cap_linear;
    return (sizeof(fadehip_index_chunk) + sizeof(fadehip_index_ref)) * n_cap + sizeof(fadehip_index_linear) * cap_linear;
}

// the stage up to its counts (a.n > 0): the ctl cleared, keys, the running maximum, heads and counts, their sums
// (geo.depth 0: BAI's fixed tree, the key kernel as it always was; else the key kernel under the geometry)
int enqueue_index_counts(fadehip_ctx *ctx, hipStream_t q, const bam::IndexArgs &a, IndexGeometry geo = IndexGeometry()) {
    const unsigned nb = (a.n + bam::TAG_BLOCK - 1u) / bam::TAG_BLOCK;
    HIPCHK(ctx, hipMemsetAsync(a.ctl, 0, sizeof(bam::IndexCtl), q));
    HIPCHK(ctx, hipMemsetAsync(&a.ctl->bad_order, 0xff, 8, q));  // (bad_order and bad_span: IX_NONE)
    if (geo.depth) {
        bam::IndexGeoArgs g;
        g.a = a;
        g.min_shift = (uint32_t)geo.min_shift;
        g.depth = (uint32_t)geo.depth;
        g.limit = geo.limit();
        hipLaunchKernelGGL(bam::bam_index_key_geo_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, q, g);
    } else
        hipLaunchKernelGGL(bam::bam_index_key_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, q, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_index_max_scan_kernel, dim3(1), dim3(1024), 0, q, a, nb);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_index_count_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, q, a, nb);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_index_sum_scan_kernel, dim3(1), dim3(1024), 0, q, a, nb);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// ... and behind them the three arrays (a.chunks, a.refs and a.linear are set)
int enqueue_index_write(fadehip_ctx *ctx, hipStream_t q, const bam::IndexArgs &a) {
    const unsigned nb = (a.n + bam::TAG_BLOCK - 1u) / bam::TAG_BLOCK;
    hipLaunchKernelGGL(bam::bam_index_write_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, q, a, nb);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_index_refs_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, q, a, a.n);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// what the stage's flags fail a call with: the lower record of the two, the order first; `first` is record 0's index in the stream
int index_bad(fadehip_ctx *ctx, const bam::IndexCtl &c, long long first, const char *who, IndexGeometry geo = IndexGeometry()) {
    if (c.bad_order != bam::IX_NONE && c.bad_order <= c.bad_span)
        return set_err(ctx, FADEHIP_E_INVALID, "%s: record %lld: not in coordinate order (--write-index needs coordinate-sorted output)", who, first + (long long)c.bad_order);
    if (c.bad_span != bam::IX_NONE && geo.depth)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "%s: record %lld: ends beyond 2^%d on its reference (a CSI index of min_shift %d and depth %d cannot hold it)", who,
                       first + (long long)c.bad_span, geo.min_shift + 3 * geo.depth, geo.min_shift, geo.depth);
    if (c.bad_span != bam::IX_NONE)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "%s: record %lld: ends beyond 2^29 on its reference (a BAI index cannot hold it)", who, first + (long long)c.bad_span);
    return 0;
}

// C's part under FADEHIP_BAM_INDEX, behind the rewrite or the move on the slot's stream and in front of the event the
// compressor waits for: where every record the call writes lies in its output, dense and in the order it leaves — the set's
// arrays are the next call's to overwrite once this one is finished, so the offsets move to the ring place here.
int bam_finish_index(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, hipStream_t q) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *out = S.out;
    int rc;
    out->ix_n_cap = 0;
    bam::IndexArgs &a = out->ixa;
    memset(&a, 0, sizeof a);
    if (!out->bytes) return 0;
    if ((rc = reserve(ctx, out->ix_ctl, 256))) return rc;
    if (st->keep_sorted) {
        const bam::ResortCtl c = *(const bam::ResortCtl *)S.h_rs.p;
        if ((rc = reserve_roomy(ctx, out->ix_at, 8 * ((size_t)c.n_emit + 1)))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(out->ix_at.p, S.ra.dst, 8 * ((size_t)c.n_emit + 1), hipMemcpyDeviceToDevice, q));
        a.n = c.n_emit;
    } else {
        const uint32_t n = S.n_rec, ntb = (n + bam::TAG_BLOCK - 1u) / bam::TAG_BLOCK;
        if ((rc = reserve_roomy(ctx, out->ix_at, 8 * ((size_t)n + 1) + 8 * (size_t)ntb + 8))) return rc;
        bam::IndexAtArgs g;
        g.out_size = (const uint32_t *)S.out_size.p;
        g.blk_base = st->from_tags ? S.fa.blk_base : S.ta.blk_base;
        g.n = n;
        g.at = (uint64_t *)out->ix_at.p;
        g.cnt = (uint32_t *)(g.at + n + 1);
        g.cnt_base = g.cnt + ntb;
        g.n_out = (uint32_t *)((uint8_t *)out->ix_ctl.p + 128);
        hipLaunchKernelGGL(bam::bam_index_present_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, g);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_index_present_scan_kernel, dim3(1), dim3(1024), 0, q, g, ntb);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_index_at_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, g);
        HIPCHK(ctx, hipGetLastError());
        a.n = n;
        a.n_ptr = g.n_out;
    }
    out->ix_n_cap = a.n;
    return 0;
}

// The back half's part, on the compressor lane's stream behind the scan that fixes member_off[] (or the stored members,
// whose offsets the host knows): the stage, writing its arrays and — in one small copy behind them — its ctl into the pinned
// block of the call's ring place.  Room for one linear entry per record and 65536 more; a call that needs more (known when
// back has waited) has its arrays written again into a larger block.
size_t index_pinned_bytes(size_t n_cap, size_t cap_linear) {
    bam::IndexArgs t;
    return 128 + index_out_layout(t, nullptr, n_cap, cap_linear);
}
int bam_enqueue_index(fadehip_bam_stream *st, uint64_t k, int lane) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *o = &st->ring[k % FADEHIP_BAM_CHUNKS];
    if (!o->ix_n_cap) return 0;
    hipStream_t q = ctx->bgzf[lane].stream;
    bam::IndexArgs &a = o->ixa;
    const size_t n = o->ix_n_cap, cap_linear = n + 65536;
    PinBuf &pb = st->ixbuf[k % FADEHIP_BAM_CHUNKS];
    int rc;
    if ((rc = reserve_roomy(ctx, o->ix_work, index_layout(a, nullptr, n))) || (rc = reserve_pinned(ctx, pb, index_pinned_bytes(n, cap_linear)))) return rc;
    index_layout(a, (uint8_t *)o->ix_work.p, n);
    index_out_layout(a, pb.p + 128, n, cap_linear);
    a.ctl = (bam::IndexCtl *)o->ix_ctl.p;
    a.u = (const uint8_t *)o->o.p;
    a.at = (const uint64_t *)o->ix_at.p;
    const BgzfGeometry g = bgzf_lane_geometry(ctx, lane, st->stored);
    a.block = g.block;
    a.member_off = g.member_off;
    a.behind_ptr = g.behind_ptr;
    a.member_stride = g.member_stride;
    a.behind = g.behind;
    if ((rc = enqueue_index_counts(ctx, q, a, st->ix_geo)) || (rc = enqueue_index_write(ctx, q, a))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(pb.p, a.ctl, sizeof(bam::IndexCtl), hipMemcpyDeviceToHost, q));
    if (!o->iready) HIPCHK(ctx, hipEventCreateWithFlags(&o->iready, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    HIPCHK(ctx, hipEventRecord(o->iready, q));
    return 0;
}

// back has waited for the call's members: its index entries.  Fails the call on what the stage flagged and on keys that step
// back between two calls; fills st->last_ix.
int bam_take_index(fadehip_bam_stream *st, uint64_t k, int lane) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *o = &st->ring[k % FADEHIP_BAM_CHUNKS];
    fadehip_index_call &r = st->last_ix;
    memset(&r, 0, sizeof r);
    st->have_ix = true;
    if (!o->ix_n_cap) return 0;
    PinBuf &pb = st->ixbuf[k % FADEHIP_BAM_CHUNKS];
    HIPCHK(ctx, hipEventSynchronize(o->iready));
    bam::IndexCtl c = *(const bam::IndexCtl *)pb.p;
    int rc;
    if ((rc = index_bad(ctx, c, (long long)st->ix_records, "bam stream", st->ix_geo))) return rc;
    if (c.n && st->ix_have_key && c.first_key < st->ix_last_key)
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: record %lld: not in coordinate order (--write-index needs coordinate-sorted output)", (long long)st->ix_records);
    if (c.n_linear > o->ixa.cap_linear) {
        // (a call whose records reach more windows than it has records + 65536: the arrays once more, with room for all)
        if (c.n_linear >> 31) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu linear index entries in one call (at most 2^31)", (unsigned long long)c.n_linear);
        hipStream_t q = ctx->bgzf[lane].stream;
        if ((rc = reserve_pinned(ctx, pb, index_pinned_bytes(o->ix_n_cap, (size_t)c.n_linear)))) return rc;
        index_out_layout(o->ixa, pb.p + 128, o->ix_n_cap, (size_t)c.n_linear);
        if ((rc = enqueue_index_write(ctx, q, o->ixa))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(q));
    }
    r.chunks = o->ixa.chunks;
    r.linear = o->ixa.linear;
    r.refs = o->ixa.refs;
    r.n_chunks = (int64_t)c.n_chunks;
    r.n_linear = (int64_t)c.n_linear;
    r.n_refs = (int64_t)c.n_refs;
    r.n_records = (int64_t)c.n;
    r.first_key = c.first_key;
    r.last_key = c.last_key;
    if (c.n) {
        st->ix_last_key = c.last_key;
        st->ix_have_key = true;
    }
    st->ix_records += (int64_t)c.n;
    return 0;
}

// B's last part under FADEHIP_BAM_KEEP_SORTED, behind the sizes and their scan (an empty call comes here too: the last call
// hands out what is still held): the held-over records and the call's become items, are sorted, cut at W and given their
// offsets in final order; the ctl goes to the host behind the counts, which back waits for anyway.
int bam_front_resort(fadehip_bam_stream *st, uint64_t k, uint32_t n_rec, int last) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Set &S = st->set[k & 1], &P = st->set[(k + 1) & 1];
    hipStream_t q = ctx->slots[k & 1].stream;
    int rc;
    // what the previous call may hold at most: call k - 2's hold is known (front has finished that call), call k - 1 adds
    // at most its own records
    const uint64_t h_cap64 = k == 0 ? 0 : (k >= 2 ? S.rs_held : 0) + P.rs_n_rec;
    const uint64_t m_cap = h_cap64 + n_rec;
    if (m_cap >= ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu records held and framed in one call (at most 2^31)", (unsigned long long)m_cap);
    bam::ResortArgs &a = S.ra;
    memset(&a, 0, sizeof a);
    if ((rc = reserve_roomy(ctx, S.rs_arr, resort_layout(a, nullptr, (size_t)m_cap))) || (rc = reserve(ctx, S.rs_ctl, 256)) || (rc = reserve_pinned(ctx, S.h_rs, 64))) return rc;
    resort_layout(a, (uint8_t *)S.rs_arr.p, (size_t)m_cap);
    a.ctl = (bam::ResortCtl *)S.rs_ctl.p;
    if (k) {
        a.prev = (const bam::ResortCtl *)P.rs_ctl.p;
        a.p_key = P.ra.key0;
        a.p_dst = P.ra.dst;
        a.p_size = P.ra.msize;
        HIPCHK(ctx, hipStreamWaitEvent(q, P.rs_meta, 0));
    }
    a.h_cap = (uint32_t)h_cap64;
    a.n = n_rec;
    a.last = last ? 1u : 0u;
    a.u = S.pa.u;
    a.rec_off = S.pa.rec_off;
    a.out_size = (const uint32_t *)S.out_size.p;
    a.blk_base = st->from_tags ? S.fa.blk_base : S.ta.blk_base;
    hipLaunchKernelGGL(bam::bam_resort_carry_kernel, dim3((unsigned)(h_cap64 / 256 + 1)), dim3(256), 0, q, a);
    HIPCHK(ctx, hipGetLastError());
    if (n_rec) {
        if (st->from_tags) hipLaunchKernelGGL(bam::bam_resort_keys_kernel<true>, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, a, S.ta, S.fa);
        else hipLaunchKernelGGL(bam::bam_resort_keys_kernel<false>, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, a, S.ta, S.fa);
        HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = enqueue_resort_sort(ctx, q, a, (size_t)m_cap))) return rc;
    const uint32_t ntb_cap = (uint32_t)((std::max<uint64_t>(m_cap, 1) + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK);
    hipLaunchKernelGGL(bam::bam_resort_cut_kernel, dim3(ntb_cap), dim3(bam::TAG_BLOCK), 0, q, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_resort_offsets_scan_kernel, dim3(1), dim3(1024), 0, q, a, ntb_cap);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::bam_resort_offsets_kernel, dim3(ntb_cap), dim3(bam::TAG_BLOCK), 0, q, a, ntb_cap);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S.h_rs.p, a.ctl, sizeof(bam::ResortCtl), hipMemcpyDeviceToHost, q));
    if (!S.rs_meta) HIPCHK(ctx, hipEventCreateWithFlags(&S.rs_meta, hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(S.rs_meta, q));
    S.rs_n_rec = n_rec;
    return 0;
}

// C's last part under FADEHIP_BAM_KEEP_SORTED, behind the rewrite into the staging bytes: every item to its place in the
// call's output or in the hold the next call reads.  The ctl is on the host (the caller has waited for the stream).
int bam_finish_resort(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, uint64_t k, hipStream_t q) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Set &P = st->set[(k + 1) & 1];
    fadehip_bam_stream::Out *out = S.out;
    const bam::ResortCtl c = *(const bam::ResortCtl *)S.h_rs.p;
    int rc;
    if (c.emit_bytes > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu output bytes in one call (at most 2^31)", (unsigned long long)c.emit_bytes);
    const uint64_t hold_bytes = c.total_bytes - c.emit_bytes;
    // (a buffer that grows is given back first, which waits for the device: the previous call's move, which read this set's
    // old hold, is through then)
    if ((rc = reserve_roomy(ctx, out->o, (size_t)c.emit_bytes + 256)) || (rc = reserve_roomy(ctx, S.rs_hold, (size_t)hold_bytes + 256))) return rc;
    if (k && P.rs_moved) HIPCHK(ctx, hipStreamWaitEvent(q, P.rs_moved, 0));
    if (c.n_in) {
        bam::ResortArgs &a = S.ra;
        a.stage = (const uint8_t *)S.rs_stage.p;
        a.hold_in = (const uint8_t *)P.rs_hold.p;
        a.out = (uint8_t *)out->o.p;
        a.hold_out = (uint8_t *)S.rs_hold.p;
        hipLaunchKernelGGL(bam::bam_resort_move_kernel, dim3((c.n_in + 15u) / 16u), dim3(256), 0, q, a, c.n_in, c.n_emit, (uint64_t)c.emit_bytes);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!S.rs_moved) HIPCHK(ctx, hipEventCreateWithFlags(&S.rs_moved, hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(S.rs_moved, q));
    out->bytes = (size_t)c.emit_bytes;
    S.rs_held = c.n_in - c.n_emit;
    std::lock_guard<std::mutex> l(st->mu);
    st->held_recs = (int64_t)S.rs_held;
    st->held_bytes = (int64_t)hold_bytes;
    return 0;
}

// ---- the record store (bam_recstore.hpp): what a launch names of it, its growth, a call's items
// The sort's item numbers are uint32 (bam_resort.hpp's idx arrays and its kernels' j); the launches here are sized in int32.
constexpr uint64_t RECSTORE_MAX_ITEMS = ((uint64_t)1 << 31) - 1;
constexpr uint64_t RECSTORE_DEFAULT_BYTES = (uint64_t)64 << 20;
constexpr uint64_t RECSTORE_MAX_DRAIN = (uint64_t)1 << 30;  // bytes of one drain at most (the compressor takes 2^31 a call)

bam::RecStoreRef recstore_ref(const fadehip_recstore *s) {
    bam::RecStoreRef r;
    r.arena = (uint8_t *)s->arena.p;
    r.key = (uint64_t *)s->key.p;
    r.off = (uint64_t *)s->off.p;
    r.size = (uint32_t *)s->size.p;
    return r;
}

int recstore_alloc(fadehip_ctx *ctx, DevBuf &b, size_t bytes) {
    b.p = nullptr;
    b.cap = 0;
    const size_t want = (std::max<size_t>(bytes, 256) + 255) & ~(size_t)255;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return set_err(ctx, FADEHIP_E_NOMEM, "recstore: allocating %zu bytes on the device failed (the sorted extract holds every extract record on the device)", want);
    }
    b.cap = want;
    return 0;
}

// a larger buffer with the first `keep` bytes of the old one (the caller holds s->mu and has waited for the device)
int recstore_regrow(fadehip_ctx *ctx, hipStream_t q, DevBuf &b, size_t keep, size_t want) {
    DevBuf nb;
    if (const int rc = recstore_alloc(ctx, nb, want)) return rc;
    if (keep && (hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)) {
        release(nb);
        return set_err(ctx, FADEHIP_E_HIP, "recstore: moving the records to a larger buffer failed");
    }
    release(b);
    b = nb;
    return 0;
}

// Room for a call that adds bytes_new bytes and items_new items, made before anything of it is enqueued on q (the caller
// holds s->mu).  Where there is none the device is waited for — the store's kernels may be on any of the ctx's streams — and
// the arena, or the item arrays, move to buffers of twice the size (or what the call needs, if that is more).
int recstore_room(fadehip_recstore *s, hipStream_t q, uint64_t bytes_new, uint64_t items_new) {
    fadehip_ctx *ctx = s->ctx;
    if (s->sorted) return set_err(ctx, FADEHIP_E_STATE, "recstore: the store has been sorted, nothing can be added to it any more");
    if (s->n_items + items_new > RECSTORE_MAX_ITEMS)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "recstore: more than %llu records (the sort numbers its items in 32 bits)", (unsigned long long)RECSTORE_MAX_ITEMS);
    if (s->budget_set && recstore::sortwin_cost(s->used + bytes_new, s->n_items + items_new) > s->budget)
        return set_err(ctx, FADEHIP_E_NOMEM, "recstore: %llu bytes in %llu records would cost more than the budget of %llu bytes (the store holds every output record on the device)",
                       (unsigned long long)(s->used + bytes_new), (unsigned long long)(s->n_items + items_new), (unsigned long long)s->budget);
    const bool grow_arena = s->used + bytes_new + 8 > (uint64_t)s->arena.cap, grow_items = s->n_items + items_new > s->item_cap;
    if (!grow_arena && !grow_items) return 0;
    HIPCHK(ctx, hipDeviceSynchronize());
    int rc;
    // (under a budget a growth stops at what the budget lets the store hold: at most `budget` bytes, budget / 64 records)
    const uint64_t need_bytes = s->used + bytes_new + 8, need_items = s->n_items + items_new;
    uint64_t want_bytes = std::max<uint64_t>(2 * (uint64_t)s->arena.cap, need_bytes);
    if (s->budget_set) want_bytes = std::max<uint64_t>(std::min<uint64_t>(want_bytes, s->budget + 8), need_bytes);
    if (grow_arena && (rc = recstore_regrow(ctx, q, s->arena, (size_t)s->used, (size_t)want_bytes))) return rc;
    if (grow_items) {
        uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(2 * s->item_cap, need_items), 1024);
        if (s->budget_set) cap = std::max<uint64_t>(std::min<uint64_t>(cap, std::max<uint64_t>(s->budget / recstore::SORTWIN_ITEM_COST, 1024)), need_items);
        if ((rc = recstore_regrow(ctx, q, s->key, 8 * (size_t)s->n_items, 8 * (size_t)cap)) || (rc = recstore_regrow(ctx, q, s->off, 8 * (size_t)s->n_items, 8 * (size_t)cap)) ||
            (rc = recstore_regrow(ctx, q, s->size, 4 * (size_t)s->n_items, 4 * (size_t)cap)))
            return rc;  // (an array that has grown already stays grown: it holds what it held)
        s->item_cap = cap;
    }
    return 0;
}

// The items of a call's n_slots slots, behind the kernel that wrote their records at arena + base (bam_recstore.hpp); cnt:
// 2 x blocks u32 of the caller's.  Enqueued under s->mu.
int enqueue_recstore_append(fadehip_recstore *s, hipStream_t q, uint64_t base, uint64_t item0, uint32_t n_slots, uint32_t n_items, const uint32_t *x_size,
                            const uint64_t *blk_base, uint32_t *cnt) {
    fadehip_ctx *ctx = s->ctx;
    const uint32_t ntb = (n_slots + bam::TAG_BLOCK - 1u) / bam::TAG_BLOCK;
    bam::RecAppendArgs a;
    a.s = recstore_ref(s);
    a.base = base;
    a.item0 = item0;
    a.n = n_slots;
    a.n_items = n_items;
    a.x_size = x_size;
    a.blk_base = blk_base;
    a.cnt_sums = cnt;
    a.cnt_base = cnt + ntb;
    hipLaunchKernelGGL(bam::recstore_count_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::recstore_count_scan_kernel, dim3(1), dim3(1024), 0, q, a, ntb);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(bam::recstore_append_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// FADEHIP_BAM_STORE_OUTPUT, B of a call behind the kernels that decide which records leave and in front of the scan of the
// blocks' sums (bam_sortwin.hpp): the store's table, if it measures, and its window as they are now — both are set before a
// pass begins.  S.ta and S.fa are the call's (the key follows the clip plan the rewrite will follow).
int enqueue_sortwin(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, hipStream_t q, uint32_t n_rec, uint32_t ntb, uint32_t *out_size, uint32_t *info, uint64_t *blk_sums) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_recstore *rs = st->recstore;
    bam::SortWinArgs a;
    memset(&a, 0, sizeof a);
    a.u = S.pa.u;
    a.rec_off = S.pa.rec_off;
    a.n = n_rec;
    a.clip = st->clip ? 1u : 0u;
    a.out_size = out_size;
    a.info = info;
    a.blk_sums = blk_sums;
    a.counts = S.pa.counts;
    if (st->clip) {
        if (const int rc = reserve_roomy(ctx, S.sw_key, 8 * (size_t)n_rec)) return rc;
        a.leave_key = (uint64_t *)S.sw_key.p;
    }
    {
        std::lock_guard<std::mutex> sl(rs->mu);
        if (rs->measuring) {
            a.table = (unsigned long long *)rs->table.p;
            a.first = (const uint32_t *)rs->lay_dev.p;
            a.n_ref = (uint32_t)rs->lay.nb.size();
            a.nb = a.first + a.n_ref;
            a.n_buckets = rs->lay.n_buckets;
        }
        a.lo = rs->win_lo;
        a.hi = rs->win_hi;
    }
    if (st->from_tags) hipLaunchKernelGGL(bam::bam_sortwin_kernel<true>, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, a, S.ta, S.fa);
    else hipLaunchKernelGGL(bam::bam_sortwin_kernel<false>, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, a, S.ta, S.fa);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

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
        if (xb && st->store_extract) {
            // FADEHIP_BAM_STORE_EXTRACT: the call's bytes and items are reserved here, in call order (bam_finish_call) and with
            // numbers that have crossed to the host; the write kernels then put the records at the arena's reserved place, and
            // the append kernels behind them make the items.  All under the store's lock: the arena must not move before
            // these launches have run.
            fadehip_recstore *rs = st->recstore;
            const uint32_t n_x = xc->n_records;
            std::lock_guard<std::mutex> sl(rs->mu);
            if ((rc = recstore_room(rs, q, xb, n_x)) || (rc = reserve_roomy(ctx, S.rx_cnt, 8 * (size_t)S.ntb + 8))) return rc;
            uint8_t *at = (uint8_t *)rs->arena.p + rs->used;
            const uint64_t *blk_base;
            if (st->from_tags) {
                const uint64_t n_ops = ((const bam::StageCounts *)(S.h_counts.p + st->stage_counts_at()))->ops.out_bytes;
                if (n_ops > ((uint64_t)1 << 29)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu CIGAR ops in one call's am tags (at most 2^29)", (unsigned long long)n_ops);
                if ((rc = reserve_roomy(ctx, S.ft_ops, 4 * (size_t)n_ops + 8))) return rc;
                S.fa.ops = (uint32_t *)S.ft_ops.p;
                S.fa.xo = at;
                blk_base = S.fa.x_blk_base;
                hipLaunchKernelGGL(bam::bam_tags_ops_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.fa);
                HIPCHK(ctx, hipGetLastError());
                hipLaunchKernelGGL(bam::bam_tags_extract_write_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.fa);
            } else {
                S.xa.o = at;
                blk_base = S.xa.blk_base;
                hipLaunchKernelGGL(bam::bam_extract_write_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.xa);
            }
            HIPCHK(ctx, hipGetLastError());
            if ((rc = enqueue_recstore_append(rs, q, rs->used, rs->n_items, S.n_rec, n_x, (const uint32_t *)S.ex_size.p, blk_base, (uint32_t *)S.rx_cnt.p))) return rc;
            rs->used += xb;
            rs->n_items += n_x;
            out->xrecs = (int64_t)n_x;
        } else if (xb) {
            PinBuf &xh = st->xbuf[k % (FADEHIP_BAM_CHUNKS + 1)];
            if ((rc = reserve_roomy(ctx, out->x, (size_t)xb + 256)) || (rc = reserve_pinned(ctx, xh, (size_t)xb + (size_t)xb / 4 + 256))) return rc;
            if (st->from_tags) {
                // the sides' ops, materialised now that their total has crossed with the counts, then the records
                const uint64_t n_ops = ((const bam::StageCounts *)(S.h_counts.p + st->stage_counts_at()))->ops.out_bytes;
                if (n_ops > ((uint64_t)1 << 29)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu CIGAR ops in one call's am tags (at most 2^29)", (unsigned long long)n_ops);
                if ((rc = reserve_roomy(ctx, S.ft_ops, 4 * (size_t)n_ops + 8))) return rc;
                S.fa.ops = (uint32_t *)S.ft_ops.p;
                S.fa.xo = (uint8_t *)out->x.p;
                hipLaunchKernelGGL(bam::bam_tags_ops_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.fa);
                HIPCHK(ctx, hipGetLastError());
                hipLaunchKernelGGL(bam::bam_tags_extract_write_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.fa);
            } else {
                S.xa.o = (uint8_t *)out->x.p;
                hipLaunchKernelGGL(bam::bam_extract_write_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, S.xa);
            }
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

// FADEHIP_BAM_REPORT_*, C of call k: the stage's ctl has crossed with the counts (what fails the call has been looked at); the
// stats sides' alignments class by class, the rows' sizes and the scans — then the ONE wait a report call adds to a
// FROM_TAGS | EXTRACT | NO_OUTPUT call, for the reports' bytes, which size the buffers the rows are written and copied into
int bam_finish_report(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, uint64_t k, hipStream_t q) {
    fadehip_ctx *ctx = st->ctx;
    fadehip_bam_stream::Out *out = S.out;
    int rc;
    for (uint32_t w = 0; w < 2u; w++) {
        out->rbytes[w] = 0;
        out->rrows[w] = 0;
    }
    if (S.n_rec) {
        const bam::RepCtl c = *(const bam::RepCtl *)S.h_rp.p;
        const size_t ns = 2 * (size_t)S.n_rec;
        for (uint32_t w = 0; w < 2u; w++)
            if ((st->report & (1u << w)) && c.rows[w] && (rc = enqueue_report_sizes(ctx, q, S.rpa, w, c, S.rp_scratch, S.rpm))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(S.h_rp.p, S.rpa.ctl, sizeof(bam::RepCtl), hipMemcpyDeviceToHost, q));
        HIPCHK(ctx, hipStreamSynchronize(q));
        const bam::RepCtl *t = (const bam::RepCtl *)S.h_rp.p;
        for (uint32_t w = 0; w < 2u; w++) {
            const uint64_t rb = t->total[w];
            if (!(st->report & (1u << w)) || !c.rows[w] || !rb) continue;
            if (rb > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu report bytes in one call (at most 2^31)", (unsigned long long)rb);
            PinBuf &rh = st->rbuf[w][k % (FADEHIP_BAM_CHUNKS + 1)];
            if ((rc = reserve_roomy(ctx, out->r[w], (size_t)rb + 256)) || (rc = reserve_pinned(ctx, rh, (size_t)rb + (size_t)rb / 4 + 256))) return rc;
            S.rpa.out[w] = (uint8_t *)out->r[w].p;
            if (S.rpm && w == 0u) hipLaunchKernelGGL((bam::report_write_kernel<true>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, q, S.rpa, w, (const uint8_t *)S.rpm);
            else hipLaunchKernelGGL((bam::report_write_kernel<false>), dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, q, S.rpa, w, (const uint8_t *)nullptr);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(rh.p, out->r[w].p, (size_t)rb, hipMemcpyDeviceToHost, q));
            out->rbytes[w] = (size_t)rb;
            out->rrows[w] = (int64_t)c.rows[w];
        }
    }
    if (!out->rready) HIPCHK(ctx, hipEventCreateWithFlags(&out->rready, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    HIPCHK(ctx, hipEventRecord(out->rready, q));
    return 0;
}

// C of call k (see fadehip_bam_stream): waits for the call's run and tag sizes, sizes the output, enqueues the rewrite.
// Idempotent; front and back may both arrive here for the same call.
int bam_finish_one(fadehip_bam_stream *st, uint64_t k) {
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
        if (st->from_tags) {
            HIPCHK(ctx, hipStreamSynchronize(q));  // the stage, the eject kernels, the scans, the counts
            const bam::StageCounts *sc = (const bam::StageCounts *)(S.h_counts.p + st->stage_counts_at());
            std::lock_guard<std::mutex> l(st->mu);
            if (sc->bad) {
                const long long rec = (long long)st->n_records + (long long)(0xffffffffu - (uint32_t)(sc->bad >> 8));
                const uint32_t kind = (uint32_t)(sc->bad & 0xffu);
                return set_err(ctx, FADEHIP_E_INVALID, "bam stream: record %lld: malformed am tag (%s)", rec,
                               kind == bam::FT_BAD_CLIP ? "rs names a side whose CIGAR is missing or does not parse"
                               : kind == bam::FT_BAD_OPS ? "a side holds more than 65535 CIGAR ops" : "rs names a side that is not name,pos,cigar");
            }
            if (st->report && ((const bam::RepCtl *)S.h_rp.p)->bad) return report_bad(ctx, ((const bam::RepCtl *)S.h_rp.p)->bad, (long long)st->n_records);
            if (st->names && S.h_ns.p && ((const unsigned long long *)S.h_ns.p)[bam::NS_ERR])
                return set_err(ctx, FADEHIP_E_STATE, "bam stream: the name set's table or arena was full (names may be missing: the set cannot be used)");
            if (st->mates && S.h_ns.p && ((const unsigned long long *)S.h_ns.p)[4 + bam::NS_ERR])
                return set_err(ctx, FADEHIP_E_STATE, "bam stream: the mate set's table or arena was full (placements may be missing: the set cannot be used)");
            for (int t = 0; t < 8; t++) st->stats[t] += (int64_t)sc->stats[t];
            st->n_fixed += (int64_t)(sc->mates & 0xffffffffull);
            st->n_mate_ambiguous += (int64_t)(sc->mates >> 32);
            st->n_calmd_updated += (int64_t)(sc->calmd & 0xffffffffull);
            st->n_calmd_skipped += (int64_t)(sc->calmd >> 32);
        } else if (S.n_sent) {
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
        std::unique_lock<std::mutex> store_lock;  // store_output: the store's, from the reservation until the append is enqueued
        bool write = true;
        if (st->store_output) {
            // FADEHIP_BAM_STORE_OUTPUT: as bam_finish_extract does for the extract records — the call's bytes and records
            // (pad2: what bam_sortwin_kernel counted) are reserved here, in call order and with numbers that have crossed to the
            // host; the untouched rewrite kernel then writes at the arena's reserved place and the append kernels make the items.
            // A store that measures goes OVER instead of failing: its contents are dropped and nothing more is written.
            fadehip_recstore *rs = st->recstore;
            const uint64_t n_keep = h_counts->pad2 & 0xffffffffull;
            if (out_bytes > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu output bytes in one call (at most 2^31)", (unsigned long long)out_bytes);
            store_lock = std::unique_lock<std::mutex>(rs->mu);
            if (!rs->over && rs->measuring && rs->budget_set && recstore::sortwin_cost(rs->used + out_bytes, rs->n_items + n_keep) > rs->budget) {
                rs->over = true;
                rs->used = 0;
                rs->n_items = 0;
            }
            write = !rs->over;
            if (write) {
                if ((rc = recstore_room(rs, q, out_bytes, n_keep)) || (rc = reserve_roomy(ctx, S.rx_cnt, 8 * (size_t)S.ntb + 8))) return rc;
                S.ta.o = (uint8_t *)rs->arena.p + rs->used;
                S.fa.o = S.ta.o;
            }
        } else if (st->keep_sorted) {
            // the order check first: nothing of a call that fails it is written.  The rewrite then goes to the staging bytes,
            // from where the move takes the records; what leaves is sized there
            const unsigned long long bad = ((const bam::ResortCtl *)S.h_rs.p)->bad;
            if (bad)
                return set_err(ctx, FADEHIP_E_INVALID, "bam stream: record %lld: not in coordinate order (--keep-sorted needs coordinate-sorted input)",
                               (long long)st->n_records + (long long)(0xffffffffu - (uint32_t)(bad >> 8)));
            if (out_bytes > ((uint64_t)1 << 32)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu bytes of records in one call (at most 2^32)", (unsigned long long)out_bytes);
            if ((rc = reserve_roomy(ctx, S.rs_stage, (size_t)out_bytes + 256))) return rc;
            S.ta.o = (uint8_t *)S.rs_stage.p;
            S.fa.o = (uint8_t *)S.rs_stage.p;
        } else {
            if (out_bytes > ((uint64_t)1 << 31)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "bam stream: %llu output bytes in one call (at most 2^31)", (unsigned long long)out_bytes);
            if ((rc = reserve_roomy(ctx, out->o, (size_t)out_bytes + 256))) return rc;
            S.ta.o = (uint8_t *)out->o.p;
            S.fa.o = (uint8_t *)out->o.p;
        }
        if (!write) {
        } else if (st->fix_mates) {  // (under the set's lock: the arena may have moved since the plan, and must not move before this launch has run)
            fadehip_nameset *ms = &st->mates->core;
            std::lock_guard<std::mutex> ml(ms->mu);
            S.fa.ms = nameset_ref(ms);
            S.fa.fix = (const bam::MateFix *)S.mt_fix.p;
            if (st->calmd) hipLaunchKernelGGL(bam::bam_tags_calmd_write_kernel<true>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.fa, calmd_write_args(ctx, S.cm_fix));
            else hipLaunchKernelGGL((bam::bam_tags_write_kernel<true, true>), dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.fa);
        } else if (st->from_tags && st->clip) {  // (calmd is open's to refuse without the two)
            if (st->calmd) hipLaunchKernelGGL(bam::bam_tags_calmd_write_kernel<false>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.fa, calmd_write_args(ctx, S.cm_fix));
            else hipLaunchKernelGGL(bam::bam_tags_write_kernel<true>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.fa);
        }
        else if (st->from_tags) hipLaunchKernelGGL(bam::bam_tags_write_kernel<false>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.fa);
        else if (st->clip) hipLaunchKernelGGL(bam::bam_rewrite_kernel<true>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.ta);
        else hipLaunchKernelGGL(bam::bam_rewrite_kernel<false>, dim3(S.ntb), dim3(bam::REWRITE_WAVES * 64), 0, q, S.ta);
        HIPCHK(ctx, hipGetLastError());
        out->bytes = (size_t)out_bytes;
        if (st->store_output) {
            fadehip_recstore *rs = st->recstore;
            const uint32_t n_keep = (uint32_t)h_counts->pad2;
            rs->n_reset += h_counts->pad2 >> 32;
            if (write && n_keep) {
                if ((rc = enqueue_recstore_append(rs, q, rs->used, rs->n_items, S.n_rec, n_keep, (const uint32_t *)S.out_size.p, (const uint64_t *)S.blk64.p + S.ntb, (uint32_t *)S.rx_cnt.p))) return rc;
                if (st->clip) {  // (a reset record's item: the key it leaves with, not the one its zero-filled bytes spell)
                    bam::RecAppendArgs ka;
                    memset(&ka, 0, sizeof ka);
                    ka.s = recstore_ref(rs);
                    ka.item0 = rs->n_items;
                    ka.n = S.n_rec;
                    ka.n_items = n_keep;
                    ka.x_size = (const uint32_t *)S.out_size.p;
                    ka.cnt_base = (uint32_t *)S.rx_cnt.p + S.ntb;
                    hipLaunchKernelGGL(bam::bam_sortwin_rekey_kernel, dim3(S.ntb), dim3(bam::TAG_BLOCK), 0, q, ka, (const uint64_t *)S.sw_key.p);
                    HIPCHK(ctx, hipGetLastError());
                }
                rs->used += out_bytes;
                rs->n_items += n_keep;
            }
            store_lock.unlock();
            out->bytes = 0;  // (nothing for the compressor: back hands out 0 bytes)
        }
        std::lock_guard<std::mutex> l(st->mu);
        st->n_records += S.n_rec;
        st->n_ejected += h_counts->n_ejected;
    } else if (st->keep_sorted) {
        HIPCHK(ctx, hipStreamSynchronize(q));  // (an empty call: the ctl alone)
    }
    if (st->keep_sorted && (rc = bam_finish_resort(st, S, k, q))) return rc;
    if (st->index && (rc = bam_finish_index(st, S, q))) return rc;
    if (!out->ready) HIPCHK(ctx, hipEventCreateWithFlags(&out->ready, hipEventDisableTiming | (ctx->blocking_sync ? hipEventBlockingSync : 0)));
    HIPCHK(ctx, hipEventRecord(out->ready, q));
    if (st->extract && (rc = bam_finish_extract(st, S, k, q))) return rc;
    if (st->report && (rc = bam_finish_report(st, S, k, q))) return rc;
    S.pending = false;
    st->t_tags += now_s() - t0;
    {
        std::lock_guard<std::mutex> l(st->mu);
        out->state = 2;
    }
    st->cv.notify_all();
    return 0;
}

// Under FADEHIP_BAM_KEEP_SORTED call k's move reads the hold that call k - 1's move writes, so the calls are finished in
// their order (they are anyway: back takes them in order, and front finishes k - 2 before k - 1 exists; this says so).
int bam_finish_call(fadehip_bam_stream *st, uint64_t k) {
    int rc;
    if ((st->keep_sorted || st->store_extract || st->store_output) && k && (rc = bam_finish_one(st, k - 1))) return rc;  // (store_extract: a call's place in the store is handed out when it is finished)
    return bam_finish_one(st, k);
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
    // (eject: the scan comes behind the eject kernels, which come behind the extract sizes — see below; store_output: behind
    // the window kernel, which comes behind those)
    if (!st->eject) {
        if (st->store_output && (rc = enqueue_sortwin(st, S, q, n_rec, ntb, ta.out_size, pa.info, ta.blk_sums))) return rc;
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
        if (st->store_output && (rc = enqueue_sortwin(st, S, q, n_rec, ntb, ta.out_size, pa.info, ta.blk_sums))) return rc;
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
    bound_counted_batch(s, n_sent, h_counts->l_seq_min, h_counts->l_seq_max, h_counts->n_long_q, h_counts->span_max);
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

// B of call k under FADEHIP_BAM_FROM_TAGS: nothing is packed, gated or aligned — the stage kernel of bam_from_tags.hpp reads
// rs and am out of the records, then the eject kernels (untouched: sent_of = nullptr, the stage's byte per record), the
// scans, and the counts to the host, the stage's own behind the call's
int bam_front_tags(fadehip_bam_stream *st, fadehip_bam_stream::Set &S, Slot &s, uint32_t n_rec) {
    fadehip_ctx *ctx = st->ctx;
    hipStream_t q = s.stream;
    const bam::PackArgs &pa = S.pa;
    const bam::ChunkCounts *h_counts = (const bam::ChunkCounts *)S.h_counts.p;
    bam::ChunkCounts *d_counts = pa.counts;
    int rc;
    const uint32_t ntb = (n_rec + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    if (h_counts->n_bad_layout)
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: call %llu: %u records whose fields do not fit their block_size or whose tags are not whole fields (corrupt BAM)", (unsigned long long)st->k_front, h_counts->n_bad_layout);
    const size_t n = n_rec;
    if ((rc = reserve_roomy(ctx, S.blk64, 16 * (size_t)ntb)) || (rc = reserve_roomy(ctx, S.ft_rec, 9 * n + 16))) return rc;
    bam::FromTagsArgs &fa = S.fa;
    memset(&fa, 0, sizeof fa);
    fa.u = pa.u;
    fa.rec_off = pa.rec_off;
    fa.counts_in = d_counts;
    fa.r1_cap = n_rec;
    fa.mode = (st->clip ? bam::FT_CLIP : 0u) | (st->eject && !st->eject_groups ? bam::FT_EJECT_RECORDS : 0u) | (st->extract ? bam::FT_EXTRACT : 0u);
    fa.info = pa.info;
    fa.names.bytes = (const uint8_t *)st->names_text.p;
    fa.names.off = (const uint32_t *)st->names_off.p;
    fa.names.first = (const int32_t *)st->names_first.p;
    fa.names.n_ref = st->n_ref;
    fa.trim_l = (uint32_t *)S.ft_rec.p;
    fa.trim_r = fa.trim_l + n;
    fa.rsb = (uint8_t *)(fa.trim_r + n);
    fa.out_size = (uint32_t *)S.out_size.p;
    fa.blk_sums = (uint64_t *)S.blk64.p;
    fa.blk_base = fa.blk_sums + ntb;
    fa.sc = (bam::StageCounts *)((uint8_t *)d_counts + st->stage_counts_at());
    if (st->extract) {
        // per side: pos i64 | tid i32 | cnt u32 | cig_at u32
        if ((rc = reserve_roomy(ctx, S.ex_size, 4 * n)) || (rc = reserve_roomy(ctx, S.ex_blk, 16 * (size_t)ntb)) || (rc = reserve_roomy(ctx, S.ft_side, 40 * n + 16)) ||
            (rc = reserve_roomy(ctx, S.ft_ops_blk, 16 * (size_t)ntb)) || (rc = reserve_roomy(ctx, S.ft_ops_at, 8 * n)))
            return rc;
        fa.x_size = (uint32_t *)S.ex_size.p;
        fa.x_blk_sums = (uint64_t *)S.ex_blk.p;
        fa.x_blk_base = fa.x_blk_sums + ntb;
        fa.x_counts = d_counts + 1;
        fa.pos = (int64_t *)S.ft_side.p;
        fa.tid = (int32_t *)(fa.pos + 2 * n);
        fa.cnt = (uint32_t *)(fa.tid + 2 * n);
        fa.cig_at = fa.cnt + 2 * n;
        fa.ops_blk_sums = (uint64_t *)S.ft_ops_blk.p;
        fa.ops_blk_base = fa.ops_blk_sums + ntb;
        fa.ops_at = (uint64_t *)S.ft_ops_at.p;
    }
    hipLaunchKernelGGL(bam::bam_tags_stage_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, fa);
    HIPCHK(ctx, hipGetLastError());
    // the scans are bam_tag_scan_kernel's, over TagArgs that name the sums, the bases and where the total goes
    bam::TagArgs &ta = S.ta;
    memset(&ta, 0, sizeof ta);
    ta.blk_sums = fa.blk_sums;
    ta.blk_base = fa.blk_base;
    ta.counts = d_counts;
    if (st->extract) {
        bam::TagArgs xa = ta;
        xa.blk_sums = fa.x_blk_sums;
        xa.blk_base = fa.x_blk_base;
        xa.counts = d_counts + 1;
        hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, xa, ntb);
        HIPCHK(ctx, hipGetLastError());
        xa.blk_sums = fa.ops_blk_sums;
        xa.blk_base = fa.ops_blk_base;
        xa.counts = &fa.sc->ops;
        hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, xa, ntb);
        HIPCHK(ctx, hipGetLastError());
    }
    if (st->eject) {
        bam::EjectArgs ea;
        memset(&ea, 0, sizeof ea);
        ea.u = pa.u;
        ea.off32 = pa.rec_off;
        ea.n = n_rec;
        ea.sent_of = nullptr;  // (rs is per record here)
        ea.rs = fa.rsb;
        ea.out_size = fa.out_size;
        ea.info = pa.info;
        ea.blk_sums = fa.blk_sums;
        ea.counts = d_counts;
        if (st->eject_groups) {
            if ((rc = reserve_roomy(ctx, S.ej_head, 4 * n)) || (rc = reserve_roomy(ctx, S.ej_blk, 8 * (size_t)ntb)) || (rc = reserve_roomy(ctx, S.ej_grp, 4 * n))) return rc;
            ea.head_of = (uint32_t *)S.ej_head.p;
            ea.blk_head = (uint32_t *)S.ej_blk.p;
            ea.blk_carry = ea.blk_head + ntb;
            ea.grp = (uint32_t *)S.ej_grp.p;
        }
        if ((rc = enqueue_eject(ctx, q, ea, ntb, st->eject_groups))) return rc;
    }
    if (st->collect_names || st->eject_named) {
        // Under the set's lock: what the launch names of the set stays as it is until the launch has run (growth waits for
        // the device under the same lock).  COLLECT: room first, from the call's bounds — at most n_rec names, of at most
        // min(256 n_rec, the call's record bytes) bytes; the other slot's insert may run beside this one, a rehash never.
        // EJECT_NAMED: the decision, in front of the scan as bam_eject_apply_kernel's.
        fadehip_nameset *ns = st->names;
        if ((rc = reserve_pinned(ctx, S.h_ns, 64))) return rc;
        std::lock_guard<std::mutex> sl(ns->mu);
        bam::NameArgs na;
        memset(&na, 0, sizeof na);
        na.u = pa.u;
        na.off32 = pa.rec_off;
        na.n = n_rec;
        na.counts_in = d_counts;
        if (st->collect_names) {
            if ((rc = nameset_room(ns, q, n, std::min<uint64_t>(256 * (uint64_t)n, h_counts->consumed), 4))) return rc;
            na.s = nameset_ref(ns);
            na.pick = fa.rsb;
            na.pick_mask = 6u;
            hipLaunchKernelGGL(bam::bam_names_insert_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, na);
        } else {
            na.s = nameset_ref(ns);
            na.out_size = fa.out_size;
            na.info = pa.info;
            na.blk_sums = fa.blk_sums;
            na.counts = d_counts;
            hipLaunchKernelGGL(bam::bam_eject_named_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, na);
        }
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(S.h_ns.p, ns->ctrl.p, 24, hipMemcpyDeviceToHost, q));
    }
    if (st->collect_mates || st->fix_mates) {
        // Under the sets' locks, as above (the name set's first).  COLLECT_MATES: the name look-up, room in the map from the
        // call's bounds — at most n_rec entries of at most key 260 + fixed 24 + padding 3 + two H ops 22 bytes and 11 bytes for
        // each of the call's CIGAR ops, of which there are at most a quarter of its record bytes — then the insert.
        // FIX_MATES: the plan, in front of the scan.  The write kernel gets the map as it is when IT is launched (bam_finish_call).
        fadehip_nameset *ms = &st->mates->core;
        if ((rc = reserve_pinned(ctx, S.h_ns, 64))) return rc;
        bam::MateArgs ma;
        memset(&ma, 0, sizeof ma);
        ma.u = pa.u;
        ma.off32 = pa.rec_off;
        ma.n = n_rec;
        ma.counts_in = d_counts;
        ma.rs = fa.rsb;
        ma.trim_l = fa.trim_l;
        ma.trim_r = fa.trim_r;
        if (st->collect_mates) {
            fadehip_nameset *ns = st->names;
            if ((rc = reserve_roomy(ctx, S.mt_hit, n + 8))) return rc;
            std::lock_guard<std::mutex> nl(ns->mu);
            std::lock_guard<std::mutex> ml(ms->mu);
            bam::NameArgs na;
            memset(&na, 0, sizeof na);
            na.s = nameset_ref(ns);
            na.u = pa.u;
            na.off32 = pa.rec_off;
            na.n = n_rec;
            na.counts_in = d_counts;
            na.hit = (uint8_t *)S.mt_hit.p;
            hipLaunchKernelGGL(bam::bam_names_lookup_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, na);
            HIPCHK(ctx, hipGetLastError());
            if ((rc = nameset_room(ms, q, n, 312 * (uint64_t)n + 3 * (uint64_t)h_counts->consumed, 4))) return rc;
            ma.s = nameset_ref(ms);
            ma.pick = na.hit;
            hipLaunchKernelGGL(bam::bam_mates_insert_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ma);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(S.h_ns.p, ns->ctrl.p, 32, hipMemcpyDeviceToHost, q));
        } else {
            if ((rc = reserve_roomy(ctx, S.mt_fix, sizeof(bam::MateFix) * n + 8))) return rc;
            std::lock_guard<std::mutex> ml(ms->mu);
            ma.s = nameset_ref(ms);
            ma.info = pa.info;
            ma.fix = (bam::MateFix *)S.mt_fix.p;
            ma.out_size = fa.out_size;
            ma.blk_sums = fa.blk_sums;
            ma.n_mates = &fa.sc->mates;
            hipLaunchKernelGGL(bam::bam_mates_plan_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ma);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipMemcpyAsync(S.h_ns.p + 32, ms->ctrl.p, 32, hipMemcpyDeviceToHost, q));
    }
    if (st->calmd) {  // behind the mate plan (whose out_size it corrects further), in front of the scan that reads the sizes
        if (ctx->n_contigs == 0) return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_CALMD and no genome uploaded (fadehip_genome_upload / fadehip_genome_upload_fasta)");
        if ((rc = reserve_roomy(ctx, S.cm_fix, sizeof(bam::CalmdFix) * n + 8))) return rc;
        bam::CalmdArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.g = genome_ref(ctx);
        ca.u = pa.u;
        ca.off32 = pa.rec_off;
        ca.n = n_rec;
        ca.counts_in = d_counts;
        ca.rs = fa.rsb;
        ca.trim_l = fa.trim_l;
        ca.trim_r = fa.trim_r;
        ca.info = pa.info;
        ca.blk_sums = fa.blk_sums;
        ca.n_calmd = &fa.sc->calmd;
        ca.fix = (bam::CalmdFix *)S.cm_fix.p;
        ca.out_size = fa.out_size;
        hipLaunchKernelGGL(bam::bam_calmd_plan_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ca);
        HIPCHK(ctx, hipGetLastError());
    }
    if (st->store_output && (rc = enqueue_sortwin(st, S, q, n_rec, ntb, fa.out_size, pa.info, fa.blk_sums))) return rc;
    hipLaunchKernelGGL(bam::bam_tag_scan_kernel, dim3(1), dim3(1024), 0, q, ta, ntb);
    HIPCHK(ctx, hipGetLastError());
    if (st->report) {  // the reports' stage (bam_report.hpp); its ctl crosses with the counts
        bam::RepArgs &ra = S.rpa;
        memset(&ra, 0, sizeof ra);
        S.rpm = nullptr;
        uint8_t **rpm = st->repeats ? &S.rpm : nullptr;
        if ((rc = reserve_roomy(ctx, S.rp, report_layout(ra, nullptr, n, st->report, rpm))) || (rc = reserve_pinned(ctx, S.h_rp, 128))) return rc;
        report_layout(ra, (uint8_t *)S.rp.p, n, st->report, rpm);
        ra.base = pa.u;
        ra.off32 = pa.rec_off;
        ra.n = n_rec;
        ra.which = st->report;
        ra.names = fa.names;
        HIPCHK(ctx, hipMemsetAsync(ra.ctl, 0, 128, q));
        hipLaunchKernelGGL(bam::report_stage_kernel, dim3(ntb), dim3(bam::TAG_BLOCK), 0, q, ra);
        HIPCHK(ctx, hipGetLastError());
        if (st->repeats && (rc = enqueue_report_repeats(ctx, q, ra, st->intervals, (const int32_t *)st->ref_chrom.p, S.rpm))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(S.h_rp.p, ra.ctl, sizeof(bam::RepCtl), hipMemcpyDeviceToHost, q));
    }
    HIPCHK(ctx, hipMemcpyAsync(S.h_counts.p, d_counts, st->counts_bytes(), hipMemcpyDeviceToHost, q));
    S.n_sent = 0;
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
    if (ctx->n_contigs == 0 && !st->from_tags) return set_err(ctx, FADEHIP_E_STATE, "fadehip_genome_upload has not been called");
    if ((st->collect_names || st->eject_named || st->collect_mates) && !st->names)
        return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_%s and no name set attached (fadehip_bam_use_nameset)",
                       st->collect_names ? "COLLECT_NAMES" : st->eject_named ? "EJECT_NAMED" : "COLLECT_MATES");
    if (st->repeats && !st->intervals)
        return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_REPORT_REPEATS and no set of intervals attached (fadehip_bam_use_intervals)");
    if (st->store_extract && !st->recstore)
        return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_STORE_EXTRACT and no record store attached (fadehip_bam_use_recstore)");
    if (st->store_output && !st->recstore)
        return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_STORE_OUTPUT and no record store attached (fadehip_bam_use_recstore)");
    if ((st->collect_mates || st->fix_mates) && !st->mates)
        return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened with FADEHIP_BAM_%s and no mate set attached (fadehip_bam_use_mateset)", st->collect_mates ? "COLLECT_MATES" : "FIX_MATES");
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
    if (n_rec && (rc = st->from_tags ? bam_front_tags(st, S, s, n_rec) : bam_front_run(st, S, s, tr, n_rec))) return rc;
    if (st->keep_sorted && (rc = bam_front_resort(st, k, n_rec, last))) return rc;
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
    if (!cfg || !out || cfg->n_ref < 0 || (cfg->n_ref && !cfg->ref_names) || (cfg->window < 0 && !(cfg->flags & FADEHIP_BAM_FROM_TAGS)) ||
        (cfg->flags & ~(FADEHIP_BAM_STORED | FADEHIP_BAM_NO_OUTPUT | FADEHIP_BAM_CLIP | FADEHIP_BAM_EXTRACT | FADEHIP_BAM_EJECT | FADEHIP_BAM_EJECT_GROUPS | FADEHIP_BAM_FROM_TAGS |
                        FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_EJECT_NAMED | FADEHIP_BAM_KEEP_SORTED | FADEHIP_BAM_REPORT_STATS | FADEHIP_BAM_REPORT_CLIP | FADEHIP_BAM_INDEX |
                        FADEHIP_BAM_COLLECT_MATES | FADEHIP_BAM_FIX_MATES | FADEHIP_BAM_STORE_EXTRACT | FADEHIP_BAM_REPORT_REPEATS | FADEHIP_BAM_STORE_OUTPUT | FADEHIP_BAM_CALMD)))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: bad configuration");
    if (cfg->flags & FADEHIP_BAM_STORE_OUTPUT) {
        // the store takes the records a stream writes, and gives them an order of its own: what writes nothing, what writes
        // elsewhere and what keeps or indexes the stream's own order do not stand beside it
        static const struct { int32_t flag; const char *name; } no[] = {
            {FADEHIP_BAM_NO_OUTPUT, "FADEHIP_BAM_NO_OUTPUT"}, {FADEHIP_BAM_STORED, "FADEHIP_BAM_STORED"}, {FADEHIP_BAM_KEEP_SORTED, "FADEHIP_BAM_KEEP_SORTED"},
            {FADEHIP_BAM_INDEX, "FADEHIP_BAM_INDEX"}, {FADEHIP_BAM_STORE_EXTRACT, "FADEHIP_BAM_STORE_EXTRACT"}, {FADEHIP_BAM_EXTRACT, "FADEHIP_BAM_EXTRACT"},
            {FADEHIP_BAM_COLLECT_NAMES, "FADEHIP_BAM_COLLECT_NAMES"}, {FADEHIP_BAM_COLLECT_MATES, "FADEHIP_BAM_COLLECT_MATES"},
            {FADEHIP_BAM_REPORT_REPEATS, "FADEHIP_BAM_REPORT_REPEATS"}, {FADEHIP_BAM_REPORT_STATS, "FADEHIP_BAM_REPORT_STATS"}, {FADEHIP_BAM_REPORT_CLIP, "FADEHIP_BAM_REPORT_CLIP"}};
        for (const auto &f : no)
            if (cfg->flags & f.flag)
                return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_STORE_OUTPUT does not combine with %s (it stands with FROM_TAGS, CLIP, EJECT, EJECT_GROUPS, EJECT_NAMED and FIX_MATES)", f.name);
    }
    if ((cfg->flags & FADEHIP_BAM_REPORT_REPEATS) && !(cfg->flags & FADEHIP_BAM_REPORT_STATS))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_REPORT_REPEATS needs FADEHIP_BAM_REPORT_STATS (it adds two columns to that report's rows)");
    if ((cfg->flags & FADEHIP_BAM_STORE_EXTRACT) && !(cfg->flags & FADEHIP_BAM_EXTRACT))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_STORE_EXTRACT needs FADEHIP_BAM_EXTRACT (it says where the extract records go)");
    // the index describes records that are written: a stream that writes none has nothing to index.  It stands beside every
    // flag that writes output, and the checks below look at the flags without it
    const int32_t all_flags = cfg->flags;
    if (all_flags & FADEHIP_BAM_INDEX) {
        const char *no = (all_flags & FADEHIP_BAM_NO_OUTPUT) ? "FADEHIP_BAM_NO_OUTPUT" : (all_flags & FADEHIP_BAM_REPORT_STATS) ? "FADEHIP_BAM_REPORT_STATS"
                         : (all_flags & FADEHIP_BAM_REPORT_CLIP) ? "FADEHIP_BAM_REPORT_CLIP" : (all_flags & FADEHIP_BAM_COLLECT_NAMES) ? "FADEHIP_BAM_COLLECT_NAMES" : nullptr;
        if (no) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_INDEX does not combine with %s (the index is of the records a stream writes)", no);
    }
    // (STORE_EXTRACT only says where EXTRACT's records go: it stands wherever EXTRACT does)
    fadehip_bam_config cfg_plain = *cfg;
    // (REPORT_REPEATS stands wherever REPORT_STATS does; STORE_OUTPUT only says where the output goes: what it excludes was refused above)
    cfg_plain.flags &= ~(FADEHIP_BAM_INDEX | FADEHIP_BAM_STORE_EXTRACT | FADEHIP_BAM_REPORT_REPEATS | FADEHIP_BAM_STORE_OUTPUT);
    cfg = &cfg_plain;
    if (cfg->flags & FADEHIP_BAM_CALMD) {
        // NM and MD follow the clip of a stream that reads its calls from the tags; the flag only says what the clipped records'
        // two fields hold, so it stands beside what a clipping FROM_TAGS stream stands beside, and the checks below look at the
        // flags without it
        const int32_t need = FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP;
        if ((cfg->flags & need) != need || (all_flags & FADEHIP_BAM_STORE_OUTPUT) ||
            (cfg->flags & ~(need | FADEHIP_BAM_CALMD | FADEHIP_BAM_STORED | FADEHIP_BAM_FIX_MATES | FADEHIP_BAM_KEEP_SORTED | FADEHIP_BAM_NO_OUTPUT)))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_CALMD needs FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP and combines with STORED, FIX_MATES, KEEP_SORTED, INDEX and NO_OUTPUT only");
        cfg_plain.flags &= ~FADEHIP_BAM_CALMD;
    }
    if (cfg->flags & (FADEHIP_BAM_REPORT_STATS | FADEHIP_BAM_REPORT_CLIP)) {
        const int32_t need = FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_NO_OUTPUT;
        if ((cfg->flags & need) != need || (cfg->flags & ~(need | FADEHIP_BAM_STORED | FADEHIP_BAM_REPORT_STATS | FADEHIP_BAM_REPORT_CLIP)))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_REPORT_STATS and FADEHIP_BAM_REPORT_CLIP need FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_NO_OUTPUT and combine with STORED only");
    }
    if (cfg->flags & FADEHIP_BAM_COLLECT_MATES) {
        const int32_t need = FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP | FADEHIP_BAM_NO_OUTPUT;
        if ((cfg->flags & need) != need || (cfg->flags & ~(need | FADEHIP_BAM_COLLECT_MATES | FADEHIP_BAM_STORED)))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_COLLECT_MATES needs FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP | FADEHIP_BAM_NO_OUTPUT and combines with STORED only");
    }
    if (cfg->flags & FADEHIP_BAM_FIX_MATES) {
        const int32_t need = FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP;
        if ((cfg->flags & need) != need || (cfg->flags & ~(need | FADEHIP_BAM_FIX_MATES | FADEHIP_BAM_STORED | FADEHIP_BAM_KEEP_SORTED)))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_FIX_MATES needs FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_CLIP and combines with STORED, KEEP_SORTED and INDEX only");
    }
    if (cfg->flags & FADEHIP_BAM_KEEP_SORTED) {
        if (!(cfg->flags & FADEHIP_BAM_CLIP)) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_KEEP_SORTED needs FADEHIP_BAM_CLIP (without a clip nothing moves)");
        if (cfg->flags & ~(FADEHIP_BAM_KEEP_SORTED | FADEHIP_BAM_CLIP | FADEHIP_BAM_STORED | FADEHIP_BAM_EXTRACT | FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_FIX_MATES))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_KEEP_SORTED combines with CLIP, STORED, EXTRACT, FROM_TAGS and FIX_MATES only");
    }
    if (cfg->flags & (FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_EJECT_NAMED)) {
        const int32_t one = cfg->flags & (FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_EJECT_NAMED);
        if (one == (FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_EJECT_NAMED) || !(cfg->flags & FADEHIP_BAM_FROM_TAGS) ||
            (cfg->flags & ~(one | FADEHIP_BAM_FROM_TAGS | FADEHIP_BAM_STORED | FADEHIP_BAM_NO_OUTPUT)))
            return set_err(ctx, FADEHIP_E_INVALID, "bam stream: FADEHIP_BAM_COLLECT_NAMES and FADEHIP_BAM_EJECT_NAMED need FADEHIP_BAM_FROM_TAGS, exclude each other, and combine with STORED and NO_OUTPUT only");
    }
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
    st->from_tags = (cfg->flags & FADEHIP_BAM_FROM_TAGS) != 0;
    st->collect_names = (cfg->flags & FADEHIP_BAM_COLLECT_NAMES) != 0;
    st->eject_named = (cfg->flags & FADEHIP_BAM_EJECT_NAMED) != 0;
    st->keep_sorted = (cfg->flags & FADEHIP_BAM_KEEP_SORTED) != 0;
    st->collect_mates = (cfg->flags & FADEHIP_BAM_COLLECT_MATES) != 0;
    st->fix_mates = (cfg->flags & FADEHIP_BAM_FIX_MATES) != 0;
    st->calmd = (all_flags & FADEHIP_BAM_CALMD) != 0;
    st->report = ((cfg->flags & FADEHIP_BAM_REPORT_STATS) ? bam::RP_STATS : 0u) | ((cfg->flags & FADEHIP_BAM_REPORT_CLIP) ? bam::RP_CLIP : 0u);
    st->index = (all_flags & FADEHIP_BAM_INDEX) != 0;
    st->store_extract = (all_flags & FADEHIP_BAM_STORE_EXTRACT) != 0;
    st->store_output = (all_flags & FADEHIP_BAM_STORE_OUTPUT) != 0;
    st->repeats = (all_flags & FADEHIP_BAM_REPORT_REPEATS) != 0;
    std::string text;
    std::vector<uint32_t> off((size_t)cfg->n_ref + 1, 0);
    for (int k = 0; k < cfg->n_ref; k++) {
        if (!cfg->ref_names[k]) { delete st; return set_err(ctx, FADEHIP_E_INVALID, "bam stream: ref_names[%d] is NULL", k); }
        if (st->repeats) st->ref_names_h.push_back(cfg->ref_names[k]);
        off[(size_t)k] = (uint32_t)text.size();
        text += cfg->ref_names[k];
    }
    off[(size_t)cfg->n_ref] = (uint32_t)text.size();
    int rc;
    if (st->from_tags) {  // a header that names a contig twice: the first of that name is meant (fadehip_tags_batch's rule)
        std::vector<int32_t> first((size_t)cfg->n_ref);
        std::map<std::string, int32_t> seen;
        for (int32_t k = 0; k < cfg->n_ref; k++) first[(size_t)k] = seen.emplace(cfg->ref_names[k], k).first->second;
        if ((rc = reserve(ctx, st->names_first, 4 * first.size() + 4))) { fadehip_bam_close(st); return rc; }
        if (cfg->n_ref && (hipMemcpyAsync(st->names_first.p, first.data(), 4 * first.size(), hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
                           hipStreamSynchronize(ctx->copy_stream) != hipSuccess)) {
            fadehip_bam_close(st);
            return set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the contig names failed");
        }
    }
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

int fadehip_bam_use_nameset(fadehip_bam_stream *st, fadehip_nameset *s) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!s) return set_err(ctx, FADEHIP_E_INVALID, "nameset is NULL");
    if (s->ctx != ctx) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the name set belongs to another ctx");
    if (!st->collect_names && !st->eject_named && !st->collect_mates)
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: opened without FADEHIP_BAM_COLLECT_NAMES, FADEHIP_BAM_EJECT_NAMED or FADEHIP_BAM_COLLECT_MATES");
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: use_nameset comes before the first front call");
    st->names = s;
    return 0;
}

int fadehip_bam_use_mateset(fadehip_bam_stream *st, fadehip_mateset *m) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!m) return set_err(ctx, FADEHIP_E_INVALID, "mateset is NULL");
    if (m->core.ctx != ctx) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the mate set belongs to another ctx");
    if (!st->collect_mates && !st->fix_mates) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: opened without FADEHIP_BAM_COLLECT_MATES or FADEHIP_BAM_FIX_MATES");
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: use_mateset comes before the first front call");
    st->mates = m;
    return 0;
}

int fadehip_bam_use_recstore(fadehip_bam_stream *st, fadehip_recstore *s) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!s) return set_err(ctx, FADEHIP_E_INVALID, "recstore is NULL");
    if (s->ctx != ctx) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the record store belongs to another ctx");
    if (!st->store_extract && !st->store_output) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: opened without FADEHIP_BAM_STORE_EXTRACT or FADEHIP_BAM_STORE_OUTPUT");
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: use_recstore comes before the first front call");
    st->recstore = s;
    return 0;
}

int fadehip_bam_index_geometry(fadehip_bam_stream *st, int32_t min_shift, int32_t depth) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!st->index) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: opened without FADEHIP_BAM_INDEX");
    if (!IndexGeometry::valid(min_shift, depth))
        return set_err(ctx, FADEHIP_E_INVALID, "bam stream: CSI geometry (min_shift %d, depth %d): 4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32", (int)min_shift, (int)depth);
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: index_geometry comes before the first front call");
    st->ix_geo.min_shift = min_shift;
    st->ix_geo.depth = depth;
    return 0;
}

int fadehip_bam_use_intervals(fadehip_bam_stream *st, fadehip_intervals *s) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!s) return set_err(ctx, FADEHIP_E_INVALID, "intervals is NULL");
    if (s->ctx != ctx) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the set of intervals belongs to another ctx");
    if (!st->repeats) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: opened without FADEHIP_BAM_REPORT_REPEATS");
    if (st->k_front) return set_err(ctx, FADEHIP_E_STATE, "bam stream: use_intervals comes before the first front call");
    if (!s->sealed) return set_err(ctx, FADEHIP_E_INVALID, "bam stream: the set of intervals has not been sealed (fadehip_intervals_seal)");
    std::vector<const char *> names;
    for (const std::string &nm : st->ref_names_h) names.push_back(nm.c_str());
    const std::vector<int32_t> refc = intervals_ref_chrom(s, (int32_t)names.size(), names.data());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int rc = reserve(ctx, st->ref_chrom, 4 * refc.size())) return rc;
    if (hipMemcpyAsync(st->ref_chrom.p, refc.data(), 4 * refc.size(), hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess || hipStreamSynchronize(ctx->copy_stream) != hipSuccess)
        return set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the contigs' chrom ids failed");
    st->intervals = s;
    return 0;
}

int fadehip_bam_calmd(fadehip_bam_stream *st, int64_t *n_updated, int64_t *n_skipped) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    if (!n_updated || !n_skipped) return set_err(st->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> l(st->mu);
    *n_updated = st->n_calmd_updated;
    *n_skipped = st->n_calmd_skipped;
    return 0;
}

int fadehip_bam_mates(fadehip_bam_stream *st, int64_t *n_fixed, int64_t *n_ambiguous) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    if (!n_fixed || !n_ambiguous) return set_err(st->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> l(st->mu);
    *n_fixed = st->n_fixed;
    *n_ambiguous = st->n_mate_ambiguous;
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
    const bool with_out = !st->no_output && !st->store_output;
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
        rc = reserve_pinned(ctx, st->outbuf[q], st->stored ? bgzf_store_cap(out_est) : bgzf_out_cap(out_est, 32));
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
    if (st->stored) rc = bgzf_store_enqueue(ctx, lane, (const uint8_t *)o->o.p, o->bytes, ob);
    else rc = bgzf_enqueue(ctx, lane, (const uint8_t *)o->o.p, o->bytes, bgzf_pick_geom(ctx), &ob);
    tr.mark("compressor enqueued");
    if (!rc && st->index) rc = bam_enqueue_index(st, k, lane);
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
    if (st->index && (rc = bam_take_index(st, k, (int)(k & 1)))) {
        *out = nullptr;  // (nothing of a call that fails is handed out)
        *out_bytes = 0;
        return bam_fail(st, rc);
    }
    if (st->extract) {
        if (o->xready && hipEventSynchronize(o->xready) != hipSuccess) return bam_fail(st, set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the extract records failed"));
        st->last_x = o->xbytes ? st->xbuf[k % (FADEHIP_BAM_CHUNKS + 1)].p : nullptr;
        st->last_xbytes = o->xbytes;
        st->last_xrecs = o->xrecs;
        st->have_back = true;
    }
    if (st->report) {
        if (o->rready && hipEventSynchronize(o->rready) != hipSuccess) return bam_fail(st, set_err(ctx, FADEHIP_E_HIP, "bam stream: copying the reports' rows failed"));
        for (uint32_t w = 0; w < 2u; w++) {
            st->last_r[w] = o->rbytes[w] ? st->rbuf[w][k % (FADEHIP_BAM_CHUNKS + 1)].p : nullptr;
            st->last_rbytes[w] = o->rbytes[w];
            st->last_rrows[w] = o->rrows[w];
        }
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

int fadehip_bam_back_report(fadehip_bam_stream *st, int32_t which, const uint8_t **text, size_t *n_bytes, int64_t *n_rows) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!text || !n_bytes || !n_rows || (which != FADEHIP_BAM_REPORT_STATS && which != FADEHIP_BAM_REPORT_CLIP)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument, or which is not one report");
    *text = nullptr;
    *n_bytes = 0;
    *n_rows = 0;
    const uint32_t w = which == FADEHIP_BAM_REPORT_STATS ? 0u : 1u;
    if (!(st->report & (1u << w))) return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened without that FADEHIP_BAM_REPORT flag");
    if (!st->have_back) return set_err(ctx, FADEHIP_E_STATE, "bam stream: back_report comes after a back call");
    *text = st->last_r[w];
    *n_bytes = st->last_rbytes[w];
    *n_rows = st->last_rrows[w];
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

int fadehip_bam_held(fadehip_bam_stream *st, int64_t *n_records, int64_t *n_bytes) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    if (!n_records || !n_bytes) return set_err(st->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> l(st->mu);
    *n_records = st->held_recs;
    *n_bytes = st->held_bytes;
    return 0;
}

// The stable coordinate order of records the caller brings, in whatever order they come: bam_resort.hpp's sort, the one of the
// file path under FADEHIP_BAM_KEEP_SORTED, on the record-batch lane.  order[j] is the record that comes j-th.
int fadehip_coord_order_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t *order) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || !rec_off || (n > 0 && (!recs || !order))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, false, [](int32_t) { return 0; }))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | the ctl;  work: the stage's arrays;  out: order [n] i32
    bam::ResortArgs a;
    memset(&a, 0, sizeof a);
    const size_t m_ctl = 8 * ((size_t)n + 1);
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, nullptr, 0, m_ctl + 256, resort_layout(a, nullptr, (size_t)n), off)) || (rc = reserve(ctx, L.out, 4 * (size_t)n + 8))) return rc;
    resort_layout(a, (uint8_t *)L.work.p, (size_t)n);
    a.ctl = (bam::ResortCtl *)((uint8_t *)L.meta.p + m_ctl);
    a.n = (uint32_t)n;
    a.u = (const uint8_t *)L.in.p;
    a.rec_off64 = (const uint64_t *)L.meta.p;
    const unsigned nb = ((unsigned)n + 255u) / 256u;
    hipLaunchKernelGGL(bam::bam_resort_batch_keys_kernel, dim3(nb), dim3(256), 0, L.stream, a);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = enqueue_resort_sort(ctx, L.stream, a, (size_t)n))) return rc;
    hipLaunchKernelGGL(bam::bam_resort_order_kernel, dim3(nb), dim3(256), 0, L.stream, a, (int32_t *)L.out.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(order, L.out.p, 4 * (size_t)n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    return 0;
}

int fadehip_bam_back_index(fadehip_bam_stream *st, fadehip_index_call *out) {
    if (!st) return set_err(nullptr, FADEHIP_E_INVALID, "stream is NULL");
    fadehip_ctx *ctx = st->ctx;
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    memset(out, 0, sizeof *out);
    if (!st->index) return set_err(ctx, FADEHIP_E_STATE, "bam stream: opened without FADEHIP_BAM_INDEX");
    if (!st->have_ix) return set_err(ctx, FADEHIP_E_STATE, "bam stream: back_index comes after a back call");
    *out = st->last_ix;
    return 0;
}

// The index entries of records the caller brings, at virtual offsets the caller brings: bam_index.hpp's kernels, the ones of
// the file path under FADEHIP_BAM_INDEX, on the record-batch lane.
static int index_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff, IndexGeometry geo, fadehip_index_call *out);
int fadehip_index_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff, fadehip_index_call *out) {
    return index_batch(ctx, n, recs, rec_off, voff, IndexGeometry(), out);
}
// ... and under a CSI geometry: the key kernel of bam_index.hpp that takes one, the kernels behind it as they are
int fadehip_index_batch_csi(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff, int32_t min_shift, int32_t depth,
                            fadehip_index_call *out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!IndexGeometry::valid(min_shift, depth))
        return set_err(ctx, FADEHIP_E_INVALID, "index batch: CSI geometry (min_shift %d, depth %d): 4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32", (int)min_shift, (int)depth);
    IndexGeometry geo;
    geo.min_shift = min_shift;
    geo.depth = depth;
    return index_batch(ctx, n, recs, rec_off, voff, geo, out);
}
static int index_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff, IndexGeometry geo, fadehip_index_call *out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (n < 0 || !rec_off || !voff || !out || (n > 0 && !recs)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    memset(out, 0, sizeof *out);
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    if (n == 0) return 0;
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, [](int32_t) { return 0; }))) return rc;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    // meta: in_off [n + 1] u64 | voff [n + 1] u64 | the ctl;  work: the stage's arrays;  out: chunks | refs | linear
    bam::IndexArgs a;
    memset(&a, 0, sizeof a);
    const size_t m_voff = 8 * ((size_t)n + 1), m_ctl = 2 * m_voff;
    std::vector<uint64_t> off;
    if ((rc = batch_upload(ctx, L, n, recs, rec_off, nullptr, 0, m_ctl + 256, index_layout(a, nullptr, (size_t)n), off))) return rc;
    HIPCHK(ctx, hipMemcpyAsync((uint8_t *)L.meta.p + m_voff, voff, m_voff, hipMemcpyHostToDevice, L.stream));
    index_layout(a, (uint8_t *)L.work.p, (size_t)n);
    a.ctl = (bam::IndexCtl *)((uint8_t *)L.meta.p + m_ctl);
    a.u = (const uint8_t *)L.in.p;
    a.at = (const uint64_t *)L.meta.p;
    a.n = (uint32_t)n;
    a.voff = (const uint64_t *)((uint8_t *)L.meta.p + m_voff);
    if ((rc = enqueue_index_counts(ctx, L.stream, a, geo))) return rc;
    bam::IndexCtl c;
    HIPCHK(ctx, hipMemcpyAsync(&c, a.ctl, sizeof c, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    if ((rc = index_bad(ctx, c, 0, "index batch", geo))) return rc;
    if (c.n_linear >> 31) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "index batch: %llu linear index entries (at most 2^31)", (unsigned long long)c.n_linear);
    const size_t out_bytes = index_out_layout(a, nullptr, (size_t)n, (size_t)c.n_linear);
    if ((rc = reserve(ctx, L.out, out_bytes + 8))) return rc;
    index_out_layout(a, (uint8_t *)L.out.p, (size_t)n, (size_t)c.n_linear);
    if ((rc = enqueue_index_write(ctx, L.stream, a))) return rc;
    L.index_host.resize(out_bytes + 8);
    HIPCHK(ctx, hipMemcpyAsync(L.index_host.data(), L.out.p, out_bytes, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    bam::IndexArgs h;
    index_out_layout(h, L.index_host.data(), (size_t)n, (size_t)c.n_linear);
    out->chunks = h.chunks;
    out->linear = h.linear;
    out->refs = h.refs;
    out->n_chunks = (int64_t)c.n_chunks;
    out->n_linear = (int64_t)c.n_linear;
    out->n_refs = (int64_t)c.n_refs;
    out->n_records = (int64_t)c.n;
    out->first_key = c.first_key;
    out->last_key = c.last_key;
    return 0;
}

// ---- the host's part of the index (host/bai_build.hpp); no device is involved
struct fadehip_bai {
    fadehip::bai::Builder b;
    explicit fadehip_bai(int32_t n_ref) : b(n_ref) {}
};
static thread_local std::string g_bai_null_err;

fadehip_bai *fadehip_bai_create(int32_t n_ref) {
    if (n_ref < 0) return nullptr;
    try {
        return new fadehip_bai(n_ref);
    } catch (...) {
        return nullptr;
    }
}
int fadehip_bai_add(fadehip_bai *b, uint64_t base_file_offset, const fadehip_index_call *call) {
    if (!b) {
        g_bai_null_err = "bai: builder is NULL";
        return FADEHIP_E_INVALID;
    }
    try {
        return b->b.add(base_file_offset, call);
    } catch (...) {
        b->b.err = "bai: out of memory";
        return FADEHIP_E_NOMEM;
    }
}
int fadehip_bai_finish(fadehip_bai *b, const uint8_t **bytes, size_t *n) {
    if (!b) {
        g_bai_null_err = "bai: builder is NULL";
        return FADEHIP_E_INVALID;
    }
    try {
        return b->b.finish(bytes, n);
    } catch (...) {
        b->b.err = "bai: out of memory";
        return FADEHIP_E_NOMEM;
    }
}
const char *fadehip_bai_error(const fadehip_bai *b) { return b ? b->b.err.c_str() : g_bai_null_err.c_str(); }
void fadehip_bai_destroy(fadehip_bai *b) { delete b; }

// ... and of a CSI (host/csi_build.hpp)
struct fadehip_csi {
    fadehip::csi::Builder b;
    fadehip_csi(int32_t n_ref, int32_t min_shift, int32_t depth) : b(n_ref, min_shift, depth) {}
};
static thread_local std::string g_csi_null_err;

fadehip_csi *fadehip_csi_create(int32_t n_ref, int32_t min_shift, int32_t depth) {
    if (n_ref < 0 || !fadehip::csi::valid_geometry(min_shift, depth)) return nullptr;
    try {
        return new fadehip_csi(n_ref, min_shift, depth);
    } catch (...) {
        return nullptr;
    }
}
int fadehip_csi_add(fadehip_csi *b, uint64_t base_file_offset, const fadehip_index_call *call) {
    if (!b) {
        g_csi_null_err = "csi: builder is NULL";
        return FADEHIP_E_INVALID;
    }
    try {
        return b->b.add(base_file_offset, call);
    } catch (...) {
        b->b.err = "csi: out of memory";
        return FADEHIP_E_NOMEM;
    }
}
int fadehip_csi_finish(fadehip_csi *b, const uint8_t **payload, size_t *n) {
    if (!b) {
        g_csi_null_err = "csi: builder is NULL";
        return FADEHIP_E_INVALID;
    }
    try {
        return b->b.finish(payload, n);
    } catch (...) {
        b->b.err = "csi: out of memory";
        return FADEHIP_E_NOMEM;
    }
}
const char *fadehip_csi_error(const fadehip_csi *b) { return b ? b->b.err.c_str() : g_csi_null_err.c_str(); }
void fadehip_csi_destroy(fadehip_csi *b) { delete b; }

// ---- the record store over records the caller brings, its sort and its drains (bam_recstore.hpp)
int fadehip_recstore_create(fadehip_ctx *ctx, fadehip_recstore **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fadehip_recstore *s = new (std::nothrow) fadehip_recstore;
    if (!s) return set_err(ctx, FADEHIP_E_NOMEM, "out of memory");
    s->ctx = ctx;
    s->first_bytes = RECSTORE_DEFAULT_BYTES;
    if (const char *e = getenv("FADEHIP_RECSTORE_BYTES")) s->first_bytes = (uint64_t)std::max<long long>(256, std::min<long long>(atoll(e), 1ll << 40));
    memset(&s->ra, 0, sizeof s->ra);
    if (const int rc = recstore_alloc(ctx, s->arena, (size_t)s->first_bytes)) {
        fadehip_recstore_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

void fadehip_recstore_destroy(fadehip_recstore *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&s->arena, &s->key, &s->off, &s->size, &s->sort_arr, &s->stage, &s->at, &s->app, &s->ix_work, &s->ix_ctl, &s->ix_out, &s->table, &s->lay_dev}) release(*b);
    release(s->h_out);
    delete s;
}

int fadehip_recstore_add_batch(fadehip_recstore *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *pick) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || !rec_off || (n > 0 && !recs)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    if (rec_off[0] < 0) return set_err(ctx, FADEHIP_E_INVALID, "offsets must be non-negative and non-decreasing (record 0)");
    int rc;
    if ((rc = check_records(ctx, n, recs, rec_off, true, [](int32_t) { return 0; }))) return rc;
    // the picked records as slots of one record each: their sizes, the blocks' bases, and the runs of neighbours to copy
    const size_t ntb = ((size_t)n + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    std::vector<uint32_t> x_size((size_t)n);
    std::vector<uint64_t> blk_base(ntb + 1);
    uint64_t bytes = 0, n_pick = 0;
    for (int32_t k = 0; k < n; k++) {
        if (k % bam::TAG_BLOCK == 0) blk_base[(size_t)k / bam::TAG_BLOCK] = bytes;
        const bool in = !pick || pick[k];
        x_size[(size_t)k] = in ? (uint32_t)(rec_off[k + 1] - rec_off[k]) : 0u;
        bytes += x_size[(size_t)k];
        n_pick += in;
    }
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!L.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sorted) return set_err(ctx, FADEHIP_E_STATE, "recstore: the store has been sorted, nothing can be added to it any more");
    if (!n_pick) return 0;
    // app: x_size [n] u32 | blk_base [blocks] u64 | counts [2 blocks] u32
    const size_t a_base = (4 * (size_t)n + 7) & ~(size_t)7, a_cnt = a_base + 8 * ntb;
    if ((rc = recstore_room(s, L.stream, bytes, n_pick)) || (rc = reserve_roomy(ctx, s->app, a_cnt + 8 * ntb + 8))) return rc;
    uint8_t *at = (uint8_t *)s->arena.p + s->used;
    for (int32_t k = 0; k < n;) {
        if (!x_size[(size_t)k]) { k++; continue; }
        int32_t e = k;
        while (e < n && x_size[(size_t)e]) e++;
        const size_t run = (size_t)(rec_off[e] - rec_off[k]);
        HIPCHK(ctx, hipMemcpyAsync(at, recs + rec_off[k], run, hipMemcpyHostToDevice, L.stream));
        at += run;
        k = e;
    }
    HIPCHK(ctx, hipMemcpyAsync(s->app.p, x_size.data(), 4 * (size_t)n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync((uint8_t *)s->app.p + a_base, blk_base.data(), 8 * ntb, hipMemcpyHostToDevice, L.stream));
    rc = enqueue_recstore_append(s, L.stream, s->used, s->n_items, (uint32_t)n, (uint32_t)n_pick, (const uint32_t *)s->app.p, (const uint64_t *)((uint8_t *)s->app.p + a_base),
                                 (uint32_t *)((uint8_t *)s->app.p + a_cnt));
    const hipError_t e = hipStreamSynchronize(L.stream);  // (the vectors go out of scope)
    if (rc) return rc;
    HIPCHK(ctx, e);
    s->used += bytes;
    s->n_items += n_pick;
    return 0;
}

int fadehip_recstore_count(fadehip_recstore *s, int64_t *n_records, int64_t *n_bytes) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    if (!n_records || !n_bytes) return set_err(s->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    *n_records = (int64_t)s->n_items;
    *n_bytes = (int64_t)s->used;
    return 0;
}

// ---- the sorted main output's part of the store (bam_sortwin.hpp): budget, bucket table, window, reset
int fadehip_recstore_set_budget(fadehip_recstore *s, uint64_t bytes) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sorted || s->n_items) return set_err(ctx, FADEHIP_E_STATE, "recstore: set_budget takes an empty, unsorted store");
    if (const char *e = getenv("FADEHIP_RECSTORE_BUDGET")) {
        char *end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end == e || *end || !v) return set_err(ctx, FADEHIP_E_INVALID, "recstore: FADEHIP_RECSTORE_BUDGET=%s is not a positive number of bytes", e);
        bytes = v;
    }
    if (!bytes) {
        // Two fifths of what is free now, less a reserve.  Under a budget the arena stops at `budget` bytes and the item arrays
        // (20 bytes a record) at budget / 64 records.  A growth holds the old and the new buffer, and the old arena may be
        // nearly as large as the new one (the last step is clamped to the budget, not a doubling): 2 x budget for the arena
        // and 20/64 x budget for the item arrays beside it, 2.32 x budget in all.  When the item arrays grow instead it is
        // 1 + 2 x 20/64, and at the sort, when nothing grows any more, 1 + 20/64 + 37/64: both less.  2.5 x budget bounds every
        // moment (§3.8n).  The reserve is for what else a pass holds: the stream's two sets of call buffers and a drain's
        // staging and members; assumed, not measured.
        HIPCHK(ctx, hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
        const uint64_t reserve_b = std::min<uint64_t>((uint64_t)2 << 30, (uint64_t)free_b / 8);
        bytes = ((uint64_t)free_b - reserve_b) / 5 * 2;
        if (!bytes) return set_err(ctx, FADEHIP_E_NOMEM, "recstore: no device memory is free to derive a budget from");
    }
    s->budget = bytes;
    s->budget_set = true;
    return 0;
}

int fadehip_recstore_budget(fadehip_recstore *s, uint64_t *bytes) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    if (!bytes) return set_err(s->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    *bytes = s->budget_set ? s->budget : 0;
    return 0;
}

int fadehip_recstore_measure(fadehip_recstore *s, int32_t n_ref, const int64_t *ref_len) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n_ref < 0 || (n_ref > 0 && !ref_len)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    std::vector<uint32_t> len((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] < 0 || ref_len[r] > (int64_t)0xffffffffll) return set_err(ctx, FADEHIP_E_INVALID, "recstore: ref_len[%d] = %lld is no contig length", r, (long long)ref_len[r]);
        len[(size_t)r] = (uint32_t)ref_len[r];
    }
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sorted || s->n_items) return set_err(ctx, FADEHIP_E_STATE, "recstore: measure takes an empty, unsorted store");
    if (s->have_table) return set_err(ctx, FADEHIP_E_STATE, "recstore: measure has been called already (the table stays until the store is destroyed)");
    recstore::BucketLayout lay;
    if (!recstore::bucket_layout(len.data(), len.size(), lay)) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "recstore: the header's contigs make more than 2^32 buckets");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t tb = 16 * (size_t)lay.n_buckets, lb = 8 * len.size();
    if ((rc = recstore_alloc(ctx, s->table, tb)) || (rc = recstore_alloc(ctx, s->lay_dev, lb))) {
        release(s->table);
        return rc;
    }
    // (on the ctx's copy stream, as the contig names of a stream are: no null stream is brought up)
    if (hipMemsetAsync(s->table.p, 0, tb, ctx->copy_stream) != hipSuccess ||
        (n_ref && (hipMemcpyAsync(s->lay_dev.p, lay.first.data(), lb / 2, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess ||
                   hipMemcpyAsync((uint8_t *)s->lay_dev.p + lb / 2, lay.nb.data(), lb / 2, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess)) ||
        hipStreamSynchronize(ctx->copy_stream) != hipSuccess) {
        release(s->table);
        release(s->lay_dev);
        return set_err(ctx, FADEHIP_E_HIP, "recstore: setting up the bucket table failed");
    }
    s->lay = std::move(lay);
    s->have_table = true;
    s->measuring = true;
    s->over = false;
    return 0;
}

int fadehip_recstore_over(fadehip_recstore *s, int32_t *over) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    if (!over) return set_err(s->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    *over = s->over ? 1 : 0;
    return 0;
}

int fadehip_recstore_resets(fadehip_recstore *s, int64_t *n_reset) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    if (!n_reset) return set_err(s->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    *n_reset = (int64_t)s->n_reset;
    return 0;
}

int fadehip_recstore_histogram(fadehip_recstore *s, uint64_t *bytes, uint64_t *records, int64_t *n_buckets) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (!n_buckets || (!bytes) != (!records)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    if (!s->have_table) return set_err(ctx, FADEHIP_E_STATE, "recstore: histogram comes after fadehip_recstore_measure");
    const int64_t n = (int64_t)s->lay.n_buckets;
    if (!bytes) {
        *n_buckets = n;
        return 0;
    }
    if (*n_buckets < n) return set_err(ctx, FADEHIP_E_INVALID, "recstore: the table has %lld buckets, the arrays hold %lld", (long long)n, (long long)*n_buckets);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());  // the streams' kernels may be on any of the ctx's streams
    if (hipMemcpyAsync(bytes, s->table.p, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->copy_stream) != hipSuccess ||
        hipMemcpyAsync(records, (const uint8_t *)s->table.p + 8 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->copy_stream) != hipSuccess ||
        hipStreamSynchronize(ctx->copy_stream) != hipSuccess)
        return set_err(ctx, FADEHIP_E_HIP, "recstore: copying the bucket table failed");
    *n_buckets = n;
    return 0;
}

int fadehip_recstore_set_window(fadehip_recstore *s, uint64_t lo_key, uint64_t hi_key_inclusive) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (lo_key > hi_key_inclusive) return set_err(ctx, FADEHIP_E_INVALID, "recstore: the window's first key lies behind its last");
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sorted || s->n_items) return set_err(ctx, FADEHIP_E_STATE, "recstore: set_window takes an empty, unsorted store (fadehip_recstore_reset empties it)");
    s->win_lo = lo_key;
    s->win_hi = hi_key_inclusive;
    return 0;
}

int fadehip_recstore_reset(fadehip_recstore *s, uint64_t bytes, uint64_t records) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (records > RECSTORE_MAX_ITEMS)
        return set_err(ctx, FADEHIP_E_UNSUPPORTED, "recstore: more than %llu records (the sort numbers its items in 32 bits)", (unsigned long long)RECSTORE_MAX_ITEMS);
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->budget_set && recstore::sortwin_cost(bytes, records) > s->budget)
        return set_err(ctx, FADEHIP_E_NOMEM, "recstore: %llu bytes in %llu records would cost more than the budget of %llu bytes (the store holds every output record on the device)",
                       (unsigned long long)bytes, (unsigned long long)records, (unsigned long long)s->budget);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());  // whatever still appends, sorts or drains
    release(s->sort_arr);
    s->h_dst.clear();
    s->cursor = 0;
    s->sorted = false;
    s->used = 0;
    s->n_items = 0;
    s->over = false;
    s->measuring = false;
    s->n_reset = 0;
    // (nothing is kept, so nothing is copied: the old buffer goes before the new one comes)
    int rc;
    if ((uint64_t)s->arena.cap < bytes + 8) {
        release(s->arena);
        if ((rc = recstore_alloc(ctx, s->arena, (size_t)(bytes + 8)))) return rc;
    }
    if (s->item_cap < records) {
        s->item_cap = 0;
        for (DevBuf *b : {&s->key, &s->off, &s->size}) release(*b);
        if ((rc = recstore_alloc(ctx, s->key, 8 * (size_t)records)) || (rc = recstore_alloc(ctx, s->off, 8 * (size_t)records)) || (rc = recstore_alloc(ctx, s->size, 4 * (size_t)records))) {
            for (DevBuf *b : {&s->key, &s->off, &s->size}) release(*b);
            return rc;
        }
        s->item_cap = records;
    }
    return 0;
}

// the sort's arrays for n items, one behind the other from `base` (nullptr: only their size is wanted); key0, isrc and isize
// are the store's own item arrays
static size_t recstore_sort_layout(bam::ResortArgs &a, uint8_t *base, size_t n) {
    const size_t m = std::max<size_t>(n, 1), tiles = (m + bam::RS_TILE - 1) / bam::RS_TILE, ntb = (m + bam::TAG_BLOCK - 1) / bam::TAG_BLOCK;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        uint8_t *p = base + at;
        at += (bytes + 7) & ~(size_t)7;
        return p;
    };
    a.ctl = (bam::ResortCtl *)take(256);
    a.key1 = (uint64_t *)take(8 * m);
    a.msrc = (uint64_t *)take(8 * m);
    a.dst = (uint64_t *)take(8 * (m + 1));
    a.sblk = (uint64_t *)take(16 * ntb);
    a.idx0 = (uint32_t *)take(4 * m);
    a.idx1 = (uint32_t *)take(4 * m);
    a.msize = (uint32_t *)take(4 * m);
    a.hist = (uint32_t *)take(4 * 256 * tiles);
    a.hist_base = (uint32_t *)take(4 * 256 * tiles);
    return at;
}

int fadehip_recstore_sort(fadehip_recstore *s) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!L.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sorted) return set_err(ctx, FADEHIP_E_STATE, "recstore: the store has been sorted already");
    HIPCHK(ctx, hipDeviceSynchronize());  // the streams' appends may be on any of the ctx's streams
    const size_t n = (size_t)s->n_items;
    std::vector<uint64_t> dst(n + 1, 0);
    if (n) {
        bam::ResortArgs &a = s->ra;
        memset(&a, 0, sizeof a);
        int rc;
        if ((rc = recstore_alloc(ctx, s->sort_arr, recstore_sort_layout(a, nullptr, n)))) return rc;
        recstore_sort_layout(a, (uint8_t *)s->sort_arr.p, n);
        a.key0 = (uint64_t *)s->key.p;
        a.isrc = (uint64_t *)s->off.p;
        a.isize = (uint32_t *)s->size.p;
        const unsigned nb = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(bam::recstore_sort_begin_kernel, dim3(nb), dim3(256), 0, L.stream, a, (uint32_t)n);
        HIPCHK(ctx, hipGetLastError());
        if ((rc = enqueue_resort_sort(ctx, L.stream, a, n))) return rc;
        // (bam_resort.hpp's kernels behind the eighth pass: W is all ones, so the cut lets every record leave)
        hipLaunchKernelGGL(bam::bam_resort_cut_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, L.stream, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_resort_offsets_scan_kernel, dim3(1), dim3(1024), 0, L.stream, a, nb);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::bam_resort_offsets_kernel, dim3(nb), dim3(bam::TAG_BLOCK), 0, L.stream, a, nb);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(dst.data(), a.dst, 8 * (n + 1), hipMemcpyDeviceToHost, L.stream));
        HIPCHK(ctx, hipStreamSynchronize(L.stream));
        if (dst[n] != s->used) return set_err(ctx, FADEHIP_E_STATE, "internal: recstore: the sorted records take %llu bytes, the arena holds %llu", (unsigned long long)dst[n], (unsigned long long)s->used);
    }
    s->h_dst.swap(dst);
    s->cursor = 0;
    s->sorted = true;
    return 0;
}

int fadehip_recstore_drain(fadehip_recstore *s, int32_t flags, uint64_t max_payload, const uint8_t **out, size_t *out_bytes, int64_t *n_records, fadehip_index_call *idx) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    const bool raw = (flags & FADEHIP_RECSTORE_RAW) != 0, stored = (flags & FADEHIP_RECSTORE_STORED) != 0, index = (flags & FADEHIP_RECSTORE_INDEX) != 0;
    if (!out || !out_bytes || !n_records || (index && !idx)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    *out_bytes = 0;
    *n_records = 0;
    if (idx) memset(idx, 0, sizeof *idx);
    if (flags & ~(FADEHIP_RECSTORE_RAW | FADEHIP_RECSTORE_STORED | FADEHIP_RECSTORE_INDEX)) return set_err(ctx, FADEHIP_E_INVALID, "recstore: unknown drain flags");
    if (raw && (stored || index))
        return set_err(ctx, FADEHIP_E_INVALID, "recstore: FADEHIP_RECSTORE_RAW does not combine with %s (raw records have no members to store or to index)", index ? "FADEHIP_RECSTORE_INDEX" : "FADEHIP_RECSTORE_STORED");
    std::lock_guard<std::mutex> sl(s->mu);
    if (!s->sorted) return set_err(ctx, FADEHIP_E_STATE, "recstore: drain comes after fadehip_recstore_sort");
    const size_t n_all = (size_t)s->n_items, j0 = (size_t)s->cursor;
    if (j0 >= n_all) return 0;
    const size_t j1 = recstore::drain_cut(s->h_dst.data(), n_all, j0, std::min<uint64_t>(max_payload, RECSTORE_MAX_DRAIN));
    const size_t n = j1 - j0, bytes = (size_t)(s->h_dst[j1] - s->h_dst[j0]);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const int lane = 0;
    if ((rc = bgzf_lane_ready(ctx, lane))) return rc;  // (RAW too: the lane's stream is the drain's)
    hipStream_t q = ctx->bgzf[lane].stream;
    if ((rc = reserve_roomy(ctx, s->stage, bytes + 256)) || (rc = reserve_roomy(ctx, s->at, 8 * (n + 1)))) return rc;
    bam::RecGatherArgs g;
    g.arena = (const uint8_t *)s->arena.p;
    g.msrc = s->ra.msrc;
    g.dst = s->ra.dst;
    g.msize = s->ra.msize;
    g.j0 = (uint32_t)j0;
    g.n = (uint32_t)n;
    g.out = (uint8_t *)s->stage.p;
    g.at = (uint64_t *)s->at.p;
    hipLaunchKernelGGL(bam::recstore_gather_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, q, g);
    HIPCHK(ctx, hipGetLastError());
    if (raw) {
        if ((rc = reserve_pinned(ctx, s->h_out, bytes + 8))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s->h_out.p, s->stage.p, bytes, hipMemcpyDeviceToHost, q));
        HIPCHK(ctx, hipStreamSynchronize(q));
        *out = s->h_out.p;
        *out_bytes = bytes;
    } else {
        BgzfLane &l = ctx->bgzf[lane];
        if (stored) rc = bgzf_store_enqueue(ctx, lane, (const uint8_t *)s->stage.p, bytes, s->h_out);
        else rc = bgzf_enqueue(ctx, lane, (const uint8_t *)s->stage.p, bytes, bgzf_pick_geom(ctx), &s->h_out);
        if (rc) return rc;
        // the index stage behind the compressor's scan on the lane's stream, as the file path's (bam_enqueue_index); its
        // counts first, then arrays of exactly their size (fadehip_index_batch's two steps)
        bam::IndexArgs a;
        memset(&a, 0, sizeof a);
        bam::IndexCtl &c = s->ixc;
        memset(&c, 0, sizeof c);
        if (index) {
            if ((rc = reserve_roomy(ctx, s->ix_work, index_layout(a, nullptr, n))) || (rc = reserve(ctx, s->ix_ctl, 256))) return rc;
            index_layout(a, (uint8_t *)s->ix_work.p, n);
            a.ctl = (bam::IndexCtl *)s->ix_ctl.p;
            a.u = (const uint8_t *)s->stage.p;
            a.at = (const uint64_t *)s->at.p;
            a.n = (uint32_t)n;
            const BgzfGeometry geo = bgzf_lane_geometry(ctx, lane, stored);
            a.block = geo.block;
            a.member_off = geo.member_off;
            a.behind_ptr = geo.behind_ptr;
            a.member_stride = geo.member_stride;
            a.behind = geo.behind;
            if ((rc = enqueue_index_counts(ctx, q, a, s->ix_geo))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(&c, a.ctl, sizeof c, hipMemcpyDeviceToHost, q));
        }
        if (stored) {
            HIPCHK(ctx, hipEventSynchronize(l.done));
            l.state = 0;
            *out = l.h_out;
            *out_bytes = (size_t)*l.h_total;
        } else if ((rc = fadehip_bgzf_deflate_wait(ctx, lane, out, out_bytes))) return rc;
        if (index) {
            const auto fail = [&](int code) {
                *out = nullptr;  // (nothing of a drain that fails is handed out, and the cursor stays)
                *out_bytes = 0;
                return code;
            };
            if (hipStreamSynchronize(q) != hipSuccess) return fail(set_err(ctx, FADEHIP_E_HIP, "recstore: the index stage failed"));
            if ((rc = index_bad(ctx, c, (long long)j0, "recstore drain", s->ix_geo))) return fail(rc);
            if (c.n_linear >> 31) return fail(set_err(ctx, FADEHIP_E_UNSUPPORTED, "recstore drain: %llu linear index entries (at most 2^31)", (unsigned long long)c.n_linear));
            const size_t ix_bytes = index_out_layout(a, nullptr, n, (size_t)c.n_linear);
            if ((rc = reserve_roomy(ctx, s->ix_out, ix_bytes + 8))) return fail(rc);
            index_out_layout(a, (uint8_t *)s->ix_out.p, n, (size_t)c.n_linear);
            if ((rc = enqueue_index_write(ctx, q, a))) return fail(rc);
            s->h_ix.resize(ix_bytes + 8);
            if (hipMemcpyAsync(s->h_ix.data(), s->ix_out.p, ix_bytes, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
                return fail(set_err(ctx, FADEHIP_E_HIP, "recstore: copying the index entries failed"));
            bam::IndexArgs h;
            index_out_layout(h, s->h_ix.data(), n, (size_t)c.n_linear);
            idx->chunks = h.chunks;
            idx->linear = h.linear;
            idx->refs = h.refs;
            idx->n_chunks = (int64_t)c.n_chunks;
            idx->n_linear = (int64_t)c.n_linear;
            idx->n_refs = (int64_t)c.n_refs;
            idx->n_records = (int64_t)c.n;
            idx->first_key = c.first_key;
            idx->last_key = c.last_key;
        }
    }
    *n_records = (int64_t)n;
    s->cursor = j1;
    s->drained = true;
    return 0;
}

int fadehip_recstore_index_geometry(fadehip_recstore *s, int32_t min_shift, int32_t depth) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "recstore is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (!IndexGeometry::valid(min_shift, depth))
        return set_err(ctx, FADEHIP_E_INVALID, "recstore: CSI geometry (min_shift %d, depth %d): 4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32", (int)min_shift, (int)depth);
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->drained) return set_err(ctx, FADEHIP_E_STATE, "recstore: index_geometry comes before the first drain");
    s->ix_geo.min_shift = min_shift;
    s->ix_geo.depth = depth;
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
    release(st->names_first);
    release(st->ref_chrom);
    for (auto &S : st->set) {
        for (DevBuf *b : {&S.comp, &S.blocks, &S.status, &S.ticket, &S.u, &S.seg, &S.slots, &S.rec_off, &S.info, &S.sent_of, &S.art_of, &S.out_size, &S.blk32,
                          &S.blk64, &S.counts, &S.ex_size, &S.ex_blk, &S.rx_cnt, &S.sw_key,&S.ej_head, &S.ej_blk, &S.ej_grp, &S.ft_rec, &S.ft_side, &S.ft_ops_blk, &S.ft_ops_at, &S.ft_ops})
            release(*b);
        release(S.h_blocks);
        release(S.h_counts);
        release(S.h_ns);
        release(S.mt_hit);
        release(S.mt_fix);
        release(S.cm_fix);
        release(S.rp);
        release(S.rp_scratch);
        release(S.h_rp);
        for (DevBuf *b : {&S.rs_ctl, &S.rs_arr, &S.rs_stage, &S.rs_hold}) release(*b);  // (records still held, no last call: given back with the rest)
        release(S.h_rs);
        if (S.rs_meta) (void)hipEventDestroy(S.rs_meta);
        if (S.rs_moved) (void)hipEventDestroy(S.rs_moved);
    }
    for (auto &ob : st->outbuf) release(ob);
    for (auto &xb : st->xbuf) release(xb);
    for (auto &ib : st->ixbuf) release(ib);
    for (auto &rw : st->rbuf)
        for (auto &rb : rw) release(rb);
    for (auto &o : st->ring) {
        release(o.o);
        release(o.x);
        release(o.r[0]);
        release(o.r[1]);
        for (DevBuf *b : {&o.ix_at, &o.ix_work, &o.ix_ctl}) release(*b);
        if (o.iready) (void)hipEventDestroy(o.iready);
        if (o.xready) (void)hipEventDestroy(o.xready);
        if (o.rready) (void)hipEventDestroy(o.rready);
        if (o.ready) (void)hipEventDestroy(o.ready);
    }
    delete st;
}

// ---- the set of intervals (bam_intervals.hpp): fadehip_intervals_*
namespace {

constexpr uint64_t INTERVALS_DEFAULT_CAP = (uint64_t)1 << 20;
constexpr uint64_t INTERVALS_MAX = ((uint64_t)1 << 31) - 1;  // the sort numbers its items in 32 bits
constexpr int64_t INTERVALS_CALL = (int64_t)1 << 22;         // intervals (or queries) of one upload and launch

int intervals_alloc(fadehip_ctx *ctx, DevBuf &b, size_t bytes) {
    b.p = nullptr;
    b.cap = 0;
    const size_t want = (std::max<size_t>(bytes, 256) + 255) & ~(size_t)255;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return set_err(ctx, FADEHIP_E_NOMEM, "intervals: allocating %zu bytes on the device failed", want);
    }
    b.cap = want;
    return 0;
}

// a larger array with the first `keep` bytes of the old one (the caller holds s->mu and the lane's lock, and has waited for the lane's stream)
int intervals_regrow(fadehip_ctx *ctx, hipStream_t q, DevBuf &b, size_t keep, size_t want) {
    DevBuf nb;
    if (const int rc = intervals_alloc(ctx, nb, want)) return rc;
    if (keep && (hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)) {
        release(nb);
        return set_err(ctx, FADEHIP_E_HIP, "intervals: moving the items to a larger buffer failed");
    }
    release(b);
    b = nb;
    return 0;
}

int intervals_room(fadehip_intervals *s, hipStream_t q, uint64_t n_new) {
    fadehip_ctx *ctx = s->ctx;
    if (s->n + n_new > INTERVALS_MAX) return set_err(ctx, FADEHIP_E_UNSUPPORTED, "intervals: more than %llu intervals (the sort numbers its items in 32 bits)", (unsigned long long)INTERVALS_MAX);
    if (s->n + n_new <= s->cap) return 0;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(2 * s->cap, s->n + n_new), s->first_cap);
    int rc;
    if ((rc = intervals_regrow(ctx, q, s->key, 8 * (size_t)s->n, 8 * (size_t)cap)) || (rc = intervals_regrow(ctx, q, s->end32, 4 * (size_t)s->n, 4 * (size_t)cap)) ||
        (rc = intervals_regrow(ctx, q, s->idx, 4 * (size_t)s->n, 4 * (size_t)cap)))
        return rc;  // (an array that has grown already stays grown: it holds what it held)
    s->cap = cap;
    return 0;
}

int intervals_new(fadehip_ctx *ctx, fadehip_intervals **out) {
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fadehip_intervals *s = new (std::nothrow) fadehip_intervals;
    if (!s) return set_err(ctx, FADEHIP_E_NOMEM, "out of memory");
    s->ctx = ctx;
    s->first_cap = INTERVALS_DEFAULT_CAP;
    if (const char *e = getenv("FADEHIP_INTERVALS_CAP")) s->first_cap = (uint64_t)std::max<long long>(16, std::min<long long>(atoll(e), (long long)INTERVALS_MAX));
    *out = s;
    return 0;
}

// a name the set does not hold yet gets the next id (before seal; create's and the BED loader's)
int intervals_name(fadehip_intervals *s, const std::string &nm) {
    if (nm.empty()) return set_err(s->ctx, FADEHIP_E_INVALID, "intervals: chrom_names[%zu] is empty", s->names.size());
    if (!s->ids.emplace(nm, (int32_t)s->names.size()).second) return set_err(s->ctx, FADEHIP_E_INVALID, "intervals: chrom_names[%zu] names \"%s\" a second time", s->names.size(), nm.c_str());
    s->names.push_back(nm);
    return 0;
}

// add, under the lane's lock and the set's
int intervals_add_locked(fadehip_intervals *s, BatchLane &L, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end) {
    fadehip_ctx *ctx = s->ctx;
    int rc;
    if ((rc = intervals_room(s, L.stream, (uint64_t)n))) return rc;
    for (int64_t c0 = 0; c0 < n; c0 += INTERVALS_CALL) {
        const size_t m = (size_t)std::min<int64_t>(INTERVALS_CALL, n - c0);
        // stage: ctl | start [m] i64 | end [m] i64 | chrom [m] i32
        if ((rc = reserve_roomy(ctx, s->stage, 16 + 20 * m + 8))) return rc;
        uint8_t *sp = (uint8_t *)s->stage.p;
        bam::IvAddArgs a;
        a.ctl = (bam::IvCtl *)sp;
        a.start = (const int64_t *)(sp + 16);
        a.end = (const int64_t *)(sp + 16 + 8 * m);
        a.chrom = (const int32_t *)(sp + 16 + 16 * m);
        a.n = (uint32_t)m;
        a.item0 = (uint32_t)(s->n + (uint64_t)c0);
        a.n_chrom = (int32_t)s->names.size();
        a.key = (uint64_t *)s->key.p;
        a.end32 = (uint32_t *)s->end32.p;
        a.idx = (uint32_t *)s->idx.p;
        HIPCHK(ctx, hipMemsetAsync(sp, 0, 16, L.stream));
        HIPCHK(ctx, hipMemcpyAsync((void *)a.start, start + c0, 8 * m, hipMemcpyHostToDevice, L.stream));
        HIPCHK(ctx, hipMemcpyAsync((void *)a.end, end + c0, 8 * m, hipMemcpyHostToDevice, L.stream));
        HIPCHK(ctx, hipMemcpyAsync((void *)a.chrom, chrom + c0, 4 * m, hipMemcpyHostToDevice, L.stream));
        hipLaunchKernelGGL(bam::intervals_key_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, L.stream, a);
        HIPCHK(ctx, hipGetLastError());
        bam::IvCtl c;
        HIPCHK(ctx, hipMemcpyAsync(&c, a.ctl, sizeof c, hipMemcpyDeviceToHost, L.stream));
        HIPCHK(ctx, hipStreamSynchronize(L.stream));
        if (c.bad) {  // (the items written so far lie beyond s->n, which stays: nothing has been added)
            const long long k = (long long)c0 + (long long)(0xffffffffu - (uint32_t)(c.bad >> 8));
            if (chrom[k] < 0 || chrom[k] >= a.n_chrom)
                return set_err(ctx, FADEHIP_E_INVALID, "intervals: interval %lld: chrom %d is outside the set's %d contigs", k, chrom[k], a.n_chrom);
            return set_err(ctx, FADEHIP_E_INVALID, "intervals: interval %lld: start %lld, end %lld (0 <= start < end <= 2^31 - 1 is required)", k, (long long)start[k], (long long)end[k]);
        }
    }
    s->n += (uint64_t)n;
    return 0;
}

int intervals_seal_locked(fadehip_intervals *s, BatchLane &L) {
    fadehip_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n, n_chrom = s->names.size();
    hipStream_t q = L.stream;
    int rc;
    std::vector<uint32_t> noff(n_chrom + 1, 0);
    std::string nbytes;
    for (size_t c = 0; c < n_chrom; c++) {
        nbytes += s->names[c];
        noff[c + 1] = (uint32_t)nbytes.size();
    }
    if ((rc = intervals_alloc(ctx, s->start, 4 * n + 8)) || (rc = intervals_alloc(ctx, s->maxend, 8 * n + 8)) || (rc = intervals_alloc(ctx, s->chrom_first, 4 * (n_chrom + 1))) ||
        (rc = intervals_alloc(ctx, s->name_bytes, nbytes.size() + 8)) || (rc = intervals_alloc(ctx, s->name_off, 4 * noff.size())))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(s->name_off.p, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, q));
    if (!nbytes.empty()) HIPCHK(ctx, hipMemcpyAsync(s->name_bytes.p, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, q));
    HIPCHK(ctx, hipMemsetAsync(s->chrom_first.p, 0, 4 * (n_chrom + 1), q));
    DevBuf sort_arr, blk;
    bam::ResortCtl rc0;
    // (whichever way this function is left: nothing enqueued still reads what goes out of scope with it)
    struct Free { hipStream_t q; DevBuf &a, &b; ~Free() { (void)hipStreamSynchronize(q); release(a); release(b); } } free_them{q, sort_arr, blk};
    if (n) {
        bam::ResortArgs ra;
        memset(&ra, 0, sizeof ra);
        if ((rc = intervals_alloc(ctx, sort_arr, recstore_sort_layout(ra, nullptr, n)))) return rc;
        recstore_sort_layout(ra, (uint8_t *)sort_arr.p, n);
        ra.key0 = (uint64_t *)s->key.p;  // (the layout's msrc, dst, sblk and msize stay unused: the cut and the offsets are the records')
        memset(&rc0, 0, sizeof rc0);
        rc0.W = ~0ull;
        rc0.n_in = (uint32_t)n;
        HIPCHK(ctx, hipMemcpyAsync(ra.ctl, &rc0, sizeof rc0, hipMemcpyHostToDevice, q));
        HIPCHK(ctx, hipMemcpyAsync(ra.idx0, s->idx.p, 4 * n, hipMemcpyDeviceToDevice, q));
        if ((rc = enqueue_resort_sort(ctx, q, ra, n))) return rc;
        const unsigned nb = (unsigned)((n + 255) / 256);
        if ((rc = intervals_alloc(ctx, blk, 16 * (size_t)nb))) return rc;
        bam::IvSealArgs a;
        a.key = ra.key0;
        a.idx = ra.idx0;
        a.end32 = (const uint32_t *)s->end32.p;
        a.n = (uint32_t)n;
        a.n_chrom = (int32_t)n_chrom;
        a.start = (uint32_t *)s->start.p;
        a.maxend = (uint64_t *)s->maxend.p;
        a.blk_max = (uint64_t *)blk.p;
        a.blk_carry = a.blk_max + nb;
        a.chrom_first = (uint32_t *)s->chrom_first.p;
        hipLaunchKernelGGL(bam::intervals_gather_kernel, dim3(nb), dim3(256), 0, q, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::intervals_block_max_kernel, dim3(nb), dim3(256), 0, q, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::intervals_max_scan_kernel, dim3(1), dim3(1024), 0, q, a, (uint32_t)nb);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::intervals_max_apply_kernel, dim3(nb), dim3(256), 0, q, a);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(bam::intervals_chrom_first_kernel, dim3((unsigned)((n_chrom + 1 + 255) / 256)), dim3(256), 0, q, a);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(q));  // (the names' vectors go out of scope; the raw items are given back)
    for (DevBuf *b : {&s->key, &s->end32, &s->idx, &s->stage}) release(*b);
    s->cap = 0;
    s->sealed = true;
    return 0;
}

// the lane made ready for a call of the set's
int intervals_lane(fadehip_ctx *ctx, BatchLane &L) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!L.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    return 0;
}

}  // namespace

int fadehip_intervals_create(fadehip_ctx *ctx, int32_t n_chrom, const char *const *chrom_names, fadehip_intervals **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!out || n_chrom < 0 || (n_chrom > 0 && !chrom_names)) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    fadehip_intervals *s = nullptr;
    int rc;
    if ((rc = intervals_new(ctx, &s))) return rc;
    for (int32_t c = 0; c < n_chrom && !rc; c++) rc = chrom_names[c] ? intervals_name(s, chrom_names[c]) : set_err(ctx, FADEHIP_E_INVALID, "intervals: chrom_names[%d] is NULL", c);
    if (rc) {
        fadehip_intervals_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

int fadehip_intervals_add(fadehip_intervals *s, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "intervals is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || (n > 0 && (!chrom || !start || !end))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    int rc;
    if ((rc = intervals_lane(ctx, L))) return rc;
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sealed) return set_err(ctx, FADEHIP_E_STATE, "intervals: the set has been sealed, nothing can be added to it any more");
    if (n == 0) return 0;
    return intervals_add_locked(s, L, n, chrom, start, end);
}

int fadehip_intervals_seal(fadehip_intervals *s) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "intervals is NULL");
    fadehip_ctx *ctx = s->ctx;
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    int rc;
    if ((rc = intervals_lane(ctx, L))) return rc;
    std::lock_guard<std::mutex> sl(s->mu);
    if (s->sealed) return set_err(ctx, FADEHIP_E_STATE, "intervals: the set has been sealed already");
    return intervals_seal_locked(s, L);
}

int fadehip_intervals_count(fadehip_intervals *s, int64_t *n_intervals, int32_t *n_chrom) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "intervals is NULL");
    if (!n_intervals || !n_chrom) return set_err(s->ctx, FADEHIP_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> sl(s->mu);
    *n_intervals = (int64_t)s->n;
    *n_chrom = (int32_t)s->names.size();
    return 0;
}

int fadehip_intervals_overlap_batch(fadehip_intervals *s, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, uint8_t *hit) {
    if (!s) return set_err(nullptr, FADEHIP_E_INVALID, "intervals is NULL");
    fadehip_ctx *ctx = s->ctx;
    if (n < 0 || (n > 0 && (!chrom || !start || !end || !hit))) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    BatchLane &L = ctx->batch;
    std::lock_guard<std::mutex> lk(L.mu);
    int rc;
    if ((rc = intervals_lane(ctx, L))) return rc;
    std::lock_guard<std::mutex> sl(s->mu);
    if (!s->sealed) return set_err(ctx, FADEHIP_E_INVALID, "intervals: a query comes after fadehip_intervals_seal");
    for (int64_t c0 = 0; c0 < n; c0 += INTERVALS_CALL) {
        const size_t m = (size_t)std::min<int64_t>(INTERVALS_CALL, n - c0);
        // stage: start [m] i64 | end [m] i64 | chrom [m] i32 | hit [m] u8
        if ((rc = reserve_roomy(ctx, s->stage, 21 * m + 8))) return rc;
        uint8_t *sp = (uint8_t *)s->stage.p;
        bam::IvQueryArgs a;
        a.s = intervals_ref(s);
        a.start = (const int64_t *)sp;
        a.end = (const int64_t *)(sp + 8 * m);
        a.chrom = (const int32_t *)(sp + 16 * m);
        a.hit = sp + 20 * m;
        a.n = (uint32_t)m;
        HIPCHK(ctx, hipMemcpyAsync((void *)a.start, start + c0, 8 * m, hipMemcpyHostToDevice, L.stream));
        HIPCHK(ctx, hipMemcpyAsync((void *)a.end, end + c0, 8 * m, hipMemcpyHostToDevice, L.stream));
        HIPCHK(ctx, hipMemcpyAsync((void *)a.chrom, chrom + c0, 4 * m, hipMemcpyHostToDevice, L.stream));
        hipLaunchKernelGGL(bam::intervals_overlap_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, L.stream, a);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(hit + c0, a.hit, m, hipMemcpyDeviceToHost, L.stream));
        HIPCHK(ctx, hipStreamSynchronize(L.stream));
    }
    return 0;
}

int fadehip_intervals_load_bed(fadehip_ctx *ctx, const char *path, fadehip_intervals **out) {
    if (!ctx) return set_err(nullptr, FADEHIP_E_INVALID, "ctx is NULL");
    if (!path || !out) return set_err(ctx, FADEHIP_E_INVALID, "NULL argument");
    *out = nullptr;
    const std::string no = bed::path_refusal(path);
    if (!no.empty()) return set_err(ctx, FADEHIP_E_INVALID, "bed: %s", no.c_str());
    FILE *f = fopen(path, "rb");
    if (!f) return set_err(ctx, FADEHIP_E_INVALID, "bed: cannot open %s: %s", path, strerror(errno));
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    fadehip_intervals *s = nullptr;
    int rc;
    if ((rc = intervals_new(ctx, &s))) return rc;
    BatchLane &L = ctx->batch;
    bed::Parser *self = nullptr;
    // a piece: the names it brought first (ids in order of first appearance, as the parser numbers them), then its intervals
    bed::Parser parser([&](const int32_t *chrom, const int64_t *start, const int64_t *end, size_t n, std::string &why) {
        std::lock_guard<std::mutex> lk(L.mu);
        int r = intervals_lane(ctx, L);
        std::lock_guard<std::mutex> sl(s->mu);
        for (size_t c = s->names.size(); !r && c < self->names().size(); c++) r = intervals_name(s, self->names()[c]);
        if (!r) r = intervals_add_locked(s, L, (int64_t)n, chrom, start, end);
        if (r) {
            rc = r;
            why = fadehip_last_error(ctx);
        }
        return r == 0;
    });
    self = &parser;
    std::vector<char> buf((size_t)1 << 20);
    bool ok = true;
    size_t got;
    while (ok && (got = fread(buf.data(), 1, buf.size(), f)) > 0) ok = parser.feed(buf.data(), got);
    if (ok && ferror(f)) {
        fadehip_intervals_destroy(s);
        return set_err(ctx, FADEHIP_E_INVALID, "bed: read error on %s", path);
    }
    ok = ok && parser.finish();
    if (!ok) {
        const std::string why = parser.error();
        fadehip_intervals_destroy(s);
        return rc ? set_err(ctx, rc, "bed: %s: %s", path, why.c_str()) : set_err(ctx, FADEHIP_E_INVALID, "bed: %s: %s", path, why.c_str());
    }
    {  // (a contig may be named by the last piece alone)
        std::lock_guard<std::mutex> sl(s->mu);
        for (size_t c = s->names.size(); !rc && c < parser.names().size(); c++) rc = intervals_name(s, parser.names()[c]);
    }
    if (!rc) rc = fadehip_intervals_seal(s);
    if (rc) {
        fadehip_intervals_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

void fadehip_intervals_destroy(fadehip_intervals *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    for (DevBuf *b : {&s->key, &s->end32, &s->idx, &s->start, &s->maxend, &s->chrom_first, &s->name_bytes, &s->name_off, &s->stage}) release(*b);
    delete s;
}

}  // extern "C"
