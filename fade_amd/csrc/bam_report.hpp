// bam_report.hpp — `fade stats` (stats.d:75-186) and `fade stats-clip` (noclip.d:17-73) over records that were annotated
// EARLIER: the rows of the two reports as device work (fadehip_report_batch).  The tags are read back where they lie
// (read_tags / am_side of bam_device.hpp, the functions of fadehip_tags_batch), the inverted-repeat search is sw_stats_kernel
// as it is, reading the as / ar pieces in place, and the text of a row — numbers included (fmt_g6.hpp) — is written by the
// sixteen lanes of its side.  The kernels here are of their own; a call without a report launches none of them.
//
// A row belongs to a SLOT: slot 2 i is the left side of record i, slot 2 i + 1 its right side, for each report.  A slot
// without a row has kind 0 and takes no bytes, so that the rows' offsets [2 n + 1] say which record and side a row is of.
//
//   report_stage_kernel   thread per record: which slots have rows, what the rules call a failure, a
//                         descriptor per row, the stats sides counted by the five row classes of fadehip_sw_stats_batch
//   report_bucket_kernel  thread per slot: the stats sides' StatsWork, class behind class
//   sw_stats_kernel<R>    (sw_stats.hpp, unchanged) one launch per class that has sides
//   report_repeats_kernel (bam_intervals.hpp; only with a set of intervals attached) thread per slot: the two repeat-overlap bits
//   report_size_kernel    sixteen lanes per slot: the sums of the qualities and ab bytes, the row's exact bytes
//   report_scan_kernel    one block: the rows' offsets in slot order, their total (scan_block_sums)
//   report_write_kernel   sixteen lanes per slot: the row
#pragma once
#include "bam_device.hpp"
#include "sw_stats.hpp"
#define FMT_G6_HD __host__ __device__
#include "fmt_g6.hpp"

namespace fadehip {
namespace bam {

enum : uint32_t { RP_STATS = 1, RP_CLIP = 2 };
// why a call fails (RepCtl::bad); RP_BAD_LONG is FADEHIP_E_UNSUPPORTED, the others FADEHIP_E_INVALID
enum : uint32_t {
    RP_BAD_AUX = 1,       // the aux area is not whole fields
    RP_BAD_SIDE = 2,      // a needed am side is not name,pos,cigar, or its position is outside int32
    RP_BAD_ART_TAGS = 3,  // as / ar / ab absent or not of type Z
    RP_BAD_PIECE = 4,     // as / ar has no piece for a needed right side, or the as piece is empty
    RP_BAD_AB = 5,        // ab is shorter than the as piece
    RP_BAD_NO_S = 6,      // the record's CIGAR has no S op
    RP_BAD_TID = 7,       // refID outside the header
    RP_BAD_LONG = 8,      // a piece longer than FADEHIP_MAX_LONG_QUERY
    RP_BAD_CLIP_EMPTY = 9,  // stats-clip: a clip, and l_seq == 0
    RP_BAD_CLIP_LONG = 10,  // stats-clip: a clip longer than l_seq
};

struct RepCtl {
    unsigned long long bad;       // 0: none; else ((0xffffffff - record) << 8) | RP_BAD_*: the first record that fails the call
    unsigned long long total[2];  // bytes of the stats rows, of the clip rows (report_scan_kernel)
    uint32_t cls[5];              // stats sides per row class (<= 64, <= 128, <= 256, <= 512 query rows, beyond)
    uint32_t cursor[5];           // report_bucket_kernel's, per class
    uint32_t long_max_lr;         // the longest reference of the last class (its scratch rows)
    uint32_t rows[2];             // rows of the stats report, of the clip report
    uint32_t pad;
};
static_assert(sizeof(RepCtl) == 80, "RepCtl layout");

// one stats row; offsets are relative to the record
struct StatsRow {
    int64_t art0, art1, aln_end;
    uint64_t qsum;                // sum of the record's qualities (report_size_kernel)
    uint32_t am_at, am_name_len;  // the am side: its contig name ...
    uint32_t am_cig_at, am_cig_len;  // ... and its CIGAR text
    uint32_t as_at, as_len, ar_at, ar_len;  // the side's pieces of as and ar
    uint32_t ab_at;               // the side's slice of ab (as_len bytes)
    uint32_t bsum;                // sum of that slice (report_size_kernel)
    int32_t aln_start;
    uint32_t rs;
};
struct ClipRow {
    uint64_t qsum, ssum;  // sums of the record's qualities, of the clip's (report_size_kernel)
    uint32_t len;         // the clip's bases
    uint32_t art;         // rs names this side an artifact
};

struct RepArgs {
    const uint8_t *base;
    const uint32_t *off32;   // the records' offsets from base: one of the two
    const uint64_t *off64;
    uint32_t n, which;       // RP_*
    RefNames names;
    RepCtl *ctl;
    uint8_t *kind[2];        // [2n] per report (stats, clip) and slot: 1 a row, 0 none
    StatsRow *srow;          // [2n]
    ClipRow *crow;           // [2n]
    StatsWork *work;         // [2n] class behind class
    fadehip_sw_stats_result *res;  // [2n] by slot
    uint64_t *size[2];       // [2n] bytes of a slot's row
    uint64_t *row_off[2];    // [2n + 1]
    uint8_t *out[2];
};

__device__ __forceinline__ const uint8_t *rep_rec(const RepArgs &a, uint32_t i) {
    return a.base + (a.off64 ? a.off64[i] : (uint64_t)a.off32[i]);
}
__device__ __forceinline__ int rep_class(uint32_t lq) { return lq <= 64u ? 0 : lq <= 128u ? 1 : lq <= 256u ? 2 : lq <= 512u ? 3 : 4; }

// the first as, ar and ab fields (as bam_aux_get finds them) of a record whose aux area is whole fields
struct ArtTags {
    uint32_t at[3], len[3];  // the strings without their NUL, relative to the record
    bool ok;                 // all three are there and of type Z
};
__device__ __forceinline__ ArtTags read_art_tags(const RecHdr &r) {
    ArtTags g;
    bool seen[3] = {false, false, false}, z[3] = {false, false, false};
    for (int k = 0; k < 3; k++) g.at[k] = g.len[k] = 0u;
    uint32_t q = r.aux_off;
    while (q + 3u <= r.end) {
        const uint32_t fs = aux_field_size(r.p, q + 2u, r.end);
        if (!fs) break;
        const uint8_t a0 = r.p[q], a1 = r.p[q + 1];
        const int k = a0 != 'a' ? -1 : a1 == 's' ? 0 : a1 == 'r' ? 1 : a1 == 'b' ? 2 : -1;
        if (k >= 0 && !seen[k]) {
            seen[k] = true;
            if (r.p[q + 2] == 'Z') {
                z[k] = true;
                g.at[k] = q + 3u;
                g.len[k] = fs - 2u;
            }
        }
        q += 2u + fs;
    }
    g.ok = z[0] && z[1] && z[2];
    return g;
}
// piece `side` (0 or 1) of s[0 .. n) cut at ';' (what split(';')[side] gives); false: there is no such piece
__device__ __forceinline__ bool semi_piece(const uint8_t *s, uint32_t n, uint32_t side, uint32_t *at, uint32_t *len) {
    uint32_t b = 0;
    if (side) {
        while (b < n && s[b] != ';') b++;
        if (b >= n) return false;
        b++;
    }
    uint32_t e = b;
    while (e < n && s[e] != ';') e++;
    *at = b;
    *len = e - b;
    return true;
}

__global__ __launch_bounds__(TAG_BLOCK) void report_stage_kernel(RepArgs a) {
    const uint32_t i = blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const RecHdr r = rec_header(rep_rec(a, i));
    const TagsRead t = read_tags(r);
    uint32_t bad = t.whole ? 0u : RP_BAD_AUX;
    const bool has = (t.have & 1) != 0;
    const uint32_t rs = has ? t.rs : 0u;
    uint8_t kind[4] = {0, 0, 0, 0};
    if ((a.which & RP_STATS) && (rs & 6u) && (t.have & 2)) {
        const ArtTags g = read_art_tags(r);
        if (!g.ok) bad = max(bad, (uint32_t)RP_BAD_ART_TAGS);
        int64_t al = 0;
        int64_t first_s = -1, last_s = -1;
        for (uint32_t k = 0; k < r.ncig; k++) {
            const uint32_t op = ld32(r.p + r.cig_off + 4u * k);
            if (FADEHIP_OP_CONSUMES_REF(op & 15u)) al += op >> 4;
            if ((op & 15u) == 4u) {
                if (first_s < 0) first_s = op >> 4;
                last_s = op >> 4;
            }
        }
        if (first_s < 0) bad = max(bad, (uint32_t)RP_BAD_NO_S);
        if (r.tid < 0 || r.tid >= a.names.n_ref) bad = max(bad, (uint32_t)RP_BAD_TID);
        uint32_t semi = 0;
        while (semi < t.am_len && r.p[t.am_off + semi] != ';') semi++;
        const uint32_t right = min(semi + 1u, t.am_len);  // (without a ';' the right side is empty)
        const uint32_t s_at[2] = {t.am_off, t.am_off + right}, s_len[2] = {semi, t.am_len - right};
        for (uint32_t side = 0; side < 2u && g.ok; side++) {
            if (!(rs & (2u << side))) continue;
            const AmSide s = am_side(r, a.names, s_at[side], s_len[side]);
            if (!s.ok || s.pos < -2147483648ll || s.pos > 2147483647ll) { bad = max(bad, (uint32_t)RP_BAD_SIDE); continue; }
            StatsRow w;
            uint32_t p_at, p_len;
            if (!semi_piece(r.p + g.at[0], g.len[0], side, &p_at, &p_len) || !p_len) { bad = max(bad, (uint32_t)RP_BAD_PIECE); continue; }
            w.as_at = g.at[0] + p_at;
            w.as_len = p_len;
            if (!semi_piece(r.p + g.at[1], g.len[1], side, &p_at, &w.ar_len)) { bad = max(bad, (uint32_t)RP_BAD_PIECE); continue; }
            w.ar_at = g.at[1] + p_at;
            if (w.as_len > (uint32_t)FADEHIP_MAX_LONG_QUERY || w.ar_len > (uint32_t)FADEHIP_MAX_LONG_QUERY) { bad = max(bad, (uint32_t)RP_BAD_LONG); continue; }
            if (g.len[2] < w.as_len) { bad = max(bad, (uint32_t)RP_BAD_AB); continue; }
            w.ab_at = side ? g.at[2] + g.len[2] - w.as_len : g.at[2];
            uint32_t c1 = 0;
            while (r.p[s_at[side] + c1] != ',') c1++;  // (the side is well-formed: it has its commas)
            w.am_at = s_at[side];
            w.am_name_len = c1;
            w.am_cig_at = s.cig_at;
            w.am_cig_len = s_at[side] + s_len[side] - s.cig_at;
            uint32_t nops;
            uint64_t ref;
            am_cigar(r.p + w.am_cig_at, w.am_cig_len, &nops, &ref);
            w.aln_start = (int32_t)s.pos;
            w.aln_end = s.pos + (int64_t)ref;
            w.art0 = side ? (int64_t)r.pos + al : (int64_t)r.pos - first_s;
            w.art1 = side ? (int64_t)r.pos + al + last_s : (int64_t)r.pos;
            w.qsum = 0;
            w.bsum = 0;
            w.rs = rs;
            if (bad) continue;
            a.srow[2 * (size_t)i + side] = w;
            kind[side] = 1;
        }
    }
    if ((a.which & RP_CLIP) && (rs & 1u)) {  // parse_clips (util.d:37-62): `first` stays set while the ops are soft clips
        uint32_t clips[2] = {0u, 0u};
        bool is[2] = {false, false}, first = true;
        for (uint32_t k = 0; k < r.ncig; k++) {
            const uint32_t op = ld32(r.p + r.cig_off + 4u * k);
            if ((op & 15u) == 5u) continue;
            const bool sc = (op & 15u) == 4u;
            if (first && !sc) first = false;
            else if (sc) { is[first ? 0 : 1] = true; clips[first ? 0 : 1] = op >> 4; }
        }
        for (uint32_t side = 0; side < 2u; side++) {
            if (!is[side]) continue;
            if (r.lseq <= 0) { bad = max(bad, (uint32_t)RP_BAD_CLIP_EMPTY); continue; }
            if (clips[side] > (uint32_t)r.lseq) { bad = max(bad, (uint32_t)RP_BAD_CLIP_LONG); continue; }
            ClipRow c;
            c.qsum = c.ssum = 0;
            c.len = clips[side];
            c.art = (rs & (2u << side)) ? 1u : 0u;
            a.crow[2 * (size_t)i + side] = c;
            kind[2 + side] = 1;
        }
    }
    if (bad) {
        atomicMax(&a.ctl->bad, ((unsigned long long)(0xffffffffu - i) << 8) | bad);
        kind[0] = kind[1] = kind[2] = kind[3] = 0;
    }
    if (kind[0] + kind[1]) atomicAdd(&a.ctl->rows[0], (uint32_t)(kind[0] + kind[1]));
    if (kind[2] + kind[3]) atomicAdd(&a.ctl->rows[1], (uint32_t)(kind[2] + kind[3]));
    for (uint32_t side = 0; side < 2u; side++) {
        if (a.which & RP_STATS) a.kind[0][2 * (size_t)i + side] = kind[side];
        if (a.which & RP_CLIP) a.kind[1][2 * (size_t)i + side] = kind[2 + side];
        if (kind[side]) {
            const StatsRow &w = a.srow[2 * (size_t)i + side];
            const uint32_t lq = (3u * w.as_len + 2u) / 4u;  // round(0.75 * length): half away from zero (stats.d:123,164)
            const int c = rep_class(lq);
            atomicAdd(&a.ctl->cls[c], 1u);
            if (c == 4) atomicMax(&a.ctl->long_max_lr, w.ar_len);
        }
    }
}

// thread per slot: a stats side's pair, its strings where the tags lie in the records, among the pairs of its class
__global__ __launch_bounds__(TAG_BLOCK) void report_bucket_kernel(RepArgs a) {
    const size_t s = (size_t)blockIdx.x * TAG_BLOCK + threadIdx.x;
    if (s >= 2 * (size_t)a.n || !a.kind[0][s]) return;
    const StatsRow &w = a.srow[s];
    const uint64_t rec = (uint64_t)(rep_rec(a, (uint32_t)(s >> 1)) - a.base);
    const uint32_t lq = (3u * w.as_len + 2u) / 4u;
    const int c = rep_class(lq);
    uint32_t at = atomicAdd(&a.ctl->cursor[c], 1u);
    for (int k = 0; k < c; k++) at += a.ctl->cls[k];
    StatsWork p;
    p.q_base = rec + w.as_at;
    p.r_base = rec + w.ar_at;
    p.lq = (int32_t)lq;
    p.lr = (int32_t)w.ar_len;
    p.idx = (int32_t)s;
    p.pad = 0;
    a.work[at] = p;
}

// A row's bytes, by the sixteen lanes of its slot: every lane counts, lane 0 writes the short fields, all of them the long ones.
struct RowSink {
    uint8_t *d;  // nullptr: count only
    uint32_t n, sl;
    __device__ __forceinline__ void put(uint8_t c) {
        if (d && sl == 0u) d[n] = c;
        n++;
    }
    __device__ __forceinline__ void dec(int64_t v) {
        Sink s;
        s.d = (d && sl == 0u) ? d : nullptr;
        s.n = n;
        s.dec(v);
        n = s.n;
    }
    __device__ __forceinline__ void text(const char *b, uint32_t len) {
        if (d && sl == 0u)
            for (uint32_t k = 0; k < len; k++) d[n + k] = (uint8_t)b[k];
        n += len;
    }
    __device__ __forceinline__ void ratio(uint64_t num, uint64_t den) {
        char b[FMT_G6_MAX];
        text(b, fmt_g6_ratio(num, den, b));
    }
    __device__ __forceinline__ void bytes(const uint8_t *src, uint32_t len) {
        if (d)
            for (uint32_t k = sl; k < len; k += 16u) d[n + k] = src[k];
        n += len;
    }
};

__device__ __forceinline__ uint64_t sum16(uint64_t v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((long long)v, m, 64);
    return v;
}

// RPM: the row ends with the two repeat-overlap columns (bam_intervals.hpp), bit 0 and bit 1 of `rpm`; <false> is the row as it was
template <bool RPM>
__device__ __forceinline__ void stats_row(const RepArgs &a, const RecHdr &r, const StatsRow &w, const fadehip_sw_stats_result &res, RowSink &s, uint32_t rpm) {
    s.bytes(r.p + 36u, r.lname - 1u);
    s.put('\t');
    s.bytes(a.names.bytes + a.names.off[r.tid], a.names.off[r.tid + 1] - a.names.off[r.tid]);
    s.put('\t');
    s.dec(r.pos);
    s.put('\t');
    for (uint32_t k = 0; k < r.ncig; k++) {
        const uint32_t op = ld32(r.p + r.cig_off + 4u * k);
        s.dec(op >> 4);
        s.put((uint8_t)"MIDNSHP=XB"[min(op & 15u, 9u)]);
    }
    s.put('\t');
    s.dec(w.art0);
    s.put('\t');
    s.dec(w.art1);
    s.put('\t');
    s.bytes(r.p + w.am_at, w.am_name_len);
    s.put('\t');
    s.dec(w.aln_start);
    s.put('\t');
    s.dec(w.aln_end);
    s.put('\t');
    s.bytes(r.p + w.am_cig_at, w.am_cig_len);
    s.put('\t');
    s.bytes(r.p + w.as_at, w.as_len);
    s.put('\t');
    s.bytes(r.p + w.ar_at, w.ar_len);
    s.put('\t');
    const uint32_t ir = min((uint32_t)res.end_query + 1u, w.as_len);  // the predicted repeat: the stem loop up to the alignment's end
    s.bytes(r.p + w.as_at, ir);
    s.put('\t');
    s.ratio((uint64_t)res.matches, (uint64_t)res.length);
    s.put('\t');
    s.ratio(w.qsum, (uint64_t)(r.lseq > 0 ? r.lseq : 0));
    s.put('\t');
    s.ratio(w.bsum, w.as_len);
    s.put('\t');
    s.bytes(r.p + w.ab_at, w.as_len);
    s.put('\t');
    s.bytes(r.p + w.ab_at, ir);
    s.put('\t');
    for (int b = 7; b >= 0; b--) s.put((uint8_t)('0' + ((w.rs >> b) & 1u)));
    s.put('\t');
    s.dec(w.rs);
    s.put('\t');
    s.put((r.flag & 16u) ? '+' : '-');
    if constexpr (RPM) {
        s.put('\t');
        s.put((uint8_t)('0' + (rpm & 1u)));
        s.put('\t');
        s.put((uint8_t)('0' + ((rpm >> 1) & 1u)));
    }
    s.put('\n');
}

__device__ __forceinline__ void clip_row(const RecHdr &r, const ClipRow &c, uint32_t side, RowSink &s) {
    const uint32_t b0 = side ? (uint32_t)r.lseq - c.len : 0u;
    s.bytes(r.p + 36u, r.lname - 1u);
    s.put('\t');
    if (s.d)  // qualities + 33 in byte arithmetic (0xff wraps to a space), the bytes as they come
        for (uint32_t k = s.sl; k < c.len; k += 16u) s.d[s.n + k] = (uint8_t)(r.p[r.qual_off + b0 + k] + 33u);
    s.n += c.len;
    s.put('\t');
    if (s.d)
        for (uint32_t k = s.sl; k < c.len; k += 16u) {
            const uint32_t j = b0 + k;
            s.d[s.n + k] = (uint8_t)"=ACMGRSVTWYHKDBN"[(r.p[r.seq_off + (j >> 1)] >> ((~j & 1u) << 2)) & 15u];
        }
    s.n += c.len;
    s.put('\t');
    s.ratio(c.ssum, c.len);
    s.put('\t');
    s.ratio(c.qsum, (uint64_t)r.lseq);
    s.put('\t');
    if (c.art) s.text("true", 4);
    else s.text("false", 5);
    s.put('\n');
}

// sixteen lanes per slot: the qualities and the ab bytes summed where they are read, then the row counted.  <true>: a stats
// row carries the two columns of rpm [2n] (report_repeats_kernel's); <false> never looks at rpm
template <bool RPM>
__global__ __launch_bounds__(256) void report_size_kernel(RepArgs a, uint32_t w, const uint8_t *rpm) {
    const size_t ns = 2 * (size_t)a.n, s = (size_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    const uint32_t sl = threadIdx.x & 15u;
    const bool on = s < ns && a.kind[w][s];
    RecHdr r;
    uint64_t qs = 0, ps = 0;
    if (on) {
        r = rec_header(rep_rec(a, (uint32_t)(s >> 1)));
        const uint32_t lq = r.lseq > 0 ? (uint32_t)r.lseq : 0u;
        for (uint32_t k = sl; k < lq; k += 16u) qs += r.p[r.qual_off + k];
        if (w == 0u) {
            const StatsRow &row = a.srow[s];
            for (uint32_t k = sl; k < row.as_len; k += 16u) ps += r.p[row.ab_at + k];
        } else {
            const ClipRow &row = a.crow[s];
            const uint32_t b0 = (s & 1u) ? lq - row.len : 0u;
            for (uint32_t k = sl; k < row.len; k += 16u) ps += r.p[r.qual_off + b0 + k];
        }
    }
    qs = sum16(qs);
    ps = sum16(ps);
    if (!on) {
        if (s < ns && sl == 0u) a.size[w][s] = 0;
        return;
    }
    RowSink sink;
    sink.d = nullptr;
    sink.n = 0;
    sink.sl = sl;
    if (w == 0u) {
        StatsRow &row = a.srow[s];
        if (sl == 0u) {
            row.qsum = qs;
            row.bsum = (uint32_t)ps;
        }
        StatsRow v = row;
        v.qsum = qs;
        v.bsum = (uint32_t)ps;
        stats_row<RPM>(a, r, v, a.res[s], sink, RPM ? (uint32_t)rpm[s] : 0u);
    } else {
        ClipRow &row = a.crow[s];
        if (sl == 0u) {
            row.qsum = qs;
            row.ssum = ps;
        }
        ClipRow v = row;
        v.qsum = qs;
        v.ssum = ps;
        clip_row(r, v, (uint32_t)(s & 1u), sink);
    }
    if (sl == 0u) a.size[w][s] = sink.n;
}

// one block: where every slot's row starts, and the report's bytes
__global__ __launch_bounds__(1024) void report_scan_kernel(RepArgs a, uint32_t w) {
    const size_t ns = 2 * (size_t)a.n;
    uint64_t *off = a.row_off[w];
    scan_block_sums<uint64_t, false>(a.size[w], off, (uint32_t)ns, (uint64_t *)&a.ctl->total[w]);
    if (threadIdx.x == 0) off[ns] = a.ctl->total[w];
}

template <bool RPM>
__global__ __launch_bounds__(256) void report_write_kernel(RepArgs a, uint32_t w, const uint8_t *rpm) {
    const size_t ns = 2 * (size_t)a.n, s = (size_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    if (s >= ns || !a.kind[w][s]) return;
    const RecHdr r = rec_header(rep_rec(a, (uint32_t)(s >> 1)));
    RowSink sink;
    sink.d = a.out[w] + a.row_off[w][s];
    sink.n = 0;
    sink.sl = threadIdx.x & 15u;
    if (w == 0u) stats_row<RPM>(a, r, a.srow[s], a.res[s], sink, RPM ? (uint32_t)rpm[s] : 0u);
    else clip_row(r, a.crow[s], (uint32_t)(s & 1u), sink);
}

}  // namespace bam
}  // namespace fadehip
