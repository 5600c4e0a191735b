// fadehip_bgzf.hip — BGZF on the device: host side of bgzf_inflate.hpp and bgzf_deflate.hpp.
// The scan of member headers and the inflate launch (used here, by the file path and by the FASTA upload), the compressor
// lanes with their one-time kernel setup, geometry choice and launches, the stored-member launch of the file path, and
// fadehip_bgzf_deflate_submit / _wait and fadehip_bgzf_inflate.
#include "fadehip_host.hpp"
#include "bgzf_deflate.hpp"
#include "bgzf_inflate.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fadehip;
using namespace fadehip::host;

namespace {

// The same choice for bytes the host can look at (fadehip_bgzf_deflate_submit): the share of bytes equal to their
// predecessor over 64 windows of 4 KB.  Packed bases and uniform qualities: a few per cent; qualities in runs: a third.
int bgzf_pick_geom_host(const fadehip_ctx *ctx, const uint8_t *p, size_t n) {
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
size_t bgzf_block_bytes(int geom) { return geom == 32 ? (size_t)bgzf32::BLOCK : (size_t)bgzf64::BLOCK; }

}  // namespace

namespace fadehip::host {

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

// ------------------------------------------------------------------------------- BGZF compression
// the compressor's launches for n_bytes at d_src (device memory with 64 readable bytes behind the end) on the lane's stream
int bgzf_lane_ready(fadehip_ctx *ctx, int lane, bool one_stream) {
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
int bgzf_pick_geom(const fadehip_ctx *ctx) {
    if (ctx->bgzf_geom_fixed) return ctx->bgzf_geom_fixed;
    return ctx->bgzf_last_ratio > 0.45 ? 32 : 64;
}
// (host_out: pinned memory the members are packed into — the lane's own buffer when NULL.  A member is at most its block's
// bytes + 5 (stored) + 26 of BGZF framing: the buffer is sized for that, the kernel writes through PCIe, and nothing but
// the 8-byte total has to be copied afterwards.)
size_t bgzf_out_cap(size_t n_bytes, int geom) {
    const size_t block = bgzf_block_bytes(geom);
    return n_bytes + ((n_bytes + block - 1) / block) * 32 + 64;
}
int bgzf_enqueue(fadehip_ctx *ctx, int lane, const uint8_t *d_src, size_t n_bytes, int geom, PinBuf *host_out) {
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

// Uncompressed BGZF (the file path's FADEHIP_BAM_STORED) on a lane made ready: the members' sizes are known here; the
// kernel stores them straight into the pinned buffer, which bgzf_store_cap sizes
size_t bgzf_store_cap(size_t n_bytes) { return (n_bytes / bgzf::STORE_BLOCK + 2) * bgzf::STORE_MEMBER; }
int bgzf_store_enqueue(fadehip_ctx *ctx, int lane, const uint8_t *d_src, size_t n_bytes, PinBuf &ob) {
    BgzfLane &l = ctx->bgzf[lane];
    int rc;
    const uint32_t nb = (uint32_t)((n_bytes + bgzf::STORE_BLOCK - 1) / bgzf::STORE_BLOCK);
    const size_t total = n_bytes + (size_t)nb * (bgzf::STORE_MEMBER - bgzf::STORE_BLOCK);
    if ((rc = reserve_pinned(ctx, ob, (size_t)nb * bgzf::STORE_MEMBER))) return rc;
    hipLaunchKernelGGL(bgzf::bgzf_store_kernel, dim3(nb), dim3(bgzf::STORE_WG), 0, l.stream, d_src, (uint64_t)n_bytes, nb, ob.p);
    if (hipGetLastError() != hipSuccess || hipEventRecord(l.done, l.stream) != hipSuccess) return set_err(ctx, FADEHIP_E_HIP, "bam stream: storing the members failed");
    l.h_out = ob.p;
    *l.h_total = total;
    l.n_bytes = n_bytes;
    l.state = 1;
    return 0;
}

// Where the members of the lane's submission in flight lie, for a kernel enqueued behind it on the lane's stream (the index
// stage of the file path): the block size, and the members' offsets — the scan kernel's member_off[] and total on the
// device, or, for stored members, what the host knows already.
BgzfGeometry bgzf_lane_geometry(const fadehip_ctx *ctx, int lane, bool stored) {
    const BgzfLane &l = ctx->bgzf[lane];
    BgzfGeometry g;
    if (stored) {
        const uint64_t nb = (l.n_bytes + bgzf::STORE_BLOCK - 1) / bgzf::STORE_BLOCK;
        g.block = bgzf::STORE_BLOCK;
        g.member_stride = bgzf::STORE_MEMBER;
        g.behind = l.n_bytes + nb * (uint64_t)(bgzf::STORE_MEMBER - bgzf::STORE_BLOCK);
        return g;
    }
    const uint32_t *d_ticket = (const uint32_t *)l.meta.p + 2 * (size_t)l.n_blocks;
    g.block = (uint32_t)bgzf_block_bytes(l.geom);
    g.member_off = (const uint64_t *)l.member_off.p;
    g.behind_ptr = (const uint64_t *)(((uintptr_t)(d_ticket + 2) + 7) & ~(uintptr_t)7);  // (d_total of bgzf_enqueue)
    return g;
}

}  // namespace fadehip::host

extern "C" {

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


}  // extern "C"
