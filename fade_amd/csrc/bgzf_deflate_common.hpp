// bgzf_deflate_common.hpp — what the compressor's two block geometries (bgzf_deflate_g64.hpp, bgzf_deflate_g32.hpp) share:
// the constants no geometry changes, the kernels' argument block, the LDS and lane-array helpers, and the two kernels
// behind the compressor (the scan of the members' sizes, the pack of the members).  The inflater takes claim_ticket from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bgzf_huff.hpp"

namespace fadehip {
namespace bgzf {

constexpr int DIST_T0 = 320;  // threads DIST_T0 .. + 29 serve the distance alphabet where the first 286 serve literals / lengths
constexpr int WAYS = 4;       // 16-bit positions in a bucket of a hash table
constexpr int MIN_MATCH = 4, MAX_MATCH = 258;
constexpr int SLOT = 65536;   // bytes of a block's output slot (payload <= 65510: BSIZE is 16 bits)
constexpr int MAX_PAYLOAD = 65536 - 26;
// ... of the head region once the matches are found
constexpr int H_H8 = 0, H_AL = H_H8 + 8 * 320 * 4, H_SL = H_AL + 320 * 4, H_AD = H_SL + 320 * 4, H_SD = H_AD + 64 * 4, H_END = H_SD + 64 * 4;

struct DeflateArgs {
    const uint8_t *src;   // the byte stream (device)
    uint64_t n_bytes;
    uint32_t n_blocks;
    uint8_t *slots;       // [n_blocks][SLOT]
    uint32_t *out_size;   // [n_blocks] payload bytes
    uint32_t *out_crc;    // [n_blocks]
    uint32_t *ticket;     // blocks are drawn from here
    unsigned long long *prof;  // optional [8]: shader clocks per phase, summed over blocks by lane 0 (FADEHIP_BGZF_PROF)
};

__device__ __forceinline__ uint32_t lds_load32u(const uint8_t *base, uint32_t p) {  // 4 bytes at any offset
    const uint32_t *w = reinterpret_cast<const uint32_t *>(base) + (p >> 2);
    return __builtin_amdgcn_alignbyte(w[1], w[0], p & 3u);
}
__device__ __forceinline__ uint64_t lds_load64u(const uint8_t *base, uint32_t p) {  // 8 bytes at any offset
    const uint32_t *w = reinterpret_cast<const uint32_t *>(base) + (p >> 2);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, p & 3u) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, p & 3u) << 32);
}

// the next ticket of a wave-shared counter, as a wave-uniform value (kept out of line: inlined into the extenders' loop of
// the role pipeline the claim was hoisted around the loop's exec-mask bookkeeping and a back edge re-used a stale ticket)
__device__ __noinline__ int claim_ticket(uint32_t *counter) {
    uint32_t tk = 0;
    if ((threadIdx.x & 63) == 0) tk = atomicAdd(counter, 1u);
    return __builtin_amdgcn_readlane((int)tk, 0);
}

// exclusive scan of one value per thread over a workgroup of N_WAVES waves (tmp: N_WAVES words of LDS); *total = the sum
template <int N_WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *tmp, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // tmp may still be read from an earlier scan
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < N_WAVES; w++) {
        const uint32_t t = tmp[w];
        if (w < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// An array of up to 64 NR entries spread over the lanes of a wavefront (entry i in lane i % 64 of register i / 64), read
// and written with v_readlane / v_writelane by code the whole wave runs in lockstep on wave-uniform indices: the accessor
// the serial Huffman routines of bgzf_huff.hpp take on the device (a dependent LDS round trip costs ~130 clocks, a lane
// access ~10, and those routines are chains of dependent accesses).
template <int NR>
struct WaveArr {
    uint32_t r[NR];
    __device__ __forceinline__ uint32_t get(int i) const {  // i is wave-uniform
        const int k = i >> 6, l = i & 63;
        uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r[0], l);
#pragma unroll
        for (int j = 1; j < NR; j++)
            if (k == j) v = (uint32_t)__builtin_amdgcn_readlane((int)r[j], l);
        return v;
    }
    __device__ __forceinline__ void set(int i, uint32_t v) {  // i and v are wave-uniform
        const int k = i >> 6, l = i & 63;
#pragma unroll
        for (int j = 0; j < NR; j++)
            if (k == j) asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(r[j]) : "s"(v), "s"(l) : "m0");  // (one SGPR per VALU instruction)
    }
};
// bit sink of the header: whole words to LDS by lane 0, the accumulator wave-uniform
struct LdsSink {
    uint32_t *w;
    uint64_t acc = 0;
    int cnt = 0;
    uint32_t wi = 0;
    __device__ __forceinline__ void put(uint32_t v, int n) {
        acc |= (uint64_t)v << cnt;
        cnt += n;
        if (cnt >= 32) {
            if ((threadIdx.x & 63) == 0) w[wi] = (uint32_t)acc;
            wi++;
            acc >>= 32;
            cnt -= 32;
        }
    }
    __device__ __forceinline__ uint32_t finish() {
        if (cnt && (threadIdx.x & 63) == 0) w[wi] = (uint32_t)acc;
        return 32u * wi + (uint32_t)cnt;
    }
};

// bits of the token that starts at bit b of bitmap word w (a literal, or the match whose record the match bitmap counts to);
// MiscT: a geometry's Misc, of which the codes (lc, dc) and their lengths (ll, dl) are read
template <class MiscT>
__device__ __forceinline__ void token_bits(const uint8_t *data, uint32_t mw, uint32_t mbase, const uint32_t *match, const MiscT *ms, int w, int b,
                                           uint64_t &bits, int &nb) {
    if ((mw >> b) & 1u) {
        const uint32_t rec = match[mbase + (uint32_t)__builtin_popcount(mw & ((1u << b) - 1u))];
        const Sym ls = length_symbol((rec >> 16) + 3u), ds = dist_symbol(rec & 0xffffu);
        uint64_t v = ms->lc[ls.sym];
        int k = ms->ll[ls.sym];
        v |= (uint64_t)ls.eval << k;
        k += (int)ls.ebits;
        v |= (uint64_t)ms->dc[ds.sym] << k;
        k += ms->dl[ds.sym];
        v |= (uint64_t)ds.eval << k;
        k += (int)ds.ebits;
        bits = v;
        nb = k;
    } else {
        const uint32_t c = data[32 * w + b];
        bits = ms->lc[c];
        nb = ms->ll[c];
    }
}

// exclusive scan of the members' sizes (payload + 26 bytes of BGZF header and trailer): one workgroup
__global__ __launch_bounds__(1024) void bgzf_scan_kernel(const uint32_t *out_size, uint32_t n_blocks, uint64_t *member_off, uint64_t *total) {
    __shared__ uint64_t part[1024];
    const int tid = threadIdx.x;
    const uint32_t per = (n_blocks + 1023u) / 1024u, lo = (uint32_t)tid * per, hi = min(lo + per, n_blocks);
    __shared__ int failed;
    if (tid == 0) failed = 0;
    __syncthreads();
    uint64_t s = 0;
    for (uint32_t k = lo; k < hi; k++) {
        if (out_size[k] > (uint32_t)MAX_PAYLOAD) failed = 1;  // a block the compressor gave up on (bgzf_deflate_g64.hpp spin_until)
        s += (uint64_t)out_size[k] + 26u;
    }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int k = 0; k < 1024; k++) { const uint64_t c = part[k]; part[k] = run; run += c; }
        *total = failed ? 0ull : run;  // 0: the host reports the failure instead of copying anything
    }
    __syncthreads();
    uint64_t at = part[tid];
    for (uint32_t k = lo; k < hi; k++) { member_off[k] = at; at += (uint64_t)out_size[k] + 26u; }
}

// member k = 18 bytes of header (BSIZE in the BC subfield), the payload, CRC32, ISIZE — packed one after the other.
// BLOCK: the geometry's block size, which only ISIZE needs (an instance per geometry: the constant stays an immediate)
template <int BLOCK>
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t *slots, const uint32_t *out_size, const uint32_t *out_crc,
                                                        const uint64_t *member_off, uint64_t n_bytes, uint32_t n_blocks, uint8_t *dst) {
    const uint32_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const uint32_t sz = out_size[blk];
    if (sz > (uint32_t)MAX_PAYLOAD) return;  // (a failed block: nothing is packed, the scan has zeroed the total)
    uint8_t *d = dst + member_off[blk];
    const uint8_t *s = slots + (uint64_t)blk * SLOT;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const uint32_t bsize = sz + 25u;  // total member size - 1
        const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255u), (uint8_t)(bsize >> 8)};
        for (int k = 0; k < 18; k++) d[k] = h[k];
        const uint64_t off = (uint64_t)blk * BLOCK;
        const uint32_t isize = (uint32_t)(n_bytes - off < (uint64_t)BLOCK ? n_bytes - off : (uint64_t)BLOCK), crc = out_crc[blk];
        uint8_t *t = d + 18 + sz;
        for (int k = 0; k < 4; k++) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)(isize >> (8 * k)); }
    }
    // payload: destination-aligned dwords assembled from the (aligned) slot, the ragged ends byte by byte
    uint8_t *p = d + 18;
    const uint32_t mis = (uint32_t)((4u - ((uintptr_t)p & 3u)) & 3u), headn = mis < sz ? mis : sz;
    if ((uint32_t)tid < headn) p[tid] = s[tid];
    const uint32_t body = (sz - headn) >> 2;
    uint32_t *p32 = reinterpret_cast<uint32_t *>(p + headn);
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s);
    for (uint32_t k = tid; k < body; k += 256) {
        const uint32_t so = headn + 4u * k;  // source byte offset of this destination word
        p32[k] = __builtin_amdgcn_alignbyte(s32[(so >> 2) + 1], s32[so >> 2], so & 3u);
    }
    const uint32_t done = headn + 4u * body;
    if ((uint32_t)tid < sz - done) p[done + tid] = s[done + tid];
}

}  // namespace bgzf
}  // namespace fadehip
