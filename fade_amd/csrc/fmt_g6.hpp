// fmt_g6.hpp — the text of the reports' float columns: D's to!string(float) of float(num) / float(den), which this tree has
// settled as C's "%g" (append_ratio in host/fade_main.cpp, stats_report_ref.ratio): nan, inf, else six significant digits of
// the float's exact binary value, ties to even, trailing zeros dropped, exponent form outside 1e-05 <= v < 1e+06.
//
// No HIP include and no float arithmetic behind the division: the device (bam_report.hpp) and the host selftest
// (host/selftest/fmt_g6_selftest.cpp) compile the same text.  FMT_G6_HD is what the includer puts in front of a function
// (__host__ __device__ under hipcc, nothing under g++).
//
// The domain is closed: 0, nan, inf, or 2^-31 <= v < 2^39 (numerators stay below 255 * 2^31, denominators below 2^31).
// There v = m * 2^e with 2^23 <= m < 2^24 and -54 <= e <= 15, and 64-bit integers suffice: for six digits at decimal exponent
// X the value wanted is v * 10^k, k = 5 - X in [-6, 15].  k >= 0: m * 5^k (< 2^59) shifted by k + e.  k < 0: (m << e) over
// 10^-k, or m over 10^-k * 2^-e.  Either is one integer with a remainder, rounded half to even.
#pragma once
#include <stdint.h>

#ifndef FMT_G6_HD
#define FMT_G6_HD
#endif

namespace fadehip {

constexpr int FMT_G6_MAX = 16;  // bytes fmt_g6 may write (the longest texts, 1.23457e+06 and 0.000123457, take 11)

// round(v * 10^(5 - X)) for v = m * 2^e, half to even
FMT_G6_HD inline uint64_t fmt_g6_scaled(uint64_t m, int e, int X) {
    const int k = 5 - X;
    uint64_t q, rem, den;  // v * 10^k = q + rem / den
    if (k >= 0) {
        uint64_t N = m;
        for (int j = 0; j < k; j++) N *= 5ull;
        const int s = k + e;
        if (s >= 0) return N << s;
        q = N >> -s;
        den = 1ull << -s;
        rem = N & (den - 1ull);
    } else {
        uint64_t p = 1;
        for (int j = 0; j < -k; j++) p *= 10ull;
        uint64_t N = m;
        if (e >= 0) N <<= e;
        else p <<= -e;
        q = N / p;
        rem = N % p;
        den = p;
    }
    const uint64_t twice = 2ull * rem;  // (rem < den <= 2^54)
    if (twice > den || (twice == den && (q & 1ull))) q++;
    return q;
}

// "%g" of the float whose bits are `bits` (sign clear), into out[0 .. FMT_G6_MAX); returns the number of bytes
FMT_G6_HD inline uint32_t fmt_g6_bits(uint32_t bits, char *out) {
    const uint32_t ex = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    if (ex == 0xffu) {
        out[0] = frac ? 'n' : 'i';
        out[1] = frac ? 'a' : 'n';
        out[2] = frac ? 'n' : 'f';
        return 3;
    }
    if (ex == 0u) {  // zero (a denormal is outside the domain and prints as zero)
        out[0] = '0';
        return 1;
    }
    const uint64_t m = (uint64_t)frac | 0x800000ull;
    const int e = (int)ex - 127 - 23;
    // floor((e + 23) * log10(2)) is the decimal exponent or one below it
    int X = ((e + 23) * 1233) >> 12;
    uint64_t D = fmt_g6_scaled(m, e, X);
    if (D > 1000000ull) D = fmt_g6_scaled(m, e, ++X);
    if (D == 1000000ull) {
        D = 100000ull;
        X++;
    }
    char d[6];
    for (int j = 5; j >= 0; j--) {
        d[j] = (char)('0' + (int)(D % 10ull));
        D /= 10ull;
    }
    int last = 5;  // the last digit that is not a trailing zero
    while (last > 0 && d[last] == '0') last--;
    uint32_t n = 0;
    if (X < -4 || X >= 6) {
        out[n++] = d[0];
        if (last > 0) {
            out[n++] = '.';
            for (int j = 1; j <= last; j++) out[n++] = d[j];
        }
        out[n++] = 'e';
        out[n++] = X < 0 ? '-' : '+';
        const int ax = X < 0 ? -X : X;
        out[n++] = (char)('0' + ax / 10);
        out[n++] = (char)('0' + ax % 10);
    } else if (X >= 0) {
        for (int j = 0; j <= X; j++) out[n++] = d[j];
        if (last > X) {
            out[n++] = '.';
            for (int j = X + 1; j <= last; j++) out[n++] = d[j];
        }
    } else {
        out[n++] = '0';
        out[n++] = '.';
        for (int j = 0; j < -X - 1; j++) out[n++] = '0';
        for (int j = 0; j <= last; j++) out[n++] = d[j];
    }
    return n;
}

// float(num) / float(den), both conversions and the division IEEE round-to-nearest (nothing here is built with fast-math)
FMT_G6_HD inline uint32_t fmt_g6_quotient_bits(uint64_t num, uint64_t den) {
    const float v = (float)num / (float)den;
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b & 0x7fffffffu;  // (0 / 0 gives a nan with its sign set on x86)
}

FMT_G6_HD inline uint32_t fmt_g6_ratio(uint64_t num, uint64_t den, char *out) {
    return fmt_g6_bits(fmt_g6_quotient_bits(num, den), out);
}

}  // namespace fadehip
