// fmt_g6_selftest — fmt_g6.hpp (the text of the reports' float columns, the function the device compiles) against libc's
// snprintf("%g") of the same float quotient (CPU only; ASan + UBSan build).  Every num / den with den 1 .. 256 and
// num 0 .. 255 * den, the named edges, and two million seeded random bit patterns with binary exponent in [-31, 38].
// Prints the number of values and of differences; exit status 1 when there is any.
#include "../../fmt_g6.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>

static unsigned long long n_checked = 0, n_diff = 0;

static void want_text(const char *what, unsigned long long a, unsigned long long b, const char *got, unsigned n, const char *want) {
    n_checked++;
    if (n == strlen(want) && !memcmp(got, want, n)) return;
    if (n_diff++ < 20) fprintf(stderr, "%s %llu / %llu: fmt_g6 '%.*s', libc '%s'\n", what, a, b, (int)n, got, want);
}

static void libc_g(float v, char *want, size_t cap) {
    if (std::isnan(v)) snprintf(want, cap, "nan");
    else if (std::isinf(v)) snprintf(want, cap, "inf");
    else snprintf(want, cap, "%g", (double)v);
}

static void check_ratio(unsigned long long num, unsigned long long den) {
    char got[fadehip::FMT_G6_MAX], want[64];
    const unsigned n = fadehip::fmt_g6_ratio(num, den, got);
    libc_g((float)num / (float)den, want, sizeof want);
    want_text("ratio", num, den, got, n, want);
}

static void check_bits(uint32_t bits) {
    char got[fadehip::FMT_G6_MAX], want[64];
    float v;
    memcpy(&v, &bits, 4);
    const unsigned n = fadehip::fmt_g6_bits(bits, got);
    libc_g(v, want, sizeof want);
    want_text("bits", bits, 0, got, n, want);
}

int main() {
    for (unsigned long long den = 1; den <= 256; den++)
        for (unsigned long long num = 0; num <= 255 * den; num++) check_ratio(num, den);
    check_ratio(0, 0);
    check_ratio(1, 0);
    check_ratio(1, 2147483647ull);
    check_ratio(255ull * 2147483647ull, 1);
    check_ratio(1999999, 2);
    check_ratio(1, 10000);
    check_ratio(1, 20000);
    check_ratio(3, 30001);
    {  // 1999999 / 2 rounds up into the exponent form, 1 / 20000 is the first value below 1e-04's form
        char got[fadehip::FMT_G6_MAX];
        unsigned n = fadehip::fmt_g6_ratio(1999999, 2, got);
        want_text("edge", 1999999, 2, got, n, "1e+06");
        n = fadehip::fmt_g6_ratio(1, 20000, got);
        want_text("edge", 1, 20000, got, n, "5e-05");
        n = fadehip::fmt_g6_ratio(1, 10000, got);
        want_text("edge", 1, 10000, got, n, "0.0001");
    }
    // the smallest and the largest value of the domain, and every power of two between
    for (int e = -31; e <= 38; e++) {
        check_bits((uint32_t)(e + 127) << 23);
        check_bits(((uint32_t)(e + 127) << 23) | 0x7fffffu);
    }
    uint64_t s = 0x9e3779b97f4a7c15ull;  // splitmix64
    for (int k = 0; k < 2000000; k++) {
        s += 0x9e3779b97f4a7c15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        const uint32_t ex = (uint32_t)((z >> 32) % 70u) + 96u;  // biased exponents 96 .. 165: 2^-31 .. 2^38
        check_bits((ex << 23) | ((uint32_t)z & 0x7fffffu));
    }
    printf("fmt_g6_selftest: %llu values, %llu differences\n", n_checked, n_diff);
    return n_diff ? 1 : 0;
}
