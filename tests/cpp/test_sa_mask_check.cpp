// Stand-alone host test of the argument and pointer check of sa_mask_f32 (include/specan_mask.h; sa_mask_check in
// csrc/sa_mask_check.cpp).  No GPU, no library: compiled together with sa_mask_check.cpp by tests/test_f32_mask_cpu.py, under
// the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic is an error they
// report).  The expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to
// 2^31 - 1 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and
// returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_mask.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    uint64_t in;
    int field;
    uint64_t upper, lower;
    int lo, hi;
    uint64_t rows_out, summary;
    int rows;
};

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return na > 0 && nb > 0 && a < b + nb && b < a + na;
}

// the five byte ranges of the header, a NULL limit and a NULL summary being empty
static void sizes(const Args &x, u128 n[5])
{
    n[0] = (u128)x.rows * 65536 * (x.field ? 2 : 1);
    n[1] = x.upper ? 65536 : 0;
    n[2] = x.lower ? 65536 : 0;
    n[3] = (u128)x.rows * 40;
    n[4] = x.summary ? 16 : 0;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2) return SA_EINVAL;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384)) return SA_EINVAL;
    if (x.upper == 0 && x.lower == 0) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.rows_out == 0) return SA_EINVAL;
    if (x.in % 16 || x.upper % 16 || x.lower % 16 || x.rows_out % 8 || x.summary % 4) return SA_EINVAL;
    u128 n[5];
    sizes(x, n);
    const uint64_t p[5] = {x.in, x.upper, x.lower, x.rows_out, x.summary};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) {
            if (i == 1 && j == 2 && x.upper == x.lower) continue;              // one line as both limits
            if (meet(p[i], n[i], p[j], n[j])) return SA_EINVAL;
        }
    return SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_mask_check(x.in, x.field, x.upper, x.lower, x.lo, x.hi, x.rows_out, x.summary, x.rows), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d [%d, %d) in %#llx upper %#llx lower %#llx rows_out %#llx summary %#llx: %d, want %d\n", x.field,
                x.rows, x.lo, x.hi, (unsigned long long)x.in, (unsigned long long)x.upper, (unsigned long long)x.lower,
                (unsigned long long)x.rows_out, (unsigned long long)x.summary, got, exp);
    return 1;
}

// does [a, a + n) stay below 2^64?  A range that wraps is outside what any address space holds: not part of the contract
static bool fits(uint64_t a, u128 n)
{
    return (u128)a + n <= ((u128)1 << 64);
}

int main()
{
    // the header's known answers, by byte count
    {
        u128 n[5];
        sizes({16, 0, 16, 16, 0, 1, 16, 16, 3}, n);
        const bool a = n[0] == 196608 && n[1] == 65536 && n[2] == 65536 && n[3] == 120 && n[4] == 16;
        sizes({16, 2, 16, 0, 0, 1, 16, 0, 1}, n);
        if (!a || n[0] != 131072 || n[1] != 65536 || n[2] != 0 || n[3] != 40 || n[4] != 0 || sizeof(sa_mask_row) != 40) {
            std::printf("FAILED known answers\n");
            return 1;
        }
    }
    if (std::strcmp(sa_mask_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    const uint64_t away[5] = {1ull << 60, 5ull << 58, 3ull << 59, 7ull << 58, 1ull << 61};      // 2^48 bytes fit between them
    // the scalar arguments and the two limits being NULL, each alone and with the pointers wrong too
    static const int fields[] = {0, 1, 2, -1, 3};
    static const int ranges[][2] = {{0, 16384}, {0, 1}, {16383, 16384}, {5, 5}, {6, 5}, {-1, 5}, {0, 16385}, {16384, 16385},
                                    {-2147483647 - 1, 2147483647}, {1023, 1025}};
    static const int rowss[] = {0, 1, 3, 4096, 16777216, 2147483647, -1, -2147483647 - 1};
    for (int field : fields)
        for (auto &rg : ranges)
            for (int limits = 0; limits < 4; ++limits)             // bit 0: upper given, bit 1: lower given
                for (int rows : rowss) {
                    const uint64_t up = limits & 1 ? away[1] : 0, low = limits & 2 ? away[2] : 0;
                    if (check({far, field, up, low, rg[0], rg[1], away[3], away[4], rows})) return 1;
                    if (check({far, field, up, low, rg[0], rg[1], away[3], 0, rows})) return 1;
                    if (check({0, field, up, low, rg[0], rg[1], 0, 0, rows})) return 1;
                    if (check({far + 1, field, up ? up + 4 : 0, low ? low + 8 : 0, rg[0], rg[1], away[3] + 4, away[4] + 2, rows})) return 1;
                    if (check({far, field, up ? far : 0, low ? far : 0, rg[0], rg[1], far, far, rows})) return 1;
                }
    // the pointers: each pair of the five ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, equal, far apart,
    // the other ranges out of the way; upper == lower is the one pair that may be equal
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, 0xFFFF000000000000ull, 0xFFFFFFFFFFF00000ull, 1ull << 20};
    static const int rows2[] = {1, 3, 5, 4096, 70000, 16777215, 2147483647};
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t base : bases)
                for (int a = 0; a < 5; ++a)
                    for (int b = 0; b < 5; ++b) {                  // range a at `base`, range b placed against it
                        if (a == b) continue;
                        Args x = {away[0], field, away[1], away[2], 0, 16384, away[3], away[4], rows};
                        u128 n[5];
                        sizes(x, n);
                        const uint64_t na = (uint64_t)n[a], nb = (uint64_t)n[b];
                        const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16, base + na + 16,
                                                  base - nb, base - nb + 1, base - nb + 4, base - nb + 8, base - nb + 16, base - nb - 16,
                                                  base, base + 4, base + 16, base + (1ull << 31), base - (1ull << 31)};
                        for (uint64_t spot : spots) {
                            uint64_t p[5] = {away[0], away[1], away[2], away[3], away[4]};
                            p[a] = base, p[b] = spot;
                            if (spot == 0 || !fits(p[a], n[a]) || !fits(p[b], n[b])) continue;
                            if (check({p[0], field, p[1], p[2], 0, 16384, p[3], p[4], rows})) return 1;
                        }
                    }
    // alignment: in and the limits 16, rows_out 8, summary 4; and the limits and the summary left out
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2) {
            for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                if (check({far + off, field, away[1], away[2], 0, 16384, away[3], away[4], rows})) return 1;
                if (check({far, field, away[1] + off, away[2], 0, 16384, away[3], away[4], rows})) return 1;
                if (check({far, field, away[1], away[2] + off, 0, 16384, away[3], away[4], rows})) return 1;
                if (check({far, field, away[1], away[2], 0, 16384, away[3] + off, away[4], rows})) return 1;
                if (check({far, field, away[1], away[2], 0, 16384, away[3], away[4] + off, rows})) return 1;
            }
            if (check({far, field, away[1], away[1], 3, 9, away[3], away[4], rows})) return 1;       // one line as both limits
            if (check({far, field, 0, away[2], 3, 9, away[3], 0, rows})) return 1;
            if (check({far, field, away[1], 0, 3, 9, away[3], 0, rows})) return 1;
        }
    std::printf("ok %d\n", g_checks);
    return 0;
}
