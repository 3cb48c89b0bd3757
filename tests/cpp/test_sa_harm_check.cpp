// Stand-alone host test of the argument and pointer check of sa_harm_f32 (include/specan_harm.h; sa_harm_check in
// csrc/sa_harm_check.cpp).  No GPU, no library: compiled together with sa_harm_check.cpp by tests/test_f32_harm_cpu.py, under
// the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic is an error they
// report).  The expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to
// 2^31 - 1 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and
// returns 1.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_harm.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, out;
    int rows;
    const sa_harm_cfg *cfg;
};

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return na > 0 && nb > 0 && a < b + nb && b < a + na;
}

static u128 bytes_in(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 bytes_out(int rows)
{
    return (u128)rows * 168;
}

// the ranges of the header's parameter list, in 64-bit integers so that no int32 value can overflow a sum here
static bool good(const sa_harm_cfg &c)
{
    const int64_t dc = c.dc, top = c.top, lo = c.lo, hi = c.hi, fund = c.fund, span = c.span, order = c.order;
    if (!(0 <= dc && dc < top && top <= 8193)) return false;
    if (!(dc <= lo && lo < hi && hi <= top)) return false;
    if (!(fund == -1 || (dc <= fund && fund < top))) return false;
    if (!(0 <= span && span <= 64)) return false;
    return 1 <= order && order <= 10;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2) return SA_EINVAL;
    if (x.cfg == nullptr || !good(*x.cfg)) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0) return SA_EINVAL;
    if (x.in % 16 || x.out % 8) return SA_EINVAL;
    return meet(x.in, bytes_in(x.field, x.rows), x.out, bytes_out(x.rows)) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_harm_check(x.field, x.in, x.out, x.rows, x.cfg), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d in %#llx out %#llx cfg %s", x.field, x.rows, (unsigned long long)x.in, (unsigned long long)x.out,
                x.cfg ? "" : "NULL");
    if (x.cfg)
        std::printf("(dc %d top %d lo %d hi %d fund %d span %d order %d)", x.cfg->dc, x.cfg->top, x.cfg->lo, x.cfg->hi, x.cfg->fund,
                    x.cfg->span, x.cfg->order);
    std::printf(": %d, want %d\n", got, exp);
    return 1;
}

// does [a, a + n) stay below 2^64?  A range that wraps is outside what any address space holds: not part of the contract
static bool fits(uint64_t a, u128 n)
{
    return (u128)a + n <= ((u128)1 << 64);
}

int main()
{
    // the header's known answers, by byte count, and the record's layout
    if (bytes_in(0, 3) != 196608 || bytes_out(3) != 504 || bytes_in(2, 1) != 131072 || bytes_out(1) != 168 || sizeof(sa_harm_row) != 168 ||
        sizeof(sa_harm_cfg) != 28 || offsetof(sa_harm_row, dist) != 80 || offsetof(sa_harm_row, nad) != 88 ||
        offsetof(sa_harm_row, noise) != 96 || offsetof(sa_harm_row, bin) != 104 || offsetof(sa_harm_row, fund) != 144 ||
        offsetof(sa_harm_row, spur) != 148 || offsetof(sa_harm_row, nonharm) != 152 || offsetof(sa_harm_row, spur_bin) != 156 ||
        offsetof(sa_harm_row, nonharm_bin) != 160 || offsetof(sa_harm_row, n_noise) != 164) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_harm_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36), away = 1ull << 60;
    const int imin = -2147483647 - 1, imax = 2147483647;
    const sa_harm_cfg ok = {4, 8193, 4, 8193, -1, 3, 5};
    // the parameters: every field at the ends of its range, one step outside, and at the ends of int32, the others good
    static const int values[] = {0, 1, 3, 4, 5, 10, 11, 63, 64, 65, 100, 4000, 8191, 8192, 8193, 8194, 16384, -1, -2, imin, imax};
    static const int rowss[] = {0, 1, 3, 4096, 16777216, imax, -1, imin};
    static const int fields[] = {0, 1, 2, -1, 3};
    for (int which = 0; which < 7; ++which)
        for (int v : values)
            for (int rows : rowss)
                for (int field : fields) {
                    sa_harm_cfg c = ok;
                    (&c.dc)[which] = v;                            // seven int32 in a row (sizeof 28 above)
                    if (check({field, far, away, rows, &c})) return 1;
                    if (check({field, 0, 0, rows, &c})) return 1;                      // the pointers wrong as well
                    if (check({field, far + 1, away + 4, rows, &c})) return 1;
                    if (check({field, far, far, rows, &c})) return 1;
                }
    // pairs of parameters that are only wrong together, a NULL cfg, and the smallest and largest good sets
    static const sa_harm_cfg sets[] = {{0, 1, 0, 1, -1, 0, 1},     {0, 1, 0, 1, 0, 64, 10},      {0, 8193, 0, 8193, 8192, 64, 10},
                                       {8192, 8193, 8192, 8193, 8192, 0, 1}, {5, 5, 5, 5, -1, 3, 5},      {6, 5, 5, 6, -1, 3, 5},
                                       {4, 100, 3, 100, -1, 3, 5},  {4, 100, 4, 101, -1, 3, 5},   {4, 100, 50, 50, -1, 3, 5},
                                       {4, 100, 51, 50, -1, 3, 5},  {4, 100, 4, 100, 3, 3, 5},    {4, 100, 4, 100, 100, 3, 5},
                                       {4, 100, 4, 100, 99, 3, 5},  {4, 100, 4, 100, 4, 3, 5},    {4, 100, 10, 20, 50, 3, 5},
                                       {imin, imax, imin, imax, imin, imin, imin}, {imax, imin, imax, imin, imax, imax, imax},
                                       {0, imax, 0, imax, -1, 3, 5}, {imin, 8193, imin, 8193, -1, 3, 5}};
    for (const sa_harm_cfg &c : sets)
        for (int rows : rowss)
            for (int field : fields) {
                if (check({field, far, away, rows, &c})) return 1;
                if (check({field, 0, 0, rows, &c})) return 1;
                if (check({field, far, far, rows, nullptr})) return 1;
                if (check({field, far, away, rows, nullptr})) return 1;
            }
    // the pointers: the two ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, equal, far apart, either first
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, (1ull << 32) - 168, 0xFFFF000000000000ull,
                                     0xFFFFFFFFFFF00000ull, 1ull << 20};
    static const int rows2[] = {1, 3, 5, 4096, 70000, 16777215, imax};
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t base : bases)
                for (int first = 0; first < 2; ++first) {          // the range placed at `base`: 0 `in`, 1 `out`
                    const u128 n[2] = {bytes_in(field, rows), bytes_out(rows)};
                    const uint64_t na = (uint64_t)n[first], nb = (uint64_t)n[1 - first];
                    const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16, base + na + 16,
                                              base - nb, base - nb + 1, base - nb + 4, base - nb + 8, base - nb + 16, base - nb - 16,
                                              base, base + 4, base + 8, base + 16, base + (1ull << 31), base - (1ull << 31),
                                              base + (1ull << 32), base - (1ull << 32)};
                    for (uint64_t spot : spots) {
                        uint64_t p[2];
                        p[first] = base, p[1 - first] = spot;
                        if (spot == 0 || !fits(p[0], n[0]) || !fits(p[1], n[1])) continue;
                        if (check({field, p[0], p[1], rows, &ok})) return 1;
                    }
                }
    // alignment: in 16, out 8
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t off : {1, 2, 4, 8, 12, 16, 24}) {
                if (check({field, far + off, away, rows, &ok})) return 1;
                if (check({field, far, away + off, rows, &ok})) return 1;
                if (check({field, (1ull << 33) + off, (1ull << 34) + off, rows, &ok})) return 1;
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
