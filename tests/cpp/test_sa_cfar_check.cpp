// Stand-alone host test of the argument and pointer check of sa_cfar_f32 (include/specan_cfar.h; sa_cfar_check in
// csrc/sa_cfar_check.cpp).  No GPU, no library: compiled together with sa_cfar_check.cpp by tests/test_f32_cfar_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic is an error
// they report).  The expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to
// 2^31 - 1 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and
// returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_cfar.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, out;
    int rows, log2_train, guard, mode, what, lo, hi;
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
    return (u128)rows * 65536;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2) return SA_EINVAL;
    if (x.mode < 0 || x.mode > 2) return SA_EINVAL;
    if (x.what < 0 || x.what > 1) return SA_EINVAL;
    if (x.log2_train < 0 || x.log2_train > 6) return SA_EINVAL;
    if (x.guard < 0 || x.guard > 64) return SA_EINVAL;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384)) return SA_EINVAL;
    if ((int64_t)x.hi - x.lo < 2 * (int64_t)x.guard + 2) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0) return SA_EINVAL;
    if (x.in % 16 || x.out % 16) return SA_EINVAL;
    if (meet(x.out, bytes_out(x.rows), x.in, bytes_in(x.field, x.rows))) return SA_EINVAL;
    return SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_cfar_check(x.field, x.in, x.out, x.rows, x.log2_train, x.guard, x.mode, x.what, x.lo, x.hi);
    const int exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d in %#llx out %#llx rows %d log2_train %d guard %d mode %d what %d lo %d hi %d: %d, want %d\n", x.field,
                (unsigned long long)x.in, (unsigned long long)x.out, x.rows, x.log2_train, x.guard, x.mode, x.what, x.lo, x.hi, got,
                exp);
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
    if (bytes_in(0, 3) != 196608 || bytes_out(3) != 196608 || bytes_in(2, 1) != 131072 || bytes_out(1) != 65536) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_cfar_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36), away = 1ull << 60;
    const int imin = -2147483647 - 1, imax = 2147483647;
    const Args ok = {0, far, away, 3, 4, 2, 0, 0, 0, 16384};
    // the integers: every one at the ends of its range, one step outside, and at the ends of int32, the others good; with
    // the pointers good, NULL, misaligned and equal, so that a refusal of the parameters is seen to come first
    static const int values[] = {0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 100, 16382, 16383, 16384, 16385, -1, -2, imin, imax};
    static const int rowss[] = {0, 1, 3, 4096, 16777216, imax, -1, imin};
    static const int fields[] = {0, 1, 2, -1, 3};
    for (int which = 0; which < 6; ++which)
        for (int v : values)
            for (int rows : rowss)
                for (int field : fields) {
                    Args a = ok;
                    a.field = field, a.rows = rows;
                    (&a.log2_train)[which] = v;                    // log2_train, guard, mode, what, lo, hi: six ints in a row
                    if (check(a)) return 1;
                    Args b = a;
                    b.in = b.out = 0;
                    if (check(b)) return 1;
                    b = a, b.in = far + 1, b.out = away + 4;
                    if (check(b)) return 1;
                    b = a, b.out = far;
                    if (check(b)) return 1;
                }
    // the range and the guard together: the range holds 2 * guard + 2 bins or it is refused, also at rows 0
    static const int ranges[][2] = {{0, 1}, {0, 2}, {16382, 16384}, {16383, 16384}, {5, 5}, {6, 5}, {0, 16385}, {-1, 16384},
                                    {imin, imax}, {imax, imin}, {100, 229}, {100, 230}, {100, 231}, {1, 131}, {3, 10}};
    for (const int(&r)[2] : ranges)
        for (int guard : {0, 1, 3, 4, 63, 64, 65, -1})
            for (int rows : rowss)
                for (int log2_train : {0, 6, 7}) {
                    Args a = ok;
                    a.lo = r[0], a.hi = r[1], a.guard = guard, a.rows = rows, a.log2_train = log2_train;
                    if (check(a)) return 1;
                    a.in = 0;
                    if (check(a)) return 1;
                }
    // the pointers: `out` against `in` -- touching, overlapping by 1, 4, 8 and 16 bytes, contained, equal, far apart, either
    // first
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, (1ull << 32) - 65536, 0xFFFF000000000000ull,
                                     0xFFFFFFFFFFF00000ull, 1ull << 20};
    static const int rows2[] = {1, 3, 5, 4096, 70000, 16777215, imax};
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t base : bases)
                for (int first = 0; first < 2; ++first) {
                    const u128 n[2] = {bytes_in(field, rows), bytes_out(rows)};
                    const int A = first, B = 1 - first;            // 0 in, 1 out
                    const uint64_t na = (uint64_t)n[A], nb = (uint64_t)n[B];
                    const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16, base + na + 16,
                                              base - nb, base - nb + 1, base - nb + 4, base - nb + 8, base - nb + 16, base - nb - 16,
                                              base, base + 4, base + 8, base + 16, base + (1ull << 31), base - (1ull << 31),
                                              base + (1ull << 32), base - (1ull << 32)};
                    for (uint64_t spot : spots) {
                        uint64_t p[2];
                        p[A] = base, p[B] = spot;
                        if (spot == 0 || !fits(p[A], n[A]) || !fits(p[B], n[B])) continue;
                        Args a = ok;
                        a.field = field, a.rows = rows, a.in = p[0], a.out = p[1];
                        if (check(a)) return 1;
                    }
                }
    // alignment: in 16, out 16
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t o : {1, 2, 4, 8, 12, 16, 24, 32}) {
                Args a = ok;
                a.field = field, a.rows = rows;
                Args b = a;
                b.in += o;
                if (check(b)) return 1;
                b = a, b.out += o;
                if (check(b)) return 1;
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
