// Stand-alone host test of the argument and pointer check of sa_signals_f32 (include/specan_signals.h; sa_signals_check in
// csrc/sa_signals_check.cpp).  No GPU, no library: compiled together with sa_signals_check.cpp by
// tests/test_f32_signals_cpu.py, under the address and undefined-behaviour sanitizers where they link (a signed overflow in
// the byte arithmetic is an error they report).  The expected answer is this file's own evaluation of the header's rules in
// 128-bit integers, at rows up to 2^31 - 1 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or
// names the first failed check and returns 1.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_signals.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, thr;
    uint32_t bits;
    uint64_t out, stats;
    int rows, k, lo, hi, gap, min_width;
};

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return na > 0 && nb > 0 && a < b + nb && b < a + na;
}

static u128 bytes_in(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 bytes_out(int rows, int k)
{
    return (u128)rows * (u128)k * 24;
}

static u128 bytes_stats(int rows)
{
    return (u128)rows * 12;
}

static u128 bytes_thr(uint64_t thr, int rows)
{
    return thr ? (u128)rows * 4 : 0;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2) return SA_EINVAL;
    if (x.k < 1 || x.k > 32) return SA_EINVAL;
    if (x.thr == 0 && x.bits > 0x7F800000u) return SA_EINVAL;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384)) return SA_EINVAL;
    if (x.gap < 0 || x.gap > 16383) return SA_EINVAL;
    if (x.min_width < 1 || x.min_width > 16384) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0 || x.stats == 0) return SA_EINVAL;
    if (x.in % 16 || x.out % 8 || x.stats % 4 || x.thr % 4) return SA_EINVAL;
    const u128 n_in = bytes_in(x.field, x.rows), n_out = bytes_out(x.rows, x.k), n_stats = bytes_stats(x.rows),
               n_thr = bytes_thr(x.thr, x.rows);
    if (meet(x.out, n_out, x.stats, n_stats) || meet(x.out, n_out, x.in, n_in) || meet(x.out, n_out, x.thr, n_thr) ||
        meet(x.stats, n_stats, x.in, n_in) || meet(x.stats, n_stats, x.thr, n_thr))
        return SA_EINVAL;
    return SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_signals_check(x.field, x.in, x.thr, x.bits, x.out, x.stats, x.rows, x.k, x.lo, x.hi, x.gap, x.min_width);
    const int exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d in %#llx thr %#llx bits %#x out %#llx stats %#llx rows %d k %d lo %d hi %d gap %d min_width %d: %d, want %d\n",
                x.field, (unsigned long long)x.in, (unsigned long long)x.thr, (unsigned)x.bits, (unsigned long long)x.out,
                (unsigned long long)x.stats, x.rows, x.k, x.lo, x.hi, x.gap, x.min_width, got, exp);
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
    if (bytes_in(0, 3) + bytes_thr(4, 3) != 196608 + 12 || bytes_out(3, 8) + bytes_stats(3) != 576 + 36 || bytes_in(2, 1) != 131072 ||
        bytes_out(1, 32) + bytes_stats(1) != 768 + 12 || sizeof(sa_signal) != 24 || offsetof(sa_signal, stop) != 4 ||
        offsetof(sa_signal, peak) != 8 || offsetof(sa_signal, peak_bin) != 12 || offsetof(sa_signal, power) != 16) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_signals_last_error(), "") != 0) {       // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36), away = 1ull << 60, apart = 1ull << 61, off = 1ull << 59;
    const int imin = -2147483647 - 1, imax = 2147483647;
    const Args ok = {0, far, 0, 0u, away, apart, 3, 8, 0, 16384, 0, 1};
    // the integers: every one at the ends of its range, one step outside, and at the ends of int32, the others good; with
    // the pointers good, NULL, misaligned and equal, so that a refusal of the parameters is seen to come first
    static const int values[] = {0, 1, 2, 3, 31, 32, 33, 100, 16382, 16383, 16384, 16385, -1, -2, imin, imax};
    static const int rowss[] = {0, 1, 3, 4096, 16777216, imax, -1, imin};
    static const int fields[] = {0, 1, 2, -1, 3};
    for (int which = 0; which < 5; ++which)
        for (int v : values)
            for (int rows : rowss)
                for (int field : fields) {
                    Args a = ok;
                    a.field = field, a.rows = rows;
                    (&a.k)[which] = v;                             // k, lo, hi, gap, min_width: five ints in a row
                    if (check(a)) return 1;
                    Args b = a;
                    b.in = b.out = b.stats = 0;
                    if (check(b)) return 1;
                    b = a, b.in = far + 1, b.out = away + 4, b.stats = apart + 2, b.thr = off + 1;
                    if (check(b)) return 1;
                    b = a, b.out = b.stats = far;
                    if (check(b)) return 1;
                }
    // the range as a pair, and the threshold: its bits count only without `thr`
    static const int ranges[][2] = {{0, 1}, {16383, 16384}, {5, 5}, {6, 5}, {0, 16385}, {-1, 16384}, {imin, imax}, {imax, imin}, {100, 200}};
    static const uint32_t bitss[] = {0u, 1u, 0x3F800000u, 0x7F7FFFFFu, 0x7F800000u, 0x7F800001u, 0x7FC00000u, 0x80000000u, 0xBF800000u,
                                     0xFF800000u, 0xFFFFFFFFu};
    for (const int(&r)[2] : ranges)
        for (uint32_t bits : bitss)
            for (uint64_t thr : {(uint64_t)0, off, off + 2})
                for (int rows : rowss) {
                    Args a = ok;
                    a.lo = r[0], a.hi = r[1], a.bits = bits, a.thr = thr, a.rows = rows;
                    if (check(a)) return 1;
                    a.in = 0;
                    if (check(a)) return 1;
                }
    // the pointers: each written range against each other range -- touching, overlapping by 1, 4, 8 and 16 bytes, contained,
    // equal, far apart, either first; and `in` against `thr`, which may meet
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, (1ull << 32) - 24, 0xFFFF000000000000ull,
                                     0xFFFFFFFFFFF00000ull, 1ull << 20};
    static const int rows2[] = {1, 3, 5, 4096, 70000, 16777215, imax};
    static const int pairs[][2] = {{2, 0}, {3, 0}, {2, 3}, {2, 1}, {3, 1}, {0, 1}};     // 0 in, 1 thr, 2 out, 3 stats
    static const uint64_t parked[4] = {1ull << 58, 0, 3ull << 58, 5ull << 58};          // where the other two stay
    for (int field = 0; field < 3; ++field)
        for (int k : {1, 8, 32})
            for (int rows : rows2)
                for (uint64_t base : bases)
                    for (const int(&pr)[2] : pairs)
                        for (int first = 0; first < 2; ++first) {
                            const u128 n[4] = {bytes_in(field, rows), bytes_thr(4, rows), bytes_out(rows, k), bytes_stats(rows)};
                            const int A = pr[first], B = pr[1 - first];
                            const uint64_t na = (uint64_t)n[A], nb = (uint64_t)n[B];
                            const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16,
                                                      base + na + 16, base - nb, base - nb + 1, base - nb + 4, base - nb + 8,
                                                      base - nb + 16, base - nb - 16, base, base + 4, base + 8, base + 16,
                                                      base + (1ull << 31), base - (1ull << 31), base + (1ull << 32), base - (1ull << 32)};
                            for (uint64_t spot : spots) {
                                uint64_t p[4] = {parked[0], parked[1], parked[2], parked[3]};
                                p[A] = base, p[B] = spot;
                                if (spot == 0 || !fits(p[A], n[A]) || !fits(p[B], n[B])) continue;
                                bool clear = true;                 // the parked ranges stay out of the pair's way
                                for (int o = 0; o < 4; ++o)
                                    for (int q : {A, B})
                                        if (o != A && o != B && p[o] && meet(p[o], n[o], p[q], n[q])) clear = false;
                                if (!clear) continue;
                                Args a = ok;
                                a.field = field, a.k = k, a.rows = rows, a.in = p[0], a.thr = p[1], a.out = p[2], a.stats = p[3];
                                if (check(a)) return 1;
                            }
                        }
    // alignment: in 16, out 8, stats 4, thr 4
    for (int field = 0; field < 3; ++field)
        for (int rows : rows2)
            for (uint64_t o : {1, 2, 4, 8, 12, 16, 24}) {
                Args a = ok;
                a.field = field, a.rows = rows, a.thr = off;
                Args b = a;
                b.in += o;
                if (check(b)) return 1;
                b = a, b.out += o;
                if (check(b)) return 1;
                b = a, b.stats += o;
                if (check(b)) return 1;
                b = a, b.thr += o;
                if (check(b)) return 1;
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
