// Stand-alone host test of the argument and pointer check of sa_peaks_f32 (include/specan_peaks.h; sa_peaks_check in
// csrc/sa_peaks_check.cpp).  No GPU, no library: compiled together with sa_peaks_check.cpp by tests/test_f32_peaks_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow or an out-of-range shift in the
// byte arithmetic is an error they report).  The expected answer is this file's own evaluation of the header's rules in
// 128-bit integers, at rows up to 2^31 - 1 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or
// names the first failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_peaks.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, out, count;
    int rows, k;
    uint32_t thr;
    int lo, hi, min_sep;
};

static u128 in_bytes(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 out_bytes(int rows, int k)
{
    return (u128)rows * (u128)k * 8;
}

static u128 count_bytes(int rows)
{
    return (u128)rows * 4;
}

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return a < b + nb && b < a + na;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2 || x.k < 1 || x.k > 32) return SA_EINVAL;
    if ((x.thr & 0x80000000u) || (x.thr & 0x7FFFFFFFu) > 0x7F800000u) return SA_EINVAL;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384) || x.min_sep < 1 || x.min_sep > 16384) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0 || x.count == 0 || x.in % 16 || x.out % 8 || x.count % 4) return SA_EINVAL;
    const u128 ni = in_bytes(x.field, x.rows), no = out_bytes(x.rows, x.k), nc = count_bytes(x.rows);
    return meet(x.in, ni, x.out, no) || meet(x.in, ni, x.count, nc) || meet(x.out, no, x.count, nc) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_peaks_check(x.field, x.in, x.out, x.count, x.rows, x.k, x.thr, x.lo, x.hi, x.min_sep), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d k %d thr %#x lo %d hi %d min_sep %d in %#llx out %#llx count %#llx: %d, want %d\n", x.field,
                x.rows, x.k, x.thr, x.lo, x.hi, x.min_sep, (unsigned long long)x.in, (unsigned long long)x.out,
                (unsigned long long)x.count, got, exp);
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
    if (in_bytes(1, 8) != 1048576 || out_bytes(8, 8) != 512 || count_bytes(8) != 32 || in_bytes(0, 3) != 196608 ||
        out_bytes(3, 32) != 768 || count_bytes(3) != 12 || in_bytes(2, 1) != 131072 || out_bytes(1, 1) != 8) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_peaks_last_error(), "") != 0) {         // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    // the scalar arguments, each alone and with the pointers wrong too
    static const int fields[] = {0, 1, 2, -1, 3};
    static const int ks[] = {1, 8, 32, 0, 33, -1};
    static const uint32_t thrs[] = {0u, 1u, 0x3F800000u, 0x7F800000u, 0x7F800001u, 0x7FC00000u, 0x80000000u, 0xBF800000u, 0xFFFFFFFFu};
    static const int ranges[][2] = {{0, 16384}, {0, 1}, {16383, 16384}, {5, 5}, {6, 5}, {-1, 5}, {0, 16385}, {16384, 16385}};
    static const int seps[] = {1, 2, 16384, 0, -1, 16385};
    static const int rowss[] = {0, 1, 3, 8, 4096, 70000, 16777216, 2147483647, -1, -2147483647 - 1};
    for (int field : fields)
        for (int k : ks)
            for (uint32_t thr : thrs)
                for (auto &rg : ranges)
                    for (int sep : seps)
                        for (int rows : rowss) {
                            if (check({field, far, 1ull << 62, 1ull << 61, rows, k, thr, rg[0], rg[1], sep})) return 1;
                            if (check({field, 0, 0, 0, rows, k, thr, rg[0], rg[1], sep})) return 1;
                            if (check({field, far + 1, far + 3, far + 2, rows, k, thr, rg[0], rg[1], sep})) return 1;
                        }
    // the pointers: every pair of ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, far apart; every alignment
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, 0xFFFF000000000000ull, 0xFFFFFFFFFFFF0000ull, 16};
    static const int rows2[] = {1, 3, 5, 8, 4096, 70000, 16777215, 2147483647};
    for (int field = 0; field < 3; ++field)
        for (int k : {1, 7, 32})
            for (int rows : rows2) {
                const u128 n[3] = {in_bytes(field, rows), out_bytes(rows, k), count_bytes(rows)};
                for (uint64_t base : bases)
                    for (int a = 0; a < 3; ++a)                    // range a at `base`, range b placed against it, the third far off
                        for (int b = 0; b < 3; ++b) {
                            if (a == b) continue;
                            const int c = 3 - a - b;
                            const uint64_t na = (uint64_t)n[a], nb = (uint64_t)n[b];
                            const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16,
                                                      base + na + 16, base - nb, base - nb + 1, base - nb + 4, base - nb + 8,
                                                      base - nb + 16, base - nb - 16, base, base + 8, base + 16,
                                                      base + (1ull << 31), base - (1ull << 31)};
                            for (uint64_t spot : spots) {
                                uint64_t p[3];
                                p[a] = base, p[b] = spot;
                                p[c] = base < (1ull << 63) ? 0xC000000000000000ull : 1ull << 40;
                                if (spot == 0 || !fits(p[a], n[a]) || !fits(p[b], n[b]) || !fits(p[c], n[c])) continue;
                                if (check({field, p[0], p[1], p[2], rows, k, 0u, 0, 16384, 1})) return 1;
                            }
                        }
                // alignment: in 16, out 8, count 4
                for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                    if (check({field, far + off, 1ull << 62, 1ull << 61, rows, k, 0u, 0, 16384, 1})) return 1;
                    if (check({field, far, (1ull << 62) + off, 1ull << 61, rows, k, 0u, 0, 16384, 1})) return 1;
                    if (check({field, far, 1ull << 62, (1ull << 61) + off, rows, k, 0u, 0, 16384, 1})) return 1;
                }
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
