// Stand-alone host test of the argument and pointer check of sa_bands_f32 (include/specan_bands.h; sa_bands_check in
// csrc/sa_bands_check.cpp).  No GPU, no library: compiled together with sa_bands_check.cpp by tests/test_f32_bands_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic or a read
// beyond the nb bands or nq fractions given is an error they report: every array here is allocated at exactly its count).
// The expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to 2^31 - 1 and
// addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/specan_bands.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, power, cross;
    int rows, nb;
    const sa_band *bands;                                      // null, or as many entries as an nb in 1..16 says (1 otherwise)
    int nq;
    const double *fracs;                                       // null, or as many entries as an nq in 1..4 says (1 otherwise)
};

static u128 in_bytes(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 power_bytes(int rows, int nb)
{
    return (u128)rows * (u128)nb * 8;
}

static u128 cross_bytes(int rows, int nb, int nq)
{
    return (u128)rows * (u128)nb * (u128)nq * 4;
}

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return na > 0 && nb > 0 && a < b + nb && b < a + na;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2 || x.nb < 1 || x.nb > 16) return SA_EINVAL;
    if (!x.bands) return SA_EINVAL;
    for (int j = 0; j < x.nb; ++j)
        if (!(0 <= x.bands[j].lo && x.bands[j].lo < x.bands[j].hi && x.bands[j].hi <= 16384)) return SA_EINVAL;
    if (x.nq < 0 || x.nq > 4) return SA_EINVAL;
    if (x.nq > 0 && !x.fracs) return SA_EINVAL;
    for (int q = 0; q < x.nq; ++q)
        if (std::isnan(x.fracs[q]) || x.fracs[q] < 0.0 || x.fracs[q] > 1.0 - std::ldexp(1.0, -32)) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.power == 0 || x.in % 16 || x.power % 8) return SA_EINVAL;
    if (x.nq > 0 && (x.cross == 0 || x.cross % 4)) return SA_EINVAL;
    const u128 ni = in_bytes(x.field, x.rows), np = power_bytes(x.rows, x.nb), nc = cross_bytes(x.rows, x.nb, x.nq);
    return meet(x.in, ni, x.power, np) || meet(x.in, ni, x.cross, nc) || meet(x.power, np, x.cross, nc) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_bands_check(x.field, x.in, x.power, x.cross, x.rows, x.nb, x.bands, x.nq, x.fracs), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d nb %d nq %d in %#llx power %#llx cross %#llx bands %s fracs %s: %d, want %d\n", x.field,
                x.rows, x.nb, x.nq, (unsigned long long)x.in, (unsigned long long)x.power, (unsigned long long)x.cross,
                x.bands ? "given" : "NULL", x.fracs ? "given" : "NULL", got, exp);
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
    if (in_bytes(0, 3) != 196608 || power_bytes(3, 2) != 48 || cross_bytes(3, 2, 2) != 48 || in_bytes(2, 1) != 131072 ||
        power_bytes(1, 16) != 128 || cross_bytes(1, 16, 0) != 0) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_bands_last_error(), "") != 0) {         // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double top = 1.0 - std::ldexp(1.0, -32);
    // the scalar arguments, the bands and the fractions, each alone and with the pointers wrong too.  A band set is one band
    // in the last slot (or slot 0) among full-width ones; a fraction set one value in the last slot among 0.5s.
    static const int fields[] = {0, 1, 2, -1, 3};
    static const int nbs[] = {1, 2, 16, 0, 17, -1};
    static const int nqs[] = {0, 1, 4, -1, 5};
    static const int ranges[][2] = {{0, 16384}, {0, 1}, {16383, 16384}, {5, 5}, {6, 5}, {-1, 5}, {0, 16385}, {16384, 16385},
                                    {-2147483647 - 1, 2147483647}};
    const double values[] = {0.5, 0.0, top, std::nextafter(top, 2.0), 1.0, -std::numeric_limits<double>::denorm_min(), -0.0, nan, inf, -inf};
    static const int rowss[] = {0, 1, 3, 4096, 16777216, 2147483647, -1, -2147483647 - 1};
    for (int field : fields)
        for (int nb : nbs)
            for (int nq : nqs)
                for (auto &rg : ranges)
                    for (int slot : {0, 15})
                        for (int bnull = 0; bnull < 2; ++bnull)
                            for (size_t vi = 0; vi <= sizeof values / sizeof values[0]; ++vi) {       // the last one: a null array
                                const int n = nb >= 1 && nb <= 16 ? nb : 1, m = nq >= 1 && nq <= 4 ? nq : 1;
                                if (slot >= n && slot != 0) continue;
                                if (bnull && (slot || vi)) continue;
                                std::vector<sa_band> held((size_t)n, sa_band{0, 16384});       // exactly n entries: a read past nb is reported
                                held[(size_t)slot] = sa_band{rg[0], rg[1]};
                                std::vector<double> fr((size_t)m, 0.5);                        // exactly m entries
                                const bool fnull = vi == sizeof values / sizeof values[0];
                                if (!fnull) fr[(size_t)(m - 1)] = values[vi];
                                const sa_band *bands = bnull ? nullptr : held.data();
                                const double *fracs = fnull ? nullptr : fr.data();
                                for (int rows : rowss) {
                                    if (check({field, far, 1ull << 62, 1ull << 63, rows, nb, bands, nq, fracs})) return 1;
                                    if (check({field, 0, 0, 0, rows, nb, bands, nq, fracs})) return 1;
                                    if (check({field, far + 1, far + 3, far + 2, rows, nb, bands, nq, fracs})) return 1;
                                    if (check({field, far, far, far, rows, nb, bands, nq, fracs})) return 1;
                                }
                            }
    // the pointers: each pair of ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, far apart, the third range
    // out of the way; every alignment
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, 0xFFFF000000000000ull, 0xFFFFFFFFFFFF0000ull, 4096};
    static const int rows2[] = {1, 3, 5, 4096, 70000, 16777215, 2147483647};
    static const sa_band good[16] = {{0, 16384}, {0, 1}, {5, 9}, {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384},
                                     {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384}, {0, 16384}, {16383, 16384}};
    static const double half[4] = {0.5, 0.005, 0.995, 0.0};
    const uint64_t away[3] = {1ull << 60, 1ull << 61, 3ull << 60};                             // 2^48 bytes fit between them
    for (int field = 0; field < 3; ++field)
        for (int nb : {1, 3, 16})
            for (int nq : {0, 1, 4})
                for (int rows : rows2) {
                    const u128 n[3] = {in_bytes(field, rows), power_bytes(rows, nb), cross_bytes(rows, nb, nq)};
                    for (uint64_t base : bases)
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b) {              // range a at `base`, range b placed against it
                                if (a == b) continue;
                                const int c = 3 - a - b;
                                const uint64_t na = (uint64_t)n[a], nbb = (uint64_t)n[b];
                                const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16,
                                                          base + na + 16, base - nbb, base - nbb + 1, base - nbb + 4, base - nbb + 8,
                                                          base - nbb + 16, base - nbb - 16, base, base + 4, base + 16,
                                                          base + (1ull << 31), base - (1ull << 31)};
                                for (uint64_t spot : spots) {
                                    uint64_t p[3];
                                    p[a] = base, p[b] = spot, p[c] = away[c];
                                    if (spot == 0 || !fits(p[a], n[a]) || !fits(p[b], n[b])) continue;
                                    if (check({field, p[0], p[1], p[2], rows, nb, good, nq, half})) return 1;
                                }
                            }
                    // alignment: in 16, power 8, cross 4
                    for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                        if (check({field, far + off, away[1], away[2], rows, nb, good, nq, half})) return 1;
                        if (check({field, far, away[1] + off, away[2], rows, nb, good, nq, half})) return 1;
                        if (check({field, far, away[1], away[2] + off, rows, nb, good, nq, half})) return 1;
                    }
                }
    std::printf("ok %d\n", g_checks);
    return 0;
}
