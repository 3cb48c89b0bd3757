// Stand-alone host test of the argument and pointer check of sa_rank_f32 (include/specan_rank.h; sa_rank_check in
// csrc/sa_rank_check.cpp).  No GPU, no library: compiled together with sa_rank_check.cpp by tests/test_f32_rank_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic or a read
// beyond the q ranks given is an error they report: every array of ranks here is allocated at exactly its q entries).  The
// expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to 2^31 - 1 and
// addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/specan_rank.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, out;
    int rows, q;
    const int32_t *ranks;                                      // null, or as many entries as a q in 1..8 says (8 otherwise)
    int lo, hi;
};

static u128 in_bytes(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 out_bytes(int rows, int q)
{
    return (u128)rows * (u128)q * 4;
}

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return a < b + nb && b < a + na;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2 || x.q < 1 || x.q > 8) return SA_EINVAL;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384)) return SA_EINVAL;
    if (!x.ranks) return SA_EINVAL;
    for (int j = 0; j < x.q; ++j)
        if (x.ranks[j] < 0 || (int64_t)x.ranks[j] >= (int64_t)x.hi - x.lo) return SA_EINVAL;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0 || x.in % 16 || x.out % 4) return SA_EINVAL;
    return meet(x.in, in_bytes(x.field, x.rows), x.out, out_bytes(x.rows, x.q)) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_rank_check(x.field, x.in, x.out, x.rows, x.q, x.ranks, x.lo, x.hi), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d q %d lo %d hi %d in %#llx out %#llx ranks %s: %d, want %d\n", x.field, x.rows, x.q, x.lo,
                x.hi, (unsigned long long)x.in, (unsigned long long)x.out, x.ranks ? "given" : "NULL", got, exp);
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
    if (in_bytes(0, 3) != 196608 || out_bytes(3, 8) != 96 || in_bytes(2, 1) != 131072 || out_bytes(1, 1) != 4 ||
        in_bytes(1, 8) != 1048576 || out_bytes(8, 2) != 64) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_rank_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    // the scalar arguments and the ranks, each alone and with the pointers wrong too.  A rank set is described by a fill
    // value relative to the range and the slot that holds it; the other slots are 0.
    static const int fields[] = {0, 1, 2, -1, 3};
    static const int qs[] = {1, 2, 8, 0, 9, -1};
    static const int ranges[][2] = {{0, 16384}, {0, 1}, {16383, 16384}, {100, 102}, {5, 5}, {6, 5}, {-1, 5}, {0, 16385}, {16384, 16385}};
    static const int rowss[] = {0, 1, 3, 8, 4096, 70000, 16777216, 2147483647, -1, -2147483647 - 1};
    enum { ZERO, LAST, WIDTH, MINUS1, BIG, MIN, NONE, KINDS };    // a rank of 0, m - 1, m, -1, INT32_MAX, INT32_MIN; a null array
    for (int field : fields)
        for (int q : qs)
            for (auto &rg : ranges)
                for (int kind = 0; kind < KINDS; ++kind)
                    for (int slot : {0, 7}) {
                        const int n = q >= 1 && q <= 8 ? q : 8;
                        if (slot >= n && slot != 0) continue;
                        const int64_t m = (int64_t)rg[1] - rg[0];
                        const int64_t v = kind == ZERO ? 0 : kind == LAST ? (m > 0 ? m - 1 : 0) : kind == WIDTH ? (m > 0 ? m : 0)
                                        : kind == MINUS1 ? -1 : kind == BIG ? 2147483647 : -2147483647 - 1;
                        std::vector<int32_t> held((size_t)n, 0);                       // exactly n entries: a read past q is reported
                        held[(size_t)(slot < n ? slot : 0)] = (int32_t)v;
                        const int32_t *ranks = kind == NONE ? nullptr : held.data();
                        for (int rows : rowss) {
                            if (check({field, far, 1ull << 62, rows, q, ranks, rg[0], rg[1]})) return 1;
                            if (check({field, 0, 0, rows, q, ranks, rg[0], rg[1]})) return 1;
                            if (check({field, far + 1, far + 3, rows, q, ranks, rg[0], rg[1]})) return 1;
                            if (check({field, far, far, rows, q, ranks, rg[0], rg[1]})) return 1;
                        }
                    }
    // the pointers: the two ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, far apart; every alignment
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, 0xFFFF000000000000ull, 0xFFFFFFFFFFFF0000ull, 16};
    static const int rows2[] = {1, 3, 5, 8, 4096, 70000, 16777215, 2147483647};
    static const int32_t good[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int field = 0; field < 3; ++field)
        for (int q : {1, 3, 8})
            for (int rows : rows2) {
                const u128 n[2] = {in_bytes(field, rows), out_bytes(rows, q)};
                for (uint64_t base : bases)
                    for (int a = 0; a < 2; ++a) {                  // range a at `base`, range b placed against it
                        const int b = 1 - a;
                        const uint64_t na = (uint64_t)n[a], nb = (uint64_t)n[b];
                        const uint64_t spots[] = {base + na, base + na - 1, base + na - 4, base + na - 8, base + na - 16,
                                                  base + na + 16, base - nb, base - nb + 1, base - nb + 4, base - nb + 8,
                                                  base - nb + 16, base - nb - 16, base, base + 4, base + 16,
                                                  base + (1ull << 31), base - (1ull << 31)};
                        for (uint64_t spot : spots) {
                            uint64_t p[2];
                            p[a] = base, p[b] = spot;
                            if (spot == 0 || !fits(p[a], n[a]) || !fits(p[b], n[b])) continue;
                            if (check({field, p[0], p[1], rows, q, good, 0, 16384})) return 1;
                        }
                    }
                // alignment: in 16, out 4
                for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                    if (check({field, far + off, 1ull << 62, rows, q, good, 0, 16384})) return 1;
                    if (check({field, far, (1ull << 62) + off, rows, q, good, 0, 16384})) return 1;
                }
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
