// Stand-alone host test of the argument and pointer check of sa_hold_f32 (include/specan_hold.h; sa_hold_check in
// csrc/sa_hold_check.cpp).  No GPU, no library: compiled together with sa_hold_check.cpp by tests/test_f32_hold_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic or a read
// beyond the q ranks given is an error they report: every array of ranks here is allocated at exactly its q entries).  The
// expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to 2^31 - 2 and
// addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/specan_hold.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    int field;
    uint64_t in, out;
    int rows, group, q;
    const int32_t *ranks;                                      // null, or as many entries as a q in 1..8 says (8 otherwise)
};

static u128 in_bytes(int field, int rows)
{
    return (u128)rows * 65536 * (field ? 2 : 1);
}

static u128 out_bytes(int rows, int group, int q)
{
    return (u128)(rows / group) * (u128)q * 65536;
}

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return a < b + nb && b < a + na;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.field < 0 || x.field > 2 || x.group < 2 || x.group > 128 || x.q < 1 || x.q > 8) return SA_EINVAL;
    if (!x.ranks) return SA_EINVAL;
    for (int j = 0; j < x.q; ++j)
        if (x.ranks[j] < 0 || x.ranks[j] >= x.group) return SA_EINVAL;
    if (x.rows % x.group) return SA_ESHAPE;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0 || x.in % 16 || x.out % 16) return SA_EINVAL;
    return meet(x.in, in_bytes(x.field, x.rows), x.out, out_bytes(x.rows, x.group, x.q)) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_hold_check(x.field, x.in, x.out, x.rows, x.group, x.q, x.ranks), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED field %d rows %d group %d q %d in %#llx out %#llx ranks %s: %d, want %d\n", x.field, x.rows, x.group, x.q,
                (unsigned long long)x.in, (unsigned long long)x.out, x.ranks ? "given" : "NULL", got, exp);
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
    if (in_bytes(0, 6) != 393216 || out_bytes(6, 3, 8) != 1048576 || in_bytes(2, 2) != 262144 || out_bytes(2, 2, 1) != 65536 ||
        in_bytes(1, 256) != 33554432 || out_bytes(256, 128, 2) != 262144) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_hold_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    // the scalar arguments and the ranks, each alone and with the pointers wrong too.  A rank set is described by a fill
    // value relative to the group and the slot that holds it; the other slots are 0.
    static const int fields[] = {0, 1, 2, -1, 3};
    static const int qs[] = {1, 2, 8, 0, 9, -1};
    static const int groups[] = {2, 3, 5, 8, 9, 127, 128, 1, 0, -1, 129, 2147483647, -2147483647 - 1};
    static const int rowss[] = {0, 1, 2, 3, 6, 10, 127, 128, 254, 256, 4096, 70000, 16777216, 2147483646, 2147483647, -1,
                                -2147483647 - 1};
    enum { ZERO, LAST, WIDTH, MINUS1, BIG, MIN, NONE, KINDS };    // a rank of 0, A - 1, A, -1, INT32_MAX, INT32_MIN; a null array
    for (int field : fields)
        for (int q : qs)
            for (int group : groups)
                for (int kind = 0; kind < KINDS; ++kind)
                    for (int slot : {0, 7}) {
                        const int n = q >= 1 && q <= 8 ? q : 8;
                        if (slot >= n && slot != 0) continue;
                        const int64_t m = group;
                        const int64_t v = kind == ZERO ? 0 : kind == LAST ? (m > 0 ? m - 1 : 0) : kind == WIDTH ? (m > 0 ? m : 0)
                                        : kind == MINUS1 ? -1 : kind == BIG ? 2147483647 : -2147483647 - 1;
                        std::vector<int32_t> held((size_t)n, 0);                       // exactly n entries: a read past q is reported
                        held[(size_t)(slot < n ? slot : 0)] = (int32_t)v;
                        const int32_t *ranks = kind == NONE ? nullptr : held.data();
                        for (int rows : rowss) {
                            if (check({field, far, 1ull << 62, rows, group, q, ranks})) return 1;
                            if (check({field, 0, 0, rows, group, q, ranks})) return 1;
                            if (check({field, far + 1, far + 3, rows, group, q, ranks})) return 1;
                            if (check({field, far, far, rows, group, q, ranks})) return 1;
                        }
                    }
    // the pointers: the two ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, far apart; every alignment
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 32, 0xFFFF000000000000ull, 0xFFFFFFFFFFFF0000ull, 16};
    static const int groups2[] = {2, 3, 128};
    static const int mult[] = {1, 3, 5, 4096, 70000, 16777215};   // groups of a call; and the largest rows a group allows
    static const int32_t good[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int field = 0; field < 3; ++field)
        for (int q : {1, 3, 8})
            for (int group : groups2) {
                std::vector<int> rows2;
                for (int k : mult) rows2.push_back(k * group);
                rows2.push_back(2147483646 / group * group);
                for (int rows : rows2) {
                    const u128 n[2] = {in_bytes(field, rows), out_bytes(rows, group, q)};
                    for (uint64_t base : bases)
                        for (int a = 0; a < 2; ++a) {              // range a at `base`, range b placed against it
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
                                if (check({field, p[0], p[1], rows, group, q, good})) return 1;
                            }
                        }
                    // alignment: both 16
                    for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                        if (check({field, far + off, 1ull << 62, rows, group, q, good})) return 1;
                        if (check({field, far, (1ull << 62) + off, rows, group, q, good})) return 1;
                    }
                }
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
