// Stand-alone host test of the argument and pointer check of sa_hist_f32 (include/specan_hist.h; sa_hist_check in
// csrc/sa_hist_check.cpp).  No GPU, no library: compiled together with sa_hist_check.cpp by tests/test_f32_hist_cpu.py,
// under the address and undefined-behaviour sanitizers where they link (a signed overflow in the byte arithmetic or a read
// beyond the L - 1 edges given is an error they report: every array of edges here is allocated at exactly its L - 1
// entries).  The expected answer is this file's own evaluation of the header's rules in 128-bit integers, at rows up to
// 2^31 - 1, groups up to 2^24 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names the first
// failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/specan_hist.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

struct Args {
    uint64_t in, out;
    int rows, group, log2w, nlev;
    const float *edges;                                        // null, or as many entries as an nlev in 2..64 says (63 otherwise)
    int lo, hi;
};

static uint32_t bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static u128 in_bytes(int rows)
{
    return (u128)rows * 65536;
}

static u128 out_bytes(int rows, int group, int log2w, int nlev, int lo, int hi)
{
    return (u128)(rows / group) * (u128)((hi - lo) >> log2w) * (u128)nlev * 4;
}

static bool meet(u128 a, u128 na, u128 b, u128 nb)
{
    return a < b + nb && b < a + na;
}

static int want(const Args &x)
{
    if (x.rows < 0) return SA_ESHAPE;
    if (x.group < 1 || x.group > (1 << 24) || x.log2w < 0 || x.log2w > 6 || x.nlev < 2 || x.nlev > 64) return SA_EINVAL;
    const int w = 1 << x.log2w;
    if (!(0 <= x.lo && x.lo < x.hi && x.hi <= 16384) || x.lo % w || x.hi % w) return SA_EINVAL;
    if (!x.edges) return SA_EINVAL;
    for (int j = 0; j < x.nlev - 1; ++j) {
        if (bits(x.edges[j]) > 0x7F800000u) return SA_EINVAL;
        if (j && bits(x.edges[j]) < bits(x.edges[j - 1])) return SA_EINVAL;
    }
    if (x.rows % x.group) return SA_ESHAPE;
    if (x.rows == 0) return SA_OK;
    if (x.in == 0 || x.out == 0 || x.in % 16 || x.out % 4) return SA_EINVAL;
    return meet(x.in, in_bytes(x.rows), x.out, out_bytes(x.rows, x.group, x.log2w, x.nlev, x.lo, x.hi)) ? SA_EINVAL : SA_OK;
}

static int check(const Args &x)
{
    ++g_checks;
    const int got = sa_hist_check(x.in, x.out, x.rows, x.group, x.log2w, x.nlev, x.edges, x.lo, x.hi), exp = want(x);
    if (got == exp) return 0;
    std::printf("FAILED rows %d group %d log2w %d nlev %d lo %d hi %d in %#llx out %#llx edges %s: %d, want %d\n", x.rows, x.group,
                x.log2w, x.nlev, x.lo, x.hi, (unsigned long long)x.in, (unsigned long long)x.out, x.edges ? "given" : "NULL", got, exp);
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
    if (in_bytes(8) != 524288 || out_bytes(8, 4, 4, 32, 0, 16384) != 262144 || in_bytes(3) != 196608 ||
        out_bytes(3, 1, 0, 2, 16, 48) != 768) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_hist_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    const uint64_t far = (1ull << 47) - (1ull << 36);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the scalar arguments and the edges, each alone and with the pointers wrong too.  An edge set is described by a kind and
    // the slot that holds the odd value; the other slots are 1.0.
    static const int groups[] = {1, 2, 3, 16777216, 0, -1, 16777217};
    static const int log2ws[] = {0, 3, 6, -1, 7};
    static const int nlevs[] = {2, 3, 33, 64, 1, 0, 65, -1};
    static const int ranges[][2] = {{0, 16384}, {0, 64}, {16320, 16384}, {8, 16}, {1, 2}, {4, 12}, {5, 5}, {6, 5}, {-1, 5}, {0, 16385}, {16384, 16385}};
    static const int rowss[] = {0, 1, 3, 6, 4096, 16777216, 2147483647, -1, -2147483647 - 1};
    enum { GOOD, ZEROS, INF, NAN_, NEGATIVE, MINUS_ZERO, BELOW, NONE, KINDS };
    for (int group : groups)
        for (int log2w : log2ws)
            for (int nlev : nlevs)
                for (auto &rg : ranges)
                    for (int kind = 0; kind < KINDS; ++kind)
                        for (int slot : {0, 62}) {
                            const int n = nlev >= 2 && nlev <= 64 ? nlev - 1 : 63;
                            if (slot >= n && slot != 0) continue;
                            std::vector<float> held((size_t)n, kind == ZEROS ? 0.0f : 1.0f);     // exactly n entries: a read past L - 1 is reported
                            float &odd = held[(size_t)slot];
                            if (kind == INF) {
                                for (int j = slot; j < n; ++j) held[(size_t)j] = inf;
                            } else if (kind == NAN_) {
                                odd = nan;
                            } else if (kind == NEGATIVE) {
                                odd = -1.0f;
                            } else if (kind == MINUS_ZERO) {
                                odd = -0.0f;
                            } else if (kind == BELOW) {
                                odd = 0.5f;                    // below the 1.0 before it, unless it is the first
                            }
                            const float *edges = kind == NONE ? nullptr : held.data();
                            for (int rows : rowss) {
                                if (check({far, 1ull << 62, rows, group, log2w, nlev, edges, rg[0], rg[1]})) return 1;
                                if (check({0, 0, rows, group, log2w, nlev, edges, rg[0], rg[1]})) return 1;
                                if (check({far + 1, far + 3, rows, group, log2w, nlev, edges, rg[0], rg[1]})) return 1;
                                if (check({far, far, rows, group, log2w, nlev, edges, rg[0], rg[1]})) return 1;
                            }
                        }
    // the pointers: the two ranges touching, overlapping by 1, 4, 8 and 16 bytes, contained, far apart; every alignment
    static const uint64_t bases[] = {far, (1ull << 47) - 65536, 1ull << 36, 0xFFFF000000000000ull, 0xFFFFFFFFFFFF0000ull, 16};
    static const int shapes[][2] = {{1, 1}, {3, 1}, {6, 3}, {4096, 4096}, {4096, 16}, {70000, 1}, {16777216, 16777216}, {33554432, 16777216},
                                    {2147483647, 1}, {2147483646, 2}};
    for (auto &sh : shapes)
        for (int log2w : {0, 4, 6})
            for (int nlev : {2, 33, 64}) {
                const int rows = sh[0], group = sh[1];
                if (group > 16777216 || rows % group) continue;
                const std::vector<float> e((size_t)nlev - 1, 1.0f);
                const u128 n[2] = {in_bytes(rows), out_bytes(rows, group, log2w, nlev, 0, 16384)};
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
                            if (check({p[0], p[1], rows, group, log2w, nlev, e.data(), 0, 16384})) return 1;
                        }
                    }
                // alignment: in 16, out 4
                for (uint64_t off : {1, 2, 4, 8, 12, 16}) {
                    if (check({far + off, 1ull << 62, rows, group, log2w, nlev, e.data(), 0, 16384})) return 1;
                    if (check({far, (1ull << 62) + off, rows, group, log2w, nlev, e.data(), 0, 16384})) return 1;
                }
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
