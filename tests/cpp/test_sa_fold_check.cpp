// Stand-alone host test of the argument and pointer check of sa_fold_mag_f32 (include/specan_fold.h; sa_fold_check in
// csrc/sa_fold_check.cpp).  No GPU, no library: compiled together with sa_fold_check.cpp by tests/test_f32_fold_cpu.py, under
// the address and undefined-behaviour sanitizers where they link (a signed overflow or an out-of-range shift in the byte
// arithmetic is an error they report).  The expected answer is this file's own evaluation of the header's rules in 128-bit
// integers, at batches up to 2^31 - 128 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names
// the first failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/specan_fold.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

static u128 in_bytes(int batch)
{
    return (u128)batch * 65536;
}

static u128 out_bytes(int log2a, int log2w, int batch)
{
    return (u128)(batch >> log2a) * (u128)(16384 >> log2w) * 8;
}

static int want(int log2a, int log2w, uint64_t in, uint64_t out, int batch)
{
    if (batch < 0) return SA_ESHAPE;
    if (log2a < 0 || log2a > 7 || log2w < 0 || log2w > 6 || (log2a == 0 && log2w == 0)) return SA_EINVAL;
    if (batch == 0) return SA_OK;
    if (batch % (1 << log2a)) return SA_ESHAPE;
    if ((u128)(batch >> log2a) * 16 > 2147483647u) return SA_ESHAPE;      // 16 workgroups per group of frames
    if (in == 0 || out == 0 || in % 16 || out % 16) return SA_EINVAL;
    const u128 n_in = in_bytes(batch), n_out = out_bytes(log2a, log2w, batch);
    return ((u128)in < (u128)out + n_out && (u128)out < (u128)in + n_in) ? SA_EINVAL : SA_OK;
}

static int check(int log2a, int log2w, uint64_t in, uint64_t out, int batch)
{
    ++g_checks;
    const int got = sa_fold_check(log2a, log2w, in, out, batch), exp = want(log2a, log2w, in, out, batch);
    if (got == exp) return 0;
    std::printf("FAILED log2a %d log2w %d batch %d in %#llx out %#llx: %d, want %d\n", log2a, log2w, batch,
                (unsigned long long)in, (unsigned long long)out, got, exp);
    return 1;
}

int main()
{
    // the header's known answers, by byte count
    if (in_bytes(8) != 524288 || out_bytes(2, 0, 8) != 262144 || out_bytes(0, 4, 8) != 65536 || out_bytes(4, 4, 16) != 8192) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    if (std::strcmp(sa_fold_last_error(), "") != 0) {          // the check alone leaves the thread's text alone
        std::printf("FAILED error text\n");
        return 1;
    }
    static const int log2as[] = {0, 1, 2, 4, 7, 8, -1};
    static const int log2ws[] = {0, 1, 2, 3, 4, 6, 7, -1};
    static const int batches[] = {0, 1, 2, 4, 8, 16, 128, 384, 69888, 70000, 70016, 134217727, 134217728, 268435456, 2147483520,
                                  3, 129, 2147483647, -1, -128};
    static const uint64_t bases[] = {(1ull << 47) - (1ull << 36), (1ull << 47) - 65536, 1ull << 32, 0xFFFFFFFFFFFF0000ull, 16};
    for (int log2a : log2as)
        for (int log2w : log2ws)
            for (int B : batches) {
                // the arguments before the addresses: with good, zero and misaligned addresses
                if (check(log2a, log2w, bases[0], bases[0] + (1ull << 46), B)) return 1;
                if (check(log2a, log2w, 0, 0, B)) return 1;
                if (check(log2a, log2w, bases[0] + 1, bases[0] + 3, B)) return 1;
                if (want(log2a, log2w, bases[0], bases[0] + (1ull << 46), B) != SA_OK || B == 0) continue;
                const u128 n_in128 = in_bytes(B), n_out128 = out_bytes(log2a, log2w, B);
                const uint64_t n_in = (uint64_t)n_in128, n_out = (uint64_t)n_out128;
                for (uint64_t in : bases) {
                    const uint64_t outs[] = {in, in + n_in, in + n_in - 1, in + n_in - 16, in + n_in + 16, in - n_out,
                                             in - n_out + 1, in - n_out + 16, in - n_out - 16, in + 1, in + 8, in + 16,
                                             in + (1ull << 32), in - (1ull << 32), in + (1ull << 31)};
                    for (uint64_t out : outs) {
                        // a range that wraps past 2^64 is outside what any address space holds: not part of the contract
                        if (out == 0 || (u128)in + n_in128 > ((u128)1 << 64) || (u128)out + n_out128 > ((u128)1 << 64)) continue;
                        if (check(log2a, log2w, in, out, B)) return 1;
                        for (uint64_t off : {1, 2, 4, 8, 12}) {
                            ++g_checks;
                            if (sa_fold_check(log2a, log2w, in + off, out, B) != SA_EINVAL) {
                                std::printf("FAILED in off by %d accepted\n", (int)off);
                                return 1;
                            }
                        }
                    }
                }
            }
    std::printf("ok %d\n", g_checks);
    return 0;
}
