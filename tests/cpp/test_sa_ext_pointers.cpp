// Stand-alone host test of the argument and pointer checks of the calls of include/specan_ext.h (sa_ext_check_pointers in
// csrc/sa_pointers.cpp).  No GPU, no library: compiled together with sa_pointers.cpp by tests/test_q15_spectra_cpu.py, under
// the address and undefined-behaviour sanitizers where they link (a signed overflow or an out-of-range shift in the byte
// arithmetic is an error they report).  The expected answer is this file's own evaluation of the header's rules in 128-bit
// integers, at batches up to 2^31 - 128 and addresses near 2^47 and near 2^64.  Prints "ok <checks>" and returns 0, or names
// the first failed check and returns 1.
#include <cstdint>
#include <cstdio>

#include "../../include/specan_ext.h"

typedef unsigned __int128 u128;

static int g_checks = 0;

// bytes read by `entry` on `batch` frames at `hop`
static u128 in_bytes(int entry, int hop, int batch)
{
    if (entry == SA_EXT_ENTRY_FOLD_IQ_Q15) return (u128)batch * 65536;
    const int num = entry == SA_EXT_ENTRY_SPECTRA_Q15_P12 ? 3 : 2, den = entry == SA_EXT_ENTRY_SPECTRA_Q15_P12 ? 2 : 1;
    if (hop == 0) return (u128)batch * SA_N * (u128)num / (u128)den;
    return (((u128)batch - 1) * (u128)hop + SA_N) * (u128)num / (u128)den;
}

static int want(int entry, int log2a, int hop, uint64_t in, uint64_t out, int batch)
{
    if (entry < 0 || entry > 2) return SA_EINVAL;
    if (batch < 0) return SA_ESHAPE;
    if (log2a < 1 || log2a > 7) return SA_EINVAL;
    if (hop != 0 && (entry == SA_EXT_ENTRY_FOLD_IQ_Q15 || hop < 8 || hop > 16384 || hop % 8)) return SA_EINVAL;
    if (batch == 0) return SA_OK;
    if (batch % (1 << log2a)) return SA_ESHAPE;
    if (in == 0 || out == 0 || in % 16 || out % 16) return SA_EINVAL;
    const u128 n_in = in_bytes(entry, hop, batch), n_out = (u128)(batch >> log2a) * 131072;
    return ((u128)in < (u128)out + n_out && (u128)out < (u128)in + n_in) ? SA_EINVAL : SA_OK;
}

static int check(int entry, int log2a, int hop, uint64_t in, uint64_t out, int batch)
{
    ++g_checks;
    const int got = sa_ext_check_pointers(entry, log2a, hop, in, out, batch), exp = want(entry, log2a, hop, in, out, batch);
    if (got == exp) return 0;
    std::printf("FAILED entry %d log2a %d hop %d batch %d in %#llx out %#llx: %d, want %d\n", entry, log2a, hop, batch,
                (unsigned long long)in, (unsigned long long)out, got, exp);
    return 1;
}

int main()
{
    // the header's known answers, by byte count
    if (in_bytes(0, 0, 8) != 262144 || in_bytes(0, 4096, 8) != 90112 || in_bytes(1, 4096, 8) != 67584 || in_bytes(2, 0, 8) != 524288 ||
        SA_Q15_HOP_STREAM_SAMPLES(8, 4096) != 45056) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    static const int hops[] = {0, 8, 4096, 4104, 16376, 16384, -8, 4, 12, 16392, 1 << 20};
    static const int log2as[] = {1, 2, 7, 0, 8, -1};
    static const int batches[] = {0, 2, 4, 8, 128, 384, 69888, 70000, 70016, 2147483520, 1, 3, 129, 2147483647, -1, -128};
    static const uint64_t bases[] = {(1ull << 47) - (1ull << 36), (1ull << 47) - 65536, 1ull << 32, 0xFFFFFFFFFFFF0000ull, 16};
    for (int entry = -1; entry <= 3; ++entry)
        for (int log2a : log2as)
            for (int hop : hops)
                for (int B : batches) {
                    // the arguments before the addresses: with good, zero and misaligned addresses
                    if (check(entry, log2a, hop, bases[0], bases[0] + (1ull << 46), B)) return 1;
                    if (check(entry, log2a, hop, 0, 0, B)) return 1;
                    if (check(entry, log2a, hop, bases[0] + 1, bases[0] + 3, B)) return 1;
                    if (want(entry, log2a, hop, bases[0], bases[0] + (1ull << 46), B) != SA_OK || B == 0) continue;
                    const u128 n_in128 = in_bytes(entry, hop, B), n_out128 = (u128)(B >> log2a) * 131072;
                    const uint64_t n_in = (uint64_t)n_in128, n_out = (uint64_t)n_out128;
                    for (uint64_t in : bases) {
                        const uint64_t behind = (uint64_t)(((u128)in + n_in + 15) / 16 * 16);
                        const uint64_t outs[] = {in, in + n_in, in + n_in - 1, in + n_in - 16, behind, behind - 16, in - n_out,
                                                 in - n_out + 1, in - n_out + 16, in + 1, in + 8, in + 16, in + (1ull << 32),
                                                 in - (1ull << 32), in + (1ull << 31)};
                        for (uint64_t out : outs) {
                            // a range that wraps past 2^64 is outside what any address space holds: not part of the contract
                            if (out == 0 || (u128)in + n_in128 > ((u128)1 << 64) || (u128)out + n_out128 > ((u128)1 << 64)) continue;
                            if (check(entry, log2a, hop, in, out, B)) return 1;
                            for (uint64_t off : {1, 2, 4, 8, 12}) {
                                ++g_checks;
                                if (sa_ext_check_pointers(entry, log2a, hop, in + off, out, B) != SA_EINVAL) {
                                    std::printf("FAILED entry %d: in off by %d accepted\n", entry, (int)off);
                                    return 1;
                                }
                            }
                        }
                    }
                }
    std::printf("ok %d\n", g_checks);
    return 0;
}
