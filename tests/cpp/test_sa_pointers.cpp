// Stand-alone host test of the pointer contract of the process and filter calls (csrc/sa_pointers.cpp; the contract is
// stated in include/specan.h).  No GPU, no library: compiled together with sa_pointers.cpp by
// tests/test_pointer_contract_cpu.py, under the address and undefined-behaviour sanitizers where they link (a signed
// overflow or an out-of-range shift in the byte arithmetic is an error they report).  The expected answer is this file's
// own evaluation of the contract in 128-bit integers.  Prints "ok <checks>" and returns 0, or names the first failed
// check and returns 1.
#include <cstdint>
#include <cstdio>

#include "../../include/specan.h"

static int g_checks = 0;

typedef unsigned __int128 u128;

struct Case {
    int entry, kind;
    bool hop_word;
    uint64_t in_frame;      // bytes per frame of input
    int num, den;           // bytes per sample
    uint64_t out_frame;     // bytes per frame of output
    uint64_t out_align;
};

static int want(const Case &c, int hop, int batch, uint64_t in, uint64_t out)
{
    const u128 n_in = hop ? (((u128)batch - 1) * (u128)hop + SA_N) * (u128)c.num / (u128)c.den : (u128)batch * c.in_frame;
    const u128 n_out = (u128)batch * c.out_frame;
    if (in % 16 || out % c.out_align) return SA_EINVAL;
    return ((u128)in < (u128)out + n_out && (u128)out < (u128)in + n_in) ? SA_EINVAL : SA_OK;
}

static int run(const Case &c)
{
    static const int hops[] = {0, 8, 4104, 16384};
    static const int batches[] = {1, 2, 5, 36000, 40000, 2147483647};
    static const uint64_t bases[] = {(1ull << 47) - (1ull << 36), 1ull << 32, 0xFFFFFFFFFFFF0000ull, 16};
    for (int hop : hops) {
        if (hop && !c.hop_word) continue;
        const int word = c.kind | (hop / 8) << 8;
        for (int B : batches) {
            const u128 n_in128 = hop ? (((u128)B - 1) * (u128)hop + SA_N) * (u128)c.num / (u128)c.den : (u128)B * c.in_frame;
            const uint64_t n_in = (uint64_t)n_in128, n_out = (uint64_t)B * c.out_frame;
            for (uint64_t in : bases) {
                const uint64_t outs[] = {in, in + n_in, in + n_in - 1, in + n_in - c.out_align, in - n_out, in - n_out + 1,
                                         in - n_out + c.out_align, in + 1, in + 4, in + 8, in + 12, in + 16, in + (1ull << 32),
                                         in + (1ull << 31), in - (1ull << 32), (in + n_in + 15) / 16 * 16};
                for (uint64_t out : outs) {
                    // a range that wraps past 2^64 is outside what any address space holds: not part of the contract
                    if (out == 0 || (u128)in + n_in128 > ((u128)1 << 64) || (u128)out + n_out > ((u128)1 << 64)) continue;
                    ++g_checks;
                    const int got = sa_debug_check_pointers(c.entry, word, in, out, B), exp = want(c, hop, B, in, out);
                    if (got != exp) {
                        std::printf("FAILED entry %d word %#x batch %d in %#llx out %#llx: %d, want %d\n", c.entry, word, B,
                                    (unsigned long long)in, (unsigned long long)out, got, exp);
                        return 1;
                    }
                    for (uint64_t off : {1, 2, 4, 8, 12}) {
                        ++g_checks;
                        if (sa_debug_check_pointers(c.entry, word, in + off, out, B) != SA_EINVAL) {
                            std::printf("FAILED entry %d word %#x: in off by %d accepted\n", c.entry, word, (int)off);
                            return 1;
                        }
                    }
                    ++g_checks;
                    if (sa_debug_check_pointers(c.entry, word, in + 1, out + 1, 0) != SA_OK) {
                        std::printf("FAILED entry %d word %#x: empty batch refused\n", c.entry, word);
                        return 1;
                    }
                }
            }
        }
    }
    return 0;
}

int main()
{
    const uint64_t F = 65536, I = 32768, P = SA_P12_FRAME_BYTES;
    const struct { int kind; uint64_t bytes, align; } fl[] = {{SA_OUT_MAG_FULL, 65536, 16}, {SA_OUT_MAG_HALF, 32772, 4},
                                                                {SA_OUT_SPEC_HALF, 65544, 8}, {SA_OUT_TIME, 65536, 16},
                                                                {SA_OUT_MARKER, 16, 16}};
    for (const auto &k : fl) {
        if (run({SA_ENTRY_PROCESS_F32, k.kind, false, F, 4, 1, k.bytes, k.align})) return 1;
        if (run({SA_ENTRY_PROCESS_F32_I16, k.kind, false, I, 2, 1, k.bytes, k.align})) return 1;
        if (run({SA_ENTRY_PROCESS_F32_P12, k.kind, false, P, 3, 2, k.bytes, k.align})) return 1;
    }
    for (int kind : {0, 1, 2, 17, 18, 19, 20, 21, 22}) {
        const uint64_t bytes = kind == SA_Q15_OUT_MARKER ? 16 : kind >= 17 ? (uint64_t)(SA_N >> (kind - 16)) * 8 : 65536;
        if (run({SA_ENTRY_PROCESS_Q15_OUT, kind, true, I, 2, 1, bytes, 16})) return 1;
        if (run({SA_ENTRY_PROCESS_Q15_P12, kind, true, P, 3, 2, bytes, 16})) return 1;
    }
    if (run({SA_ENTRY_PROCESS_Q15, 0, false, I, 2, 1, 65536, 16})) return 1;
    if (run({SA_ENTRY_FILTER_Q15, 0, false, I, 2, 1, 32768, 16})) return 1;
    if (run({SA_ENTRY_FILTER_Q15_P12, 0, false, P, 3, 2, 32768, 16})) return 1;
    std::printf("ok %d\n", g_checks);
    return 0;
}
