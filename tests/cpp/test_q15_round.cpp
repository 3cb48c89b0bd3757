// Stand-alone host test of the grouped trace's one rounding (csrc/q15_round.hpp: an exact integer power sum of up to 2^44
// to the bits of the nearest float32, ties to even, in plain integer arithmetic -- the function the fold kernel of
// SA_Q15_TRACE_AVG_KIND calls on the device).  No GPU, no library: compiled by tests/test_q15_trace_avg_cpu.py, under the
// address and undefined-behaviour sanitizers where they link.  The reference is the compiler's own (float) of the same
// uint64_t on the host (IEEE round to nearest even).  Prints "ok <values checked>" and returns 0, or names the first value
// that differs and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../fpga_real_time_fft_analyzer_amd/csrc/q15_round.hpp"

static unsigned long long g_values = 0;

static uint32_t host_bits(uint64_t v)
{
    const float f = (float)v;
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

static bool same(uint64_t v)
{
    ++g_values;
    const uint32_t got = sa_u64_to_f32_bits_rn(v), want = host_bits(v);
    if (got == want) return true;
    std::printf("FAILED v = %llu (0x%llx): got 0x%08x, (float) gives 0x%08x\n", (unsigned long long)v, (unsigned long long)v, got, want);
    return false;
}

int main()
{
    // the values named one by one
    for (uint64_t v : {0ull, 1ull, 2ull, 3ull, 1ull << 23, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1, (1ull << 24) + 2,
                       (1ull << 24) + 3, 1ull << 32, 1ull << 36, (1ull << 44) - 1, 1ull << 44, (1ull << 44) + 1})
        if (!same(v)) return 1;
    // known answers, written out: 2^24 + 1 ties to the even 2^24, 2^24 + 3 to 2^24 + 4; 2^44 is 0x55800000
    if (sa_u64_to_f32_bits_rn((1ull << 24) + 1) != 0x4B800000u || sa_u64_to_f32_bits_rn((1ull << 24) + 3) != 0x4B800002u ||
        sa_u64_to_f32_bits_rn(1ull << 44) != 0x55800000u || sa_u64_to_f32_bits_rn(0) != 0u || sa_u64_to_f32_bits_rn(1) != 0x3F800000u) {
        std::printf("FAILED known answers\n");
        return 1;
    }
    // every exact tie and its two neighbours, for each shift 1..20 (the bits dropped), at the smallest significand, the
    // next one (odd: the tie goes up) and the largest (the tie carries into the next binade)
    for (int sh = 1; sh <= 20; ++sh)
        for (uint64_t m : {1ull << 23, (1ull << 23) + 1, (1ull << 24) - 1}) {
            const uint64_t tie = (m << sh) + (1ull << (sh - 1));
            if (!same(tie - 1) || !same(tie) || !same(tie + 1)) return 1;
            if (!same(m << sh) || !same(((m + 1) << sh) - 1)) return 1;          // the ends of the interval between two floats
        }
    // carries into the next binade: 2^k - 1 and its neighbours, k = 25..44
    for (int k = 25; k <= 44; ++k)
        for (int d = -2; d <= 1; ++d)
            if (!same((1ull << k) - 1 + (uint64_t)(int64_t)d)) return 1;
    // everything below 2^25 + 2^16: the exact range, and the first binade that rounds, whole
    for (uint64_t v = 0; v < (1ull << 25) + (1ull << 16); v += 1)
        if (sa_u64_to_f32_bits_rn(v) != host_bits(v)) {
            same(v);
            return 1;
        }
    g_values += (1ull << 25) + (1ull << 16);
    // 2^20 seeded random values below 2^44 (a 64-bit linear congruential sequence, top bits), with every width of leading
    // zeros, and for each one the tie nearest below it
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < (1 << 20); ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const int width = 1 + (int)((x >> 58) % 44);                         // 1..44 significant bits
        const uint64_t v = (x >> 8) & ((1ull << width) - 1);
        if (!same(v)) return 1;
        if (width > 25) {
            const int sh = width - 24;
            const uint64_t tie = (v >> sh << sh) | 1ull << (sh - 1);
            if (!same(tie)) return 1;
        }
    }
    std::printf("ok %llu\n", g_values);
    return 0;
}
