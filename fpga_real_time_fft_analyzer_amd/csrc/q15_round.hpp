// q15_round.hpp -- the one rounding of the grouped trace (SA_Q15_TRACE_AVG_KIND of include/specan.h): an exact unsigned
// integer, here a power sum of up to 2^44, to the bits of the float32 nearest to it, ties to even.  Plain integer
// arithmetic on host and device alike (no float conversion whose rounding mode one would have to trust, no device
// intrinsic): the fold kernel (trace_fold_q15.hip) calls it, and tests/cpp/test_q15_round.cpp runs it on the host
// against the compiler's own (float) of the same integer.  Valid for every v below 2^64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SA_Q15_ROUND_FN __host__ __device__ inline
#else
#define SA_Q15_ROUND_FN inline
#endif

SA_Q15_ROUND_FN uint32_t sa_u64_to_f32_bits_rn(uint64_t v)
{
    if (v == 0) return 0u;                                       // +0.0f
    const int msb = 63 - __builtin_clzll(v);                     // v in [2^msb, 2^(msb+1))
    if (msb <= 23)                                               // at most 24 significant bits: exact
        return (uint32_t)(127 + msb) << 23 | ((uint32_t)v << (23 - msb) & 0x7FFFFFu);
    const int sh = msb - 23;                                     // bits dropped: 1..40
    uint64_t m = v >> sh;                                        // the 24-bit significand, truncated
    const uint64_t rem = v & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (m & 1))) ++m;             // nearest; a tie to the even significand
    // m = 2^24 (a carry into the next binade) adds one to the exponent field and leaves a zero fraction
    return ((uint32_t)(127 + msb) << 23) + (uint32_t)(m - (1u << 23));
}
