// spectra_fold_q15.hip -- the fold of sa_spectra_q15 / sa_spectra_q15_p12 / sa_fold_iq_q15 (include/specan_ext.h, DESIGN.md
// section 4.14): int16 (re, im) frames [B,16384,2], the wire frames of SA_Q15_OUT_IQ, folded A = 2^a frames at a time and bin
// by bin into sa_trace_point_q15 [B / A, 16384].  The 4-byte IQ word of a bin holds everything its record needs -- s =
// fl(fl(re re) + fl(im im)), whose largest value over the group goes under ONE correctly rounded root, and the exact integer
// re^2 + im^2, whose 64-bit sum over the group (at most 128 x 2^31 = 2^38) gets ONE rounding -- so there are no partial
// records.  One thread owns four adjacent bins of one group: one 16-byte load per frame, adjacent threads adjacent 16 bytes
// (1 KiB per wave instruction), frames 64 KiB apart; two 16-byte stores at the end.  Where the frames come from an FFT
// launch, the kernel boundary behind it on the same stream is the only synchronisation: no flags, no atomics, no LDS, no
// barrier, and no thread reads what another thread of this launch wrote.
#include "q15_dev.hpp"
#include "q15_round.hpp"
#include "../../include/specan_ext.h"

namespace {

constexpr int kFoldThreads = 256;
constexpr int kLog2Quads = 12;                                       // 16-byte quads of bins per frame: 4096
static_assert(SA_NPTS == 4 << kLog2Quads && sizeof(sa_trace_point_q15) == 8, "four bins per thread, two records per store");

// one frame's word of one bin into the bin's running maximum (float bits of a sum >= 0: ordered as unsigned) and power sum;
// re^2 + im^2 reaches 2^31 at (-32768, -32768): the dot product's 32-bit result is read as unsigned
__device__ __forceinline__ void fold_bin(unsigned w, unsigned &s, unsigned long long &pw)
{
    const unsigned b = __builtin_bit_cast(unsigned, fx_mag_sum(w));
    s = s > b ? s : b;
    pw += (unsigned)fx_dot2(w, w);
}

__device__ __forceinline__ void fold_quad(const uint4 &r, unsigned (&s)[4], unsigned long long (&pw)[4])
{
    fold_bin(r.x, s[0], pw[0]);
    fold_bin(r.y, s[1], pw[1]);
    fold_bin(r.z, s[2], pw[2]);
    fold_bin(r.w, s[3], pw[3]);
}

// `quads` = (B / A) 4096 threads' worth of output; groupsize = A, a power of two from 2 on.  Every offset is a size_t: frame
// 65536 of `iq` starts at byte 2^32, so a batch of 65537 frames reads beyond it, and row 32768 of `out` (131072 bytes a row)
// does, so B / A = 32769 rows write beyond it; tests/test_gpu_offsets.py goes there.
__global__ __launch_bounds__(kFoldThreads) void spectra_fold_q15_kernel(const uint4 *__restrict__ iq, uint4 *__restrict__ out,
                                                                       size_t quads, int groupsize)
{
    const size_t idx = (size_t)blockIdx.x * kFoldThreads + threadIdx.x;
    if (idx >= quads) return;                                    // the tail of the last workgroup
    constexpr size_t Q = (size_t)1 << kLog2Quads;
    const size_t g = idx >> kLog2Quads, j = idx & (Q - 1);
    const uint4 *src = iq + g * (size_t)groupsize * Q + j;        // quad j of frame g A; frame g A + i is i Q further
    unsigned s[4] = {0u, 0u, 0u, 0u};
    unsigned long long pw[4] = {0ull, 0ull, 0ull, 0ull};
    int i = 0;
    for (; i + 4 <= groupsize; i += 4) {                         // four loads in flight
        const uint4 r0 = src[(size_t)i * Q], r1 = src[(size_t)(i + 1) * Q], r2 = src[(size_t)(i + 2) * Q],
                    r3 = src[(size_t)(i + 3) * Q];
        fold_quad(r0, s, pw);
        fold_quad(r1, s, pw);
        fold_quad(r2, s, pw);
        fold_quad(r3, s, pw);
    }
    if (i < groupsize) {                                         // A = 2 (groupsize is a power of two): both loads in flight
        const uint4 r0 = src[(size_t)i * Q], r1 = src[(size_t)(i + 1) * Q];
        fold_quad(r0, s, pw);
        fold_quad(r1, s, pw);
    }
    unsigned rec[8];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        rec[2 * b] = __builtin_bit_cast(unsigned, fx_sqrt_rn(__builtin_bit_cast(float, s[b])));
        rec[2 * b + 1] = sa_u64_to_f32_bits_rn(pw[b]);
    }
    out[2 * idx] = make_uint4(rec[0], rec[1], rec[2], rec[3]);    // records 4 idx .. 4 idx + 3: row g, bins 4 j .. 4 j + 3
    out[2 * idx + 1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
}

}  // namespace

hipError_t sa_launch_spectra_fold_q15(const void *iq, void *out, int batch, int log2a, hipStream_t stream, SaLaunchEv ev)
{
    if (log2a < SA_Q15_TRACE_LOG2A_MIN || log2a > SA_Q15_TRACE_LOG2A_MAX || batch < 0 || (batch & ((1 << log2a) - 1)) != 0)
        return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const size_t quads = (size_t)(batch >> log2a) << kLog2Quads;
    const size_t blocks = (quads + kFoldThreads - 1) / kFoldThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(spectra_fold_q15_kernel, dim3((unsigned)blocks), dim3(kFoldThreads), 0, stream, ev.start, ev.stop, 0,
                          static_cast<const uint4 *>(iq), static_cast<uint4 *>(out), quads, 1 << log2a);
    return hipGetLastError();
}
