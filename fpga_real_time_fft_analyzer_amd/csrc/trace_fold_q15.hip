// trace_fold_q15.hip -- the second launch of SA_Q15_TRACE_AVG_KIND(k, a) (include/specan.h): the
// FFT launch in front of it (fft_q15.hip, the kFxOutTraceRaw arm) left one 16-byte partial record {s, hi, lo, 0} per frame
// and bucket in a workspace [B, P], P = 16384 >> k -- s the bits of the bucket's largest float sum fl(fl(re re) +
// fl(im im)), hi and lo the sums of the 16-bit halves of its integer powers -- and this kernel folds the A = 2^a records
// (gA + i, j), i = 0..A-1, into out[g, j]: the unsigned maximum of s and ONE root, the exact sum hi 65536 + lo (at most
// 2^44) and ONE rounding.  One thread per output point; adjacent threads read adjacent records (16-byte loads, 1 KiB per
// wave instruction) and write adjacent points (8-byte stores).  The kernel boundary behind the FFT launch on the same
// stream is the only synchronisation: no flags, no atomics, no LDS, no barrier, and no thread reads what another thread
// of this launch wrote.
#include "q15_dev.hpp"
#include "q15_round.hpp"
#include "../../include/specan.h"

namespace {

constexpr int kFoldThreads = 256;
static_assert(SA_NPTS == 1 << 14, "log2p = 14 - k");

// `points` = (B / A) P output points; log2p = 14 - k.  Every offset is a size_t: at W = 2 a frame's records are 131072
// bytes and those of frame 32768 start at byte 2^32, so a batch of 32769 frames reads beyond it (at W = 2^k: of
// 2^(14 + k) + 1); tests/test_gpu_offsets.py goes there.
__global__ __launch_bounds__(kFoldThreads) void trace_fold_q15_kernel(const uint4 *__restrict__ part, uint2 *__restrict__ out,
                                                                     size_t points, int log2p, int groupsize)
{
    const size_t idx = (size_t)blockIdx.x * kFoldThreads + threadIdx.x;
    if (idx >= points) return;                                   // the tail of the last workgroup
    const size_t P = (size_t)1 << log2p;
    const size_t g = idx >> log2p, j = idx & (P - 1);
    const uint4 *src = part + g * (size_t)groupsize * P + j;       // record (g A, j); record (g A + i, j) is i P further
    unsigned s = 0u;
    unsigned long long hi = 0ull, lo = 0ull;
    int i = 0;
    for (; i + 4 <= groupsize; i += 4) {                         // four loads in flight
        const uint4 r0 = src[(size_t)i * P], r1 = src[(size_t)(i + 1) * P], r2 = src[(size_t)(i + 2) * P],
                    r3 = src[(size_t)(i + 3) * P];
        const unsigned s01 = r0.x > r1.x ? r0.x : r1.x, s23 = r2.x > r3.x ? r2.x : r3.x;
        const unsigned s03 = s01 > s23 ? s01 : s23;
        s = s > s03 ? s : s03;
        hi += (unsigned long long)r0.y + r1.y + r2.y + r3.y;
        lo += (unsigned long long)r0.z + r1.z + r2.z + r3.z;
    }
    for (; i < groupsize; ++i) {                                 // A = 2
        const uint4 r = src[(size_t)i * P];
        s = s > r.x ? s : r.x;
        hi += r.y;
        lo += r.z;
    }
    const float peak = fx_sqrt_rn(__builtin_bit_cast(float, s));
    const unsigned power = sa_u64_to_f32_bits_rn((hi << 16) + lo);
    out[idx] = make_uint2(__builtin_bit_cast(unsigned, peak), power);
}

}  // namespace

hipError_t sa_launch_trace_fold_q15(const void *partial, void *out, int batch, int log2w, int log2a, hipStream_t stream,
                                    SaLaunchEv ev)
{
    if (log2w < SA_Q15_TRACE_LOG2W_MIN || log2w > SA_Q15_TRACE_LOG2W_MAX || log2a < SA_Q15_TRACE_LOG2A_MIN ||
        log2a > SA_Q15_TRACE_LOG2A_MAX || batch < 0 || (batch & ((1 << log2a) - 1)) != 0)
        return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const int log2p = 14 - log2w;
    const size_t points = (size_t)(batch >> log2a) << log2p;
    const size_t blocks = (points + kFoldThreads - 1) / kFoldThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(trace_fold_q15_kernel, dim3((unsigned)blocks), dim3(kFoldThreads), 0, stream, ev.start, ev.stop, 0,
                          static_cast<const uint4 *>(partial), static_cast<uint2 *>(out), points, log2p, 1 << log2a);
    return hipGetLastError();
}
