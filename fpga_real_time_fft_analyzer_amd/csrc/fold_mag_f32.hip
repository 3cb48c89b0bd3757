// fold_mag_f32.hip -- sa_fold_mag_f32 (include/specan_fold.h): float32 magnitudes [B,16384], the
// SA_OUT_MAG_FULL layout, folded A = 2^a frames at a time and W = 2^k bins at a time into sa_fold_point [B / A, 16384 / W].
// The kernel of libspecan_fold.so; it stands beside the fused float chain and shares no text with it.
//
// One thread owns four adjacent bins of one group, as spectra_fold_q15_kernel does: one 16-byte load per frame, adjacent
// lanes adjacent 16 bytes (1 KiB per wave instruction), frames 64 KiB apart, four frames in flight.  Per bin it keeps the
// running maximum of the bit patterns with the sign cleared (an integer compare: no flush, NaN on top) and a float64 sum of
// the exact squares, frames ascending -- step 1 of the header's order.  Step 2, the balanced pair tree over the W bins, is
// two adds in the thread for the thread's own four bins and, from W = 8 on, an xor-butterfly over the 2..16 adjacent lanes of
// the bucket, which lie inside one 16-lane DPP row: partner 1 and 2 by quad permutation, partner 4 and 8 by the mirrored
// half row and row -- after the earlier levels every lane of a mirrored block holds the same sum, so lane i ^ 7 stands for
// lane i ^ 4 and lane i ^ 15 for lane i ^ 8.  IEEE addition is commutative, so every lane ends with the bits of the tree (a
// NaN may differ in its payload; only isnan is specified), and the bucket's lowest lane stores.  A launch is whole
// workgroups, 16 per group of frames: every lane of every wave is active at the DPP moves.  No LDS, no atomics, no barrier,
// and no thread reads what another thread of this launch wrote.
#include <hip/hip_runtime.h>

#include "sa_fold.hpp"

namespace {

static_assert(sizeof(sa_fold_point) == 8, "one record per 8-byte store, two per 16-byte store");

// one frame's value of one bin into the bin's running maximum and power sum; the product of two float32 values is exact in
// float64, so whether the compiler contracts the two operations into an fma or not, the sum has the same bits
__device__ __forceinline__ void fold_bin(float m, unsigned &mx, double &s)
{
    const unsigned u = __builtin_bit_cast(unsigned, m) & 0x7FFFFFFFu;
    mx = mx > u ? mx : u;
    const double d = (double)m;
    s += d * d;
}

__device__ __forceinline__ void fold_quad(const float4 &r, unsigned (&mx)[4], double (&s)[4])
{
    fold_bin(r.x, mx[0], s[0]);
    fold_bin(r.y, mx[1], s[1]);
    fold_bin(r.z, mx[2], s[2]);
    fold_bin(r.w, mx[3], s[3]);
}

template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// one level of the butterfly: this lane's partial record joined with its partner's
template <int CTRL> __device__ __forceinline__ void fold_lanes(unsigned &mx, double &s)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, s);
    const unsigned lo = dpp_u32<CTRL>((unsigned)b), hi = dpp_u32<CTRL>((unsigned)(b >> 32));
    const unsigned m = dpp_u32<CTRL>(mx);
    mx = mx > m ? mx : m;
    s += __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b)
{
    return a > b ? a : b;
}

// the one rounding of a record's power: float64 to the nearest float32, ties to even
__device__ __forceinline__ unsigned power_bits(double s)
{
    return __builtin_bit_cast(unsigned, (float)s);
}

// grid = (B / A) 16 workgroups of 256 threads, exactly; groupsize = A, a power of two from 1 on.  Every offset is a size_t:
// B 65536 bytes pass 2^32 at B = 65536.
template <int K>
__global__ __launch_bounds__(kFoldThreads) void fold_mag_f32_kernel(const float4 *__restrict__ mag, void *__restrict__ out,
                                                                    int groupsize)
{
    const size_t idx = (size_t)blockIdx.x * kFoldThreads + threadIdx.x;
    constexpr size_t Q = (size_t)1 << kFoldLog2Quads;
    const size_t g = idx >> kFoldLog2Quads, j = idx & (Q - 1);
    const float4 *src = mag + g * (size_t)groupsize * Q + j;       // quad j of frame g A; frame g A + i is i Q further
    unsigned mx[4] = {0u, 0u, 0u, 0u};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int i = 0;
    for (; i + 4 <= groupsize; i += 4) {                          // four loads in flight
        const float4 r0 = src[(size_t)i * Q], r1 = src[(size_t)(i + 1) * Q], r2 = src[(size_t)(i + 2) * Q],
                     r3 = src[(size_t)(i + 3) * Q];
        fold_quad(r0, mx, s);
        fold_quad(r1, mx, s);
        fold_quad(r2, mx, s);
        fold_quad(r3, mx, s);
    }
    if (groupsize & 2) {                                          // A = 2 (groupsize is a power of two): both loads in flight
        const float4 r0 = src[(size_t)i * Q], r1 = src[(size_t)(i + 1) * Q];
        fold_quad(r0, mx, s);
        fold_quad(r1, mx, s);
    }
    if (groupsize & 1) fold_quad(src[0], mx, s);                  // A = 1: buckets of bins alone
    if constexpr (K == 0) {                                       // records 4 idx .. 4 idx + 3: row g, bins 4 j .. 4 j + 3
        uint4 *o = static_cast<uint4 *>(out);
        o[2 * idx] = make_uint4(mx[0], power_bits(s[0]), mx[1], power_bits(s[1]));
        o[2 * idx + 1] = make_uint4(mx[2], power_bits(s[2]), mx[3], power_bits(s[3]));
    } else if constexpr (K == 1) {                                // records 2 idx, 2 idx + 1
        static_cast<uint4 *>(out)[idx] =
            make_uint4(umax(mx[0], mx[1]), power_bits(s[0] + s[1]), umax(mx[2], mx[3]), power_bits(s[2] + s[3]));
    } else {
        unsigned m = umax(umax(mx[0], mx[1]), umax(mx[2], mx[3]));
        double t = (s[0] + s[1]) + (s[2] + s[3]);                 // two levels of the tree
        if constexpr (K >= 3) fold_lanes<0xB1>(m, t);             // quad_perm [1,0,3,2]: lane ^ 1
        if constexpr (K >= 4) fold_lanes<0x4E>(m, t);             // quad_perm [2,3,0,1]: lane ^ 2
        if constexpr (K >= 5) fold_lanes<0x141>(m, t);            // row_half_mirror: lane ^ 7, the bits of lane ^ 4
        if constexpr (K >= 6) fold_lanes<0x140>(m, t);            // row_mirror: lane ^ 15, the bits of lane ^ 8
        constexpr unsigned lanes = 1u << (K - 2);                 // threads per record
        if ((threadIdx.x & (lanes - 1)) == 0) static_cast<uint2 *>(out)[idx >> (K - 2)] = make_uint2(m, power_bits(t));
    }
}

template <int K> void launch(const float *mag, sa_fold_point *out, unsigned blocks, int groupsize, hipStream_t stream)
{
    hipLaunchKernelGGL(fold_mag_f32_kernel<K>, dim3(blocks), dim3(kFoldThreads), 0, stream,
                       reinterpret_cast<const float4 *>(mag), static_cast<void *>(out), groupsize);
}

}  // namespace

extern "C" int sa_fold_version(void)
{
    return SA_FOLD_VERSION;
}

extern "C" int sa_fold_mag_f32(const float *mag, sa_fold_point *out, int batch, int log2a, int log2w, void *stream)
{
    const char *why;
    const int rc = sa_fold_check_call(log2a, log2w, (uint64_t)(uintptr_t)mag, (uint64_t)(uintptr_t)out, batch, &why);
    sa_fold_set_error(why);
    if (rc != SA_OK || batch == 0) return rc;
    const unsigned blocks = (unsigned)((uint64_t)(batch >> log2a) * kFoldBlocksPerGroup);      // the check held it to 2^31 - 1
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (log2w) {
        case 0: launch<0>(mag, out, blocks, 1 << log2a, st); break;
        case 1: launch<1>(mag, out, blocks, 1 << log2a, st); break;
        case 2: launch<2>(mag, out, blocks, 1 << log2a, st); break;
        case 3: launch<3>(mag, out, blocks, 1 << log2a, st); break;
        case 4: launch<4>(mag, out, blocks, 1 << log2a, st); break;
        case 5: launch<5>(mag, out, blocks, 1 << log2a, st); break;
        default: launch<6>(mag, out, blocks, 1 << log2a, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_fold_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
