// cfar_f32.hip -- sa_cfar_f32 (include/specan_cfar.h): per row of 16384 points every bin against the
// mean power of T training cells on either side of it beyond G guard cells -- the ratio, or that local floor itself -- in the
// cell-averaging, greatest-of or smallest-of form.  The kernel of libspecan_cfar.so; it stands beside the chains and the
// other reductions and shares no text with them.
//
// One workgroup of 256 threads per row, which it reads once and holds in registers.  In round r a thread takes the four
// adjacent bins 1024 r + 4 t .. + 3 (one 16-byte load of magnitudes, two adjacent ones of records) and stores them, after
// the tile's work, as one 16-byte store.  The row is worked in 8 tiles of 2048 bins, two rounds, one after the other:
//
//   1  the cells of the tile and of a halo of G_max + T_max = 128 bins on either side, float64, masked to [lo, hi) and +0.0
//      beyond the row, go from the registers of the threads that hold them to LDS: 2304 cells.  The halo has its largest
//      size whatever G and T are, so every register index is known at compile time.               -> s_w[0][0..2304)
//   -- barrier
//   2  log2_train doubling steps W(l+1)[e] = W(l)[e] + W(l)[e + 2^l], each from one buffer into the other (no step reads
//      what another wave is writing), one barrier after each; a level is 2^l entries shorter than the one below it, and no
//      entry is read that the level below did not write
//   3  bin i of the tile reads L = W[i - G - T] and R = W[i + G + 1] of the last level; the side counts are integer
//      arithmetic on i, lo, hi, G and T; two float64 products decide greatest-of and smallest-of; one float64 division and
//      one conversion make the float
//   -- barrier, before the next tile's cells go in
// Static LDS of 36 KiB (four workgroups on a CU), every entry written by the launch before it is read; no workspace, no
// atomics, no FP-mode change; every float of `out` is stored exactly once and nothing but the row is read.
#include <hip/hip_runtime.h>

#include "sa_cfar.hpp"

// every sum and product is one rounded float64 operation in the header's order
#pragma clang fp contract(off)

namespace {

constexpr unsigned kQuietNan = 0x7FC00000u, kInf = 0x7F800000u;

// the point's value: the key as a float, widened (exact, denormals kept), squared unless it is a power already
template <int FIELD> __device__ __forceinline__ double value(unsigned key)
{
    const double a = (double)__builtin_bit_cast(float, key);
    return FIELD == SA_CFAR_IN_POINT_POWER ? a : a * a;
}

// lo <= i < lo + width as one unsigned compare
__device__ __forceinline__ bool within(int i, int lo, int width)
{
    return (unsigned)(i - lo) < (unsigned)width;
}

// the four cells of the quad at `bin0` into the tile's image at `idx`; `row_has` is false where the quad lies beyond the row
template <int FIELD>
__device__ __forceinline__ void put_cells(double *w, int idx, const unsigned (&p)[4], int bin0, bool row_has, int lo, int hi)
{
    double c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = row_has && within(bin0 + e, lo, hi - lo) ? value<FIELD>(p[e]) : 0.0;
    *reinterpret_cast<double2 *>(w + idx) = make_double2(c[0], c[1]);
    *reinterpret_cast<double2 *>(w + idx + 2) = make_double2(c[2], c[3]);
}

// the output's bits for bin i: v its value, L and R the window sums of its sides
__device__ __forceinline__ unsigned point(double v, double L, double R, int i, int G, int T, int mode, int what, int lo, int hi)
{
    const int nL = max(0, min(i - G, hi) - max(i - G - T, lo));
    const int nR = max(0, min(i + G + 1 + T, hi) - max(i + G + 1, lo));
    double S = L + R;
    int n = nL + nR;
    if (mode != SA_CFAR_MODE_CA) {
        const double a = L * (double)nR, b = R * (double)nL;
        bool left = mode == SA_CFAR_MODE_GO ? a >= b : a <= b;
        if (nR == 0) left = true;
        if (nL == 0) left = false;
        S = left ? L : R;
        n = left ? nL : nR;
    }
    const bool ratio = what == SA_CFAR_OUT_RATIO;
    const double dn = (double)n;
    const double q = ratio ? (v * dn) / S : S / dn;
    unsigned bits = __builtin_bit_cast(unsigned, (float)q);
    if (q != q) bits = kQuietNan;
    if (S == 0.0) bits = ratio && v != 0.0 ? kInf : 0u;
    if (L != L || R != R || (ratio && v != v)) bits = kQuietNan;
    return within(i, lo, hi - lo) ? bits : 0u;
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD>
__global__ __launch_bounds__(kCfarThreads) void cfar_f32_kernel(const uint4 *__restrict__ in, uint4 *__restrict__ out,
                                                                int log2_train, int G, int mode, int what, int lo, int hi)
{
    __shared__ __attribute__((aligned(16))) double s_w[2][kCfarCells];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    constexpr int UNITS = FIELD == SA_CFAR_IN_MAG ? 1 : 2;         // 16-byte loads per thread and round
    const uint4 *src = in + row * (size_t)(SA_N / 4 * UNITS);
    uint4 *dst = out + row * (size_t)(SA_N / 4);
    const int T = 1 << log2_train;

    // the keys: the sign is cleared once, here
    unsigned pt[kCfarRounds][4];
#pragma unroll
    for (int r = 0; r < kCfarRounds; ++r) {
        const size_t u = (size_t)UNITS * ((size_t)t + (size_t)kCfarThreads * r);
        if constexpr (FIELD == SA_CFAR_IN_MAG) {
            const uint4 v = src[u];
            pt[r][0] = v.x, pt[r][1] = v.y, pt[r][2] = v.z, pt[r][3] = v.w;
        } else {
            const uint4 v0 = src[u], v1 = src[u + 1];
            if constexpr (FIELD == SA_CFAR_IN_POINT_PEAK) {
                pt[r][0] = v0.x, pt[r][1] = v0.z, pt[r][2] = v1.x, pt[r][3] = v1.z;
            } else {
                pt[r][0] = v0.y, pt[r][1] = v0.w, pt[r][2] = v1.y, pt[r][3] = v1.w;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) pt[r][e] &= 0x7FFFFFFFu;
    }

#pragma unroll
    for (int k = 0; k < kCfarTiles; ++k) {
        constexpr int kQuads = kCfarHalo / 4;                      // the threads of a neighbouring round that hold a halo
        const int base = kCfarTile * k;
        // 1: image index e is bin base - kCfarHalo + e
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
            put_cells<FIELD>(s_w[0], kCfarHalo + 4 * kCfarThreads * rr + 4 * t, pt[2 * k + rr], base + 4 * kCfarThreads * rr + 4 * t,
                             true, lo, hi);
        if (t >= kCfarThreads - kQuads)                            // the last 128 bins of the round below the tile
            put_cells<FIELD>(s_w[0], 4 * t - (4 * kCfarThreads - kCfarHalo), pt[k > 0 ? 2 * k - 1 : 0],
                             base - 4 * kCfarThreads + 4 * t, k > 0, lo, hi);
        if (t < kQuads)                                            // the first 128 bins of the round above it
            put_cells<FIELD>(s_w[0], kCfarHalo + kCfarTile + 4 * t, pt[k < kCfarTiles - 1 ? 2 * k + 2 : 0],
                             base + kCfarTile + 4 * t, k < kCfarTiles - 1, lo, hi);
        __syncthreads();

        // 2
        int cur = 0, len = kCfarCells;
        for (int l = 0; l < log2_train; ++l) {
            const int h = 1 << l;
            len -= h;                                              // e + h < len + h: inside what the level below wrote
            const double *from = s_w[cur];
            double *to = s_w[cur ^ 1];
#pragma unroll
            for (int j = 0; j < kCfarCells / kCfarThreads; ++j) {
                const int e = t + kCfarThreads * j;
                if (e < len) to[e] = from[e] + from[e + h];
            }
            cur ^= 1;
            __syncthreads();
        }

        // 3: G + T <= kCfarHalo, so 0 <= e - G - T and e + G + 1 <= kCfarCells - T < len
        const double *w = s_w[cur];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int e0 = kCfarHalo + 4 * kCfarThreads * rr + 4 * t, bin0 = base + 4 * kCfarThreads * rr + 4 * t;
            unsigned o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = point(value<FIELD>(pt[2 * k + rr][e]), w[e0 + e - G - T], w[e0 + e + G + 1], bin0 + e, G, T, mode, what,
                             lo, hi);
            dst[bin0 / 4] = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (k + 1 < kCfarTiles) __syncthreads();
    }
}

template <int FIELD>
void launch(const void *in, float *out, int rows, int log2_train, int guard, int mode, int what, int lo, int hi,
            hipStream_t stream)
{
    hipLaunchKernelGGL((cfar_f32_kernel<FIELD>), dim3((unsigned)rows), dim3(kCfarThreads), 0, stream,
                       static_cast<const uint4 *>(in), reinterpret_cast<uint4 *>(out), log2_train, guard, mode, what, lo, hi);
}

}  // namespace

extern "C" int sa_cfar_version(void)
{
    return SA_CFAR_VERSION;
}

extern "C" int sa_cfar_f32(const void *in, int field, float *out, int rows, int log2_train, int guard, int mode, int what, int lo,
                           int hi, void *stream)
{
    const char *why;
    const int rc = sa_cfar_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, rows, log2_train, guard, mode,
                                      what, lo, hi, &why);
    sa_cfar_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_CFAR_IN_MAG: launch<0>(in, out, rows, log2_train, guard, mode, what, lo, hi, st); break;
        case SA_CFAR_IN_POINT_PEAK: launch<1>(in, out, rows, log2_train, guard, mode, what, lo, hi, st); break;
        default: launch<2>(in, out, rows, log2_train, guard, mode, what, lo, hi, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_cfar_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
