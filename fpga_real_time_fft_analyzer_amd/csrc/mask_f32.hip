// mask_f32.hip -- sa_mask_f32 (include/specan_mask.h): every row of 16384 points, float32 magnitudes or
// one float of 8-byte (peak, power) records, held against an upper and a lower limit line over a range of bins: the bins that
// left the mask counted, the first and last of them, and the worst bin of either limit by the exact ratio of point and limit;
// and, when asked, the rows that failed over the call.  The kernels of libspecan_mask.so; they stand beside the chains and the
// other reductions and share no text with them.
//
// One workgroup of 256 threads per row, and the row is read from memory once: in round r a thread takes the four adjacent bins
// 1024 r + 4 t .. + 3 (one 16-byte load of magnitudes, two adjacent ones of records) and the four limits of either line at the
// same bins (one 16-byte load each: the lines are 64 KiB, shared by every row, and come from cache), so the lanes of a wave
// read adjacent bytes.  Only the rounds that hold a bin of [lo, hi) are read, and the loads of the round ahead are issued
// before a round is looked at (measured against the plain loop).  Nothing of a row is kept: a thread carries two
// counts, a lowest and a highest bin and one candidate per limit -- the key of the point and the limit as doubles, the point's
// bits and the bin.  Candidate (a_i, u_i) replaces (a_j, u_j) when a_i u_j > a_j u_i (upper; < for the lower limit): both
// products are exact in float64, so this is the order of the exact ratios.  The counts compare the bits as integers, which is
// the float32 order of non-negative values and puts a NaN above every limit.
//
// The 256 candidates of a row are merged by a total order -- better ratio, then lower bin -- through an xor-butterfly over the
// wave and then over the four waves' results in 160 bytes of static LDS, written by the launch before it is read: the order is
// total, so the result does not depend on the shape of the reduction.  Thread 0 stores the record, five 8-byte stores, exactly
// once.  The summary is a second launch of one workgroup that reads (over, under) of every record: integers, no atomics,
// nothing to zero.  No workspace, no FP-mode change; every offset into the tensors is a size_t.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "sa_mask.hpp"

namespace {

constexpr int kMaskWaves = kMaskThreads / 64;
constexpr unsigned kInfBits = 0x7F800000u;

// the worst bin of one limit so far: the point's bits (sign cleared), its limit, its bin; bin < 0 when there is none
struct Cand {
    unsigned val;
    float lim;
    int bin;
};

// the point as it stands in the ratio: a NaN is +inf against the upper limit and 0 against the lower
template <bool UP> __device__ __forceinline__ double key(unsigned bits)
{
    const float a = __builtin_bit_cast(float, bits > kInfBits ? (UP ? kInfBits : 0u) : bits);
    return (double)a;
}

// x before y in the order of the header: the larger (UP) or smaller exact ratio, then the lower bin.  Keys lie in [0, +inf]
// and limits are finite and above 0, so no product is a NaN.
template <bool UP> __device__ __forceinline__ Cand merge(const Cand &x, const Cand &y)
{
    const double cx = key<UP>(x.val) * (double)y.lim, cy = key<UP>(y.val) * (double)x.lim;
    const bool better = UP ? cx > cy : cx < cy;
    const bool first = better || (cx == cy && x.bin < y.bin);
    const bool take_x = y.bin < 0 || (x.bin >= 0 && first);
    return take_x ? x : y;
}

__device__ __forceinline__ Cand shfl_xor(const Cand &c, int mask)
{
    Cand o;
    o.val = (unsigned)__shfl_xor((int)c.val, mask);
    o.lim = __shfl_xor(c.lim, mask);
    o.bin = __shfl_xor(c.bin, mask);
    return o;
}

// what a thread, a wave and a row know
struct Part {
    int over, under, first, last;                                  // first = INT_MAX and last = -1 when nothing was counted
    Cand up, low;
};

template <bool UP, bool LOW> __device__ __forceinline__ Part combine(const Part &a, const Part &b)
{
    Part p;
    p.over = a.over + b.over, p.under = a.under + b.under;
    p.first = a.first < b.first ? a.first : b.first;
    p.last = a.last > b.last ? a.last : b.last;
    if constexpr (UP) p.up = merge<true>(a.up, b.up);
    else p.up = a.up;
    if constexpr (LOW) p.low = merge<false>(a.low, b.low);
    else p.low = a.low;
    return p;
}

// the running candidate of a thread, the key and the limit widened once
struct Best {
    double k, l;
    unsigned val;
    int bin;
};

// the four points of a thread in one round and the limits at their bins, as bits
struct Round {
    unsigned pt[4], u[4], l[4];
};

// unit q of the row: the bins 4 q .. 4 q + 3.  A limit that is not there is never read.
template <int FIELD, bool UP, bool LOW>
__device__ __forceinline__ Round fetch(const uint4 *__restrict__ src, const uint4 *__restrict__ upper, const uint4 *__restrict__ lower,
                                       size_t q)
{
    Round x = {};
    if constexpr (FIELD == SA_MASK_IN_MAG) {
        const uint4 v = src[q];
        x.pt[0] = v.x, x.pt[1] = v.y, x.pt[2] = v.z, x.pt[3] = v.w;
    } else {
        const uint4 v0 = src[2 * q], v1 = src[2 * q + 1];
        if constexpr (FIELD == SA_MASK_IN_POINT_PEAK) {
            x.pt[0] = v0.x, x.pt[1] = v0.z, x.pt[2] = v1.x, x.pt[3] = v1.z;
        } else {
            x.pt[0] = v0.y, x.pt[1] = v0.w, x.pt[2] = v1.y, x.pt[3] = v1.w;
        }
    }
    if constexpr (UP) {
        const uint4 v = upper[q];
        x.u[0] = v.x, x.u[1] = v.y, x.u[2] = v.z, x.u[3] = v.w;
    }
    if constexpr (LOW) {
        const uint4 v = lower[q];
        x.l[0] = v.x, x.l[1] = v.y, x.l[2] = v.z, x.l[3] = v.w;
    }
    return x;
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD, bool UP, bool LOW>
__global__ __launch_bounds__(kMaskThreads) void mask_f32_kernel(const uint4 *__restrict__ in, const uint4 *__restrict__ upper,
                                                                const uint4 *__restrict__ lower, uint2 *__restrict__ rows_out, int lo,
                                                                int hi)
{
    __shared__ Part s_wave[kMaskWaves];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    constexpr int UNITS = FIELD == SA_MASK_IN_MAG ? 1 : 2;         // 16-byte loads per thread and round
    const uint4 *src = in + row * (size_t)(SA_N / 4 * UNITS);
    const unsigned width = (unsigned)(hi - lo);                    // lo <= bin < hi as one unsigned compare

    int over = 0, under = 0, first = INT_MAX, last = -1;
    Best bu = {0.0, 1.0, 0u, -1}, bl = {0.0, 1.0, 0u, -1};
    const int r0 = lo / kMaskRound, r1 = (hi - 1) / kMaskRound;    // the rounds that hold a bin of the range
    // the round ahead is requested before this one is looked at: two rounds of loads in flight per thread
    Round next = fetch<FIELD, UP, LOW>(src, upper, lower, (size_t)t + (size_t)kMaskThreads * (size_t)r0);
#pragma unroll 1
    for (int r = r0; r <= r1; ++r) {
        const Round now = next;
        if (r < r1) next = fetch<FIELD, UP, LOW>(src, upper, lower, (size_t)t + (size_t)kMaskThreads * (size_t)(r + 1));
        const unsigned(&pt)[4] = now.pt, (&u)[4] = now.u, (&l)[4] = now.l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int bin = kMaskRound * r + 4 * t + e;
            const bool inside = (unsigned)(bin - lo) < width;
            const unsigned a = pt[e] & 0x7FFFFFFFu;
            bool bad = false;
            if constexpr (UP) {
                const bool has = inside && u[e] - 1u < kInfBits - 1u;             // finite and above 0: bits 1 .. 0x7F7FFFFF
                const bool out = has && a > u[e];                                   // as integers: a NaN lies above every limit
                over += out;
                bad = out;
                const double k = key<true>(a), lim = (double)__builtin_bit_cast(float, u[e]);
                if (has && (bu.bin < 0 || k * bu.l > bu.k * lim)) bu = {k, lim, a, bin};
            }
            if constexpr (LOW) {
                const bool has = inside && l[e] - 1u < kInfBits - 1u;
                const bool out = has && (a < l[e] || a > kInfBits);
                under += out;
                bad = bad || out;
                const double k = key<false>(a), lim = (double)__builtin_bit_cast(float, l[e]);
                if (has && (bl.bin < 0 || k * bl.l < bl.k * lim)) bl = {k, lim, a, bin};
            }
            first = bad && bin < first ? bin : first;
            last = bad && bin > last ? bin : last;
        }
    }

    Part p;
    p.over = over, p.under = under, p.first = first, p.last = last;
    p.up = {bu.val, bu.bin < 0 ? 0.0f : (float)bu.l, bu.bin};     // the limit came from a float: the narrowing is exact
    p.low = {bl.val, bl.bin < 0 ? 0.0f : (float)bl.l, bl.bin};
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        Part o;
        o.over = __shfl_xor(p.over, m), o.under = __shfl_xor(p.under, m);
        o.first = __shfl_xor(p.first, m), o.last = __shfl_xor(p.last, m);
        o.up = shfl_xor(p.up, m), o.low = shfl_xor(p.low, m);
        p = combine<UP, LOW>(p, o);
    }
    if (lane == 0) s_wave[wave] = p;
    __syncthreads();
    if (t == 0) {
        Part all = s_wave[0];
#pragma unroll
        for (int w = 1; w < kMaskWaves; ++w) all = combine<UP, LOW>(all, s_wave[w]);
        uint2 *rec = rows_out + row * (size_t)(sizeof(sa_mask_row) / sizeof(uint2));
        rec[0] = make_uint2((unsigned)all.over, (unsigned)all.under);
        rec[1] = make_uint2((unsigned)(all.first == INT_MAX ? -1 : all.first), (unsigned)all.last);
        rec[2] = make_uint2((unsigned)all.up.bin, (unsigned)all.low.bin);
        rec[3] = make_uint2(all.up.val, __builtin_bit_cast(unsigned, all.up.lim));
        rec[4] = make_uint2(all.low.val, __builtin_bit_cast(unsigned, all.low.lim));
    }
}

// The trigger: one workgroup over the records the launch before it wrote.  summary = rows with over > 0, rows with under > 0,
// the first row with either or -1, the last or -1.
__global__ __launch_bounds__(kMaskSumThreads) void mask_summary_kernel(const uint2 *__restrict__ rows_out, int *__restrict__ summary,
                                                                       int rows)
{
    __shared__ int s_part[kMaskSumThreads / 64][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int n_over = 0, n_under = 0, first = INT_MAX, last = -1;
    for (size_t r = (size_t)t; r < (size_t)rows; r += (size_t)kMaskSumThreads) {
        const uint2 c = rows_out[r * (size_t)(sizeof(sa_mask_row) / sizeof(uint2))];
        const bool o = (int)c.x > 0, u = (int)c.y > 0;
        n_over += o, n_under += u;
        if (o || u) {
            first = (int)r < first ? (int)r : first;
            last = (int)r > last ? (int)r : last;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        n_over += __shfl_xor(n_over, m), n_under += __shfl_xor(n_under, m);
        const int f = __shfl_xor(first, m), l = __shfl_xor(last, m);
        first = f < first ? f : first, last = l > last ? l : last;
    }
    if (lane == 0) s_part[wave][0] = n_over, s_part[wave][1] = n_under, s_part[wave][2] = first, s_part[wave][3] = last;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kMaskSumThreads / 64; ++w) {
            n_over += s_part[w][0], n_under += s_part[w][1];
            first = s_part[w][2] < first ? s_part[w][2] : first;
            last = s_part[w][3] > last ? s_part[w][3] : last;
        }
        summary[0] = n_over, summary[1] = n_under, summary[2] = first == INT_MAX ? -1 : first, summary[3] = last;
    }
}

template <int FIELD, bool UP, bool LOW>
void launch(const void *in, const float *upper, const float *lower, int lo, int hi, sa_mask_row *rows_out, int rows, hipStream_t stream)
{
    hipLaunchKernelGGL((mask_f32_kernel<FIELD, UP, LOW>), dim3((unsigned)rows), dim3(kMaskThreads), 0, stream,
                       static_cast<const uint4 *>(in), reinterpret_cast<const uint4 *>(upper), reinterpret_cast<const uint4 *>(lower),
                       reinterpret_cast<uint2 *>(rows_out), lo, hi);
}

template <int FIELD>
void launch_field(const void *in, const float *upper, const float *lower, int lo, int hi, sa_mask_row *rows_out, int rows,
                  hipStream_t stream)
{
    if (upper && lower) launch<FIELD, true, true>(in, upper, lower, lo, hi, rows_out, rows, stream);
    else if (upper) launch<FIELD, true, false>(in, upper, lower, lo, hi, rows_out, rows, stream);
    else launch<FIELD, false, true>(in, upper, lower, lo, hi, rows_out, rows, stream);
}

}  // namespace

extern "C" int sa_mask_version(void)
{
    return SA_MASK_VERSION;
}

extern "C" int sa_mask_f32(const void *in, int field, const float *upper, const float *lower, int lo, int hi, sa_mask_row *rows_out,
                           int32_t *summary, int rows, void *stream)
{
    const char *why;
    const int rc = sa_mask_check_call((uint64_t)(uintptr_t)in, field, (uint64_t)(uintptr_t)upper, (uint64_t)(uintptr_t)lower, lo, hi,
                                      (uint64_t)(uintptr_t)rows_out, (uint64_t)(uintptr_t)summary, rows, &why);
    sa_mask_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_MASK_IN_MAG: launch_field<0>(in, upper, lower, lo, hi, rows_out, rows, st); break;
        case SA_MASK_IN_POINT_PEAK: launch_field<1>(in, upper, lower, lo, hi, rows_out, rows, st); break;
        default: launch_field<2>(in, upper, lower, lo, hi, rows_out, rows, st); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && summary) {
        hipLaunchKernelGGL(mask_summary_kernel, dim3(1), dim3(kMaskSumThreads), 0, st, reinterpret_cast<const uint2 *>(rows_out),
                           summary, rows);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        sa_mask_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
