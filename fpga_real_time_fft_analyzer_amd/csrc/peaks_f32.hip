// peaks_f32.hip -- sa_peaks_f32 (include/specan_peaks.h): the K strongest local maxima of each row
// of 16384 points, float32 magnitudes or one float of 8-byte (peak, power) records.  The kernel of libspecan_peaks.so; it
// stands beside the chains and the fold and shares no text with them.
//
// One workgroup of 256 threads per row.  The row arrives as 16-byte units, unit t + 256 j to thread t (j = 0..15 for
// magnitudes, four bins a unit; j = 0..31 for records, two bins a unit): adjacent lanes read adjacent units, 1 KiB per wave
// instruction, eight loads of a thread in flight, and every thread ends with 64 keys in registers, its bins ascending with
// the register index.  The neighbour
// keys at a unit's two edges come from the adjacent lane (ds_bpermute: no LDS word is touched); lanes 0 and 63 of a wave,
// whose neighbour unit lies in another wave, read that one float again (a cache hit), and the neighbours that bins 0 and
// 16383 do not have are decided without a load.  A key that is no candidate becomes 0, which no candidate has.
//
// Selection is K rounds.  Every thread holds the best of its candidates as one 64-bit word, key in the high half and the
// complement of the bin in the low half, so that an unsigned maximum is "larger key, then lower bin" and 0 is "none".  A
// round is an xor-butterfly of that word inside the wave (DPP inside the 16-lane rows, two bpermute levels across them), one
// LDS slot per wave, one barrier, and the maximum of the four slots in every thread.  The winner and everything closer to it
// than min_sep is then zeroed -- per block of 64 adjacent units of a wave a scalar range test, so that a wave the winner is
// far from does no vector work -- and only a thread that lost a candidate scans its 64 registers again.  The slots are
// double-buffered by the round's parity: one barrier a round.  Thread r keeps record r and the threads 0..K-1 store the
// row's records in one instruction; the count is an integer sum of the waves' ballots.  No atomics, no FP-mode change, every LDS word is written
// by the launch before it is read, and nothing outside the row is read.
#include <hip/hip_runtime.h>

#include "sa_peaks.hpp"

namespace {

static_assert(sizeof(sa_peak) == 8, "one record per 8-byte store");

constexpr unsigned kAbs = 0x7FFFFFFFu;
constexpr int kWaves = kPeaksThreads / 64;
constexpr int kPeaksLoads = 8;                                 // 16-byte loads a thread has in flight: 16 or 32 units in groups of 8
static_assert((kPeaksBins / 4) % kPeaksLoads == 0, "whole groups of loads for both unit sizes");

template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b)
{
    return a > b ? a : b;
}

// one level of the butterfly inside a 16-lane row
template <int CTRL> __device__ __forceinline__ unsigned long long max_dpp(unsigned long long v)
{
    const unsigned lo = dpp_u32<CTRL>((unsigned)v), hi = dpp_u32<CTRL>((unsigned)(v >> 32));
    return umax64(v, (unsigned long long)hi << 32 | lo);
}

// the maximum over the wave's 64 lanes, in every lane.  A maximum is idempotent: after the first two levels the four lanes
// of a quad agree, so the mirrored half row (lane ^ 7) stands for lane ^ 4 and the mirrored row (lane ^ 15) for lane ^ 8.
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    v = max_dpp<0xB1>(v);                                          // quad_perm [1,0,3,2]: lane ^ 1
    v = max_dpp<0x4E>(v);                                          // quad_perm [2,3,0,1]: lane ^ 2
    v = max_dpp<0x141>(v);                                         // row_half_mirror
    v = max_dpp<0x140>(v);                                         // row_mirror
    v = umax64(v, __shfl_xor(v, 16));
    return umax64(v, __shfl_xor(v, 32));
}

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b)
{
    return a > b ? a : b;
}

// E bins per unit: the bin of register i of thread t
template <int E> __device__ __forceinline__ int bin_of(int t, int i)
{
    return E * (t + kPeaksThreads * (i / E)) + i % E;
}

// the best candidate of a thread: the largest key, the lowest register (= the lowest bin) among equals; 0 when it has none
template <int E> __device__ __forceinline__ unsigned long long best_of(const unsigned (&ck)[kPeaksBins], int t)
{
    unsigned bk = 0;
    int bi = 0;
#pragma unroll
    for (int i = 0; i < kPeaksBins; ++i) {
        const bool up = ck[i] > bk;
        bk = up ? ck[i] : bk;
        bi = up ? i : bi;
    }
    return bk ? (unsigned long long)bk << 32 | ~(unsigned)bin_of<E>(t, bi) : 0ull;
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD>
__global__ __launch_bounds__(kPeaksThreads) void peaks_f32_kernel(const uint4 *__restrict__ in, uint2 *__restrict__ out,
                                                                  int *__restrict__ count, int k, unsigned thr, int lo, int hi,
                                                                  int min_sep)
{
    constexpr int E = FIELD == 0 ? 4 : 2;                          // bins per 16-byte unit
    constexpr int U = kPeaksBins / E;                              // units per thread
    constexpr int W = FIELD == 0 ? 1 : 2;                          // floats per bin
    __shared__ unsigned long long s_best[2][kWaves];
    __shared__ int s_count[kWaves];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    const uint4 *src = in + row * (size_t)(SA_N / E);
    const unsigned *words = reinterpret_cast<const unsigned *>(src);               // the row as 32-bit words

    // the one key beyond each unit's edge that no lane of this wave holds: left of lane 0, right of lane 63
    unsigned edge[U];
#pragma unroll
    for (int j = 0; j < U; ++j) edge[j] = 0u;                      // a neighbour that does not exist: 0 satisfies both conditions
    if (lane == 0 || lane == 63) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int u = t + kPeaksThreads * j;
            const int b = lane == 0 ? E * u - 1 : E * u + E;                       // -1 and 16384 are no bins of the row:
            const int c = b < 0 ? 0 : b >= SA_N ? SA_N - 1 : b;                    // nothing outside it is read
            const unsigned w = words[W * c + (FIELD == 2)] & kAbs;
            edge[j] = b == c ? w : 0u;
        }
    }

    const unsigned width = (unsigned)(hi - lo), floor = thr > 1u ? thr : 1u;       // lo <= bin < hi as one compare; u > 0 and u >= thr
    unsigned ck[kPeaksBins];
    int n = 0;
    uint4 rs[kPeaksLoads];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        if (j % kPeaksLoads == 0) {                                // the next eight units of the thread: eight loads in flight
#pragma unroll
            for (int q = 0; q < kPeaksLoads; ++q) rs[q] = src[t + kPeaksThreads * (j + q)];
        }
        uint4 r = rs[j % kPeaksLoads];
        // one 16-byte load, also where two of its floats are unused.  The statement also orders what it names behind the
        // statement before it, which is why the loads are issued a group ahead of it and not one by one beside it (one load in
        // flight per thread took 1.5 times as long, all 16 or 32 cost registers and occupancy: DESIGN.md section 4.17)
        asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
        unsigned key[E];
        if constexpr (FIELD == 0) {
            key[0] = r.x & kAbs, key[1] = r.y & kAbs, key[2] = r.z & kAbs, key[3] = r.w & kAbs;
        } else if constexpr (FIELD == 1) {
            key[0] = r.x & kAbs, key[1] = r.z & kAbs;
        } else {
            key[0] = r.y & kAbs, key[1] = r.w & kAbs;
        }
        unsigned left = __shfl_up(key[E - 1], 1), right = __shfl_down(key[0], 1);
        left = lane == 0 ? edge[j] : left;
        right = lane == 63 ? edge[j] : right;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned u = key[e], l = e == 0 ? left : key[e > 0 ? e - 1 : 0], rr = e == E - 1 ? right : key[e < E - 1 ? e + 1 : 0];
            const int bin = E * (t + kPeaksThreads * j) + e;
            const unsigned need = umax(umax(floor, l + 1u), rr);   // u > l is u >= l + 1: a key is below 2^31
            const bool cand = ((unsigned)(bin - lo) < width) & (u >= need);
            unsigned c = cand ? u : 0u;
            asm volatile("" : "+v"(c));                            // the select here, in a register: no compare mask is carried on
            ck[E * j + e] = c;
            n += __builtin_popcountll(__builtin_amdgcn_ballot_w64(cand));             // the wave's candidates at this register: scalar work,
            asm volatile("" : "+s"(n));                            // done here, so that the mask is not carried on either
        }
    }
    if (lane == 0) s_count[wave] = n;

    unsigned long long mine = best_of<E>(ck, t);
    unsigned rec_key = 0u, rec_bin = 0xFFFFFFFFu;                  // (+0.0f, -1)
    for (int r = 0; r < k; ++r) {
        unsigned long long v = wave_max(mine);
        if (lane == 0) s_best[r & 1][wave] = v;
        __syncthreads();
        v = umax64(umax64(s_best[r & 1][0], s_best[r & 1][1]), umax64(s_best[r & 1][2], s_best[r & 1][3]));
        const unsigned key = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        if (key == 0u) break;                                      // no candidate left; every thread reads the same slots
        const int p = (int)~__builtin_amdgcn_readfirstlane((unsigned)v);
        if (t == r) rec_key = key, rec_bin = (unsigned)p;
        if (r + 1 == k) break;
        const int a = p - min_sep + 1;
        const unsigned span = 2u * (unsigned)min_sep - 2u;         // bins a .. a + span go
        unsigned lost = 0u;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int first = E * (64 * wave + kPeaksThreads * j);                 // this wave's bins first .. first + 64 E - 1
            if (a <= first + 64 * E - 1 && a + (int)span >= first) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool gone = (unsigned)(E * (t + kPeaksThreads * j) + e - a) <= span;
                    lost |= gone ? ck[E * j + e] : 0u;
                    ck[E * j + e] = gone ? 0u : ck[E * j + e];
                }
            }
        }
        if (lost) mine = best_of<E>(ck, t);
    }
    if (t < k) out[row * (size_t)k + t] = make_uint2(rec_key, rec_bin);
    if (t == 0) count[row] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
}

template <int FIELD>
void launch(const void *in, sa_peak *out, int32_t *count, int rows, int k, unsigned thr, int lo, int hi, int min_sep,
            hipStream_t stream)
{
    hipLaunchKernelGGL(peaks_f32_kernel<FIELD>, dim3((unsigned)rows), dim3(kPeaksThreads), 0, stream,
                       static_cast<const uint4 *>(in), reinterpret_cast<uint2 *>(out), count, k, thr, lo, hi, min_sep);
}

}  // namespace

extern "C" int sa_peaks_version(void)
{
    return SA_PEAKS_VERSION;
}

extern "C" int sa_peaks_f32(const void *in, int field, sa_peak *out, int32_t *count, int rows, int k, float threshold, int lo,
                            int hi, int min_sep, void *stream)
{
    const unsigned thr = __builtin_bit_cast(unsigned, threshold);
    const char *why;
    const int rc = sa_peaks_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, (uint64_t)(uintptr_t)count, rows,
                                       k, thr, lo, hi, min_sep, &why);
    sa_peaks_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_PEAKS_IN_MAG: launch<0>(in, out, count, rows, k, thr, lo, hi, min_sep, st); break;
        case SA_PEAKS_IN_POINT_PEAK: launch<1>(in, out, count, rows, k, thr, lo, hi, min_sep, st); break;
        default: launch<2>(in, out, count, rows, k, thr, lo, hi, min_sep, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_peaks_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
