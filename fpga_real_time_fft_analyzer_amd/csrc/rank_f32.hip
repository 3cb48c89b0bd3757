// rank_f32.hip -- sa_rank_f32 (include/specan_rank.h): the keys at q given ranks of the sorted bins
// [lo, hi) of each row of 16384 points, float32 magnitudes or one float of 8-byte (peak, power) records.  The kernel of
// libspecan_rank.so; it stands beside the chains, the fold and the peak table and shares no text with them.
//
// One workgroup of 256 threads per row, and the row is read from memory once: 16-byte units, unit t + 256 j to thread t
// (16 units of four magnitudes, or 32 units of two records), so that the lanes of a wave read 1 KiB of adjacent bytes per
// instruction; a thread asks for eight units at a time and keeps 64 keys in registers.  A key whose bin lies outside
// [lo, hi) becomes 0xFFFFFFFF, which is below no threshold the selection ever forms.
//
// Selection builds each answer from bit 30 down to bit 0: with t = ans | 1 << b, the bit stays when the number of keys
// below t does not exceed the rank -- the answer is the largest v with #{u < v} <= rank, which is s[rank].  A round costs a
// thread one integer compare per register and rank; the compare's mask is counted by the scalar unit (the wave's count
// needs no exchange between lanes), lane j of every wave puts the wave's count for rank j into one LDS word, and after the
// round's one barrier every thread adds the four waves' words (one 16-byte broadcast read per rank).  The words are
// double-buffered by the round's parity.  All q ranks advance in the same round; the time does not depend on the data.
// Integer counts only: nothing depends on an order.  No workspace, no global or LDS read-modify-write, no FP-mode
// change; every LDS word is written by the launch before it is read, and nothing outside the row is read.
#include <hip/hip_runtime.h>

#include "sa_rank.hpp"

namespace {

constexpr unsigned kSignOff = 0x7FFFFFFFu;                     // a key: the float's bits without the sign
constexpr unsigned kNoBin = 0xFFFFFFFFu;                       // the key of a bin outside the range: never below a threshold
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankGroup = 8;                                  // 16-byte loads a thread has in flight
static_assert(kRankWaves == 4, "a rank's four wave counts are one 16-byte LDS read");
static_assert((kRankBins / 4) % kRankGroup == 0 && (kRankBins / 2) % kRankGroup == 0, "whole groups of loads for both unit sizes");

// the ranks, by value among the kernel's arguments: stream-ordered with the launch, and part of a captured graph's node
struct RankSet {
    int r[SA_RANK_Q_MAX];
};

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD>
__global__ __launch_bounds__(kRankThreads) void rank_f32_kernel(const uint4 *__restrict__ in, unsigned *__restrict__ out, int q,
                                                                int lo, int hi, RankSet ranks)
{
    constexpr int E = FIELD == 0 ? 4 : 2;                          // bins per 16-byte unit
    constexpr int U = kRankBins / E;                               // units per thread
    __shared__ alignas(16) unsigned s_below[2][SA_RANK_Q_MAX][kRankWaves];        // [parity][rank][wave]: keys below the threshold
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    const uint4 *src = in + row * (size_t)(SA_N / E);

    const unsigned width = (unsigned)(hi - lo);                    // lo <= bin < hi as one unsigned compare
    unsigned key[kRankBins];
    uint4 got[kRankGroup];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        if (j % kRankGroup == 0) {
#pragma unroll
            for (int g = 0; g < kRankGroup; ++g) got[g] = src[(size_t)t + (size_t)kRankThreads * (j + g)];
        }
        uint4 v = got[j % kRankGroup];
        // keeps the unit's use behind the group's loads and ahead of the next group's: eight loads in flight, not all 32
        asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
        unsigned w[E];
        if constexpr (FIELD == 0) {
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else if constexpr (FIELD == 1) {
            w[0] = v.x, w[1] = v.z;
        } else {
            w[0] = v.y, w[1] = v.w;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int bin = E * (t + kRankThreads * j) + e;
            key[E * j + e] = (unsigned)(bin - lo) < width ? w[e] & kSignOff : kNoBin;
        }
    }

    unsigned ans[SA_RANK_Q_MAX];
#pragma unroll
    for (int j = 0; j < SA_RANK_Q_MAX; ++j) ans[j] = 0u;
#pragma unroll 1
    for (int b = kRankKeyBits - 1; b >= 0; --b) {
        const unsigned bit = 1u << b;
        const int par = b & 1;
        unsigned mine = 0u;
#pragma unroll
        for (int j = 0; j < SA_RANK_Q_MAX; ++j) {
            if (j < q) {
                const unsigned thr = ans[j] | bit;
                int n = 0;
#pragma unroll
                for (int i = 0; i < kRankBins; ++i) {
                    n += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[i] < thr));
                    asm volatile("" : "+s"(n));                    // counted here: no compare mask is carried on in scalar registers
                }
                mine = lane == j ? (unsigned)n : mine;
            }
        }
        if (lane < q) s_below[par][lane][wave] = mine;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SA_RANK_Q_MAX; ++j) {
            if (j < q) {
                const uint4 c = *reinterpret_cast<const uint4 *>(s_below[par][j]);
                const int below = __builtin_amdgcn_readfirstlane((int)((c.x + c.y) + (c.z + c.w)));
                ans[j] = below <= ranks.r[j] ? ans[j] | bit : ans[j];
            }
        }
    }
    unsigned mine = 0u;
#pragma unroll
    for (int j = 0; j < SA_RANK_Q_MAX; ++j) mine = t == j ? ans[j] : mine;
    if (t < q) out[row * (size_t)q + (size_t)t] = mine;
}

template <int FIELD>
void launch(const void *in, float *out, int rows, int q, int lo, int hi, const RankSet &ranks, hipStream_t stream)
{
    hipLaunchKernelGGL(rank_f32_kernel<FIELD>, dim3((unsigned)rows), dim3(kRankThreads), 0, stream,
                       static_cast<const uint4 *>(in), reinterpret_cast<unsigned *>(out), q, lo, hi, ranks);
}

}  // namespace

extern "C" int sa_rank_version(void)
{
    return SA_RANK_VERSION;
}

extern "C" int sa_rank_f32(const void *in, int field, float *out, int rows, int q, const int32_t *ranks, int lo, int hi,
                           void *stream)
{
    const char *why;
    const int rc = sa_rank_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, rows, q, ranks, lo, hi, &why);
    sa_rank_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    RankSet set = {};
    for (int j = 0; j < q; ++j) set.r[j] = ranks[j];
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_RANK_IN_MAG: launch<0>(in, out, rows, q, lo, hi, set, st); break;
        case SA_RANK_IN_POINT_PEAK: launch<1>(in, out, rows, q, lo, hi, set, st); break;
        default: launch<2>(in, out, rows, q, lo, hi, set, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_rank_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
