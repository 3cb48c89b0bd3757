// hold_f32.hip -- sa_hold_f32 (include/specan_hold.h): the keys at q given ranks of the sorted
// frames of each bin, over groups of A consecutive rows of 16384 points, float32 magnitudes or one float of 8-byte (peak,
// power) records.  The kernel of libspecan_hold.so; it stands beside the chains and the other reductions and shares no text
// with them.
//
// A thread owns one bin of one group -- in the classes of 16 keys or fewer the adjacent bins of one 16-byte load, four
// magnitudes or two records -- and keeps that bin's keys in registers: nothing is exchanged between lanes, and there is no
// LDS.  Row a of the group is read by adjacent lanes at adjacent addresses; the loads of all rows are independent and are
// all in flight before the first use.  Registers are indexed at compile time, so the kernel is built per layout and per
// register class AMAX = 8, 16, 32, 64, 128 >= A: a row a >= A is not read (the load goes to row A - 1 again, a cache hit)
// and its key becomes 0xFFFFFFFF, which sorts behind every key of a point.
//
// The AMAX keys are sorted by Batcher's odd-even merge sort, a fixed network of compare-exchange steps (one integer minimum
// and one maximum each; 19, 63, 191, 543 and 1471 steps for the five classes), spelled out at compile time: all ranks are
// there at once, the time depends neither on the data nor, but for the pick and the stores, on q.  The key of rank r is then
// picked by AMAX selects on the wave-uniform r.  Integer compares only: nothing depends on an order.  One launch, groups on
// the grid's x, no workspace, no atomics, no FP-mode change; nothing outside the group's rows is read.
#include <hip/hip_runtime.h>

#include <utility>

#include "sa_hold.hpp"

namespace {

constexpr unsigned kSignOff = 0x7FFFFFFFu;                     // a key: the float's bits without the sign
constexpr unsigned kNoKey = 0xFFFFFFFFu;                       // the key of a row beyond the group: behind every point's

// the ranks, by value among the kernel's arguments: stream-ordered with the launch, and part of a captured graph's node
struct HoldRanks {
    int r[SA_HOLD_Q_MAX];
};

// Batcher's odd-even merge sort of n = 2^k keys as the list of its compare-exchange steps (lo[c], hi[c]), in an order in
// which they may be made one after the other
constexpr int network_steps(int n)
{
    int c = 0;
    for (int p = 1; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < n; j += 2 * k)
                for (int i = 0; i < k && i + j + k < n; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) ++c;
    return c;
}

template <int AMAX>
struct Network {
    static constexpr int kSteps = network_steps(AMAX);
    unsigned char lo[kSteps], hi[kSteps];
};

template <int AMAX>
constexpr Network<AMAX> make_network()
{
    Network<AMAX> t = {};
    int c = 0;
    for (int p = 1; p < AMAX; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < AMAX; j += 2 * k)
                for (int i = 0; i < k && i + j + k < AMAX; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        t.lo[c] = (unsigned char)(i + j);
                        t.hi[c] = (unsigned char)(i + j + k);
                        ++c;
                    }
    return t;
}

static_assert(network_steps(8) == 19 && network_steps(16) == 63 && network_steps(128) == 1471, "the counts of the header comment");

template <int LO, int HI, int AMAX>
__device__ __forceinline__ int exchange(unsigned (&key)[AMAX])
{
    static_assert(LO < HI && HI < AMAX, "a step of the network");
    const unsigned a = key[LO], b = key[HI];
    key[LO] = a < b ? a : b;
    key[HI] = a < b ? b : a;
    return 0;
}

// key[] ascending, every index a constant of the instantiation
template <int AMAX, int... C>
__device__ __forceinline__ void sort_keys(unsigned (&key)[AMAX], std::integer_sequence<int, C...>)
{
    constexpr Network<AMAX> net = make_network<AMAX>();
    const int made[] = {exchange<net.lo[C], net.hi[C]>(key)...};
    (void)made;
}

// The address of a lane's access in a row: the row's wave-uniform base stays in a scalar register pair and the lane adds
// one unsigned 32-bit byte offset, the scalar-base form of global_load / global_store.  Left transparent, the compiler adds
// the lane's offset to the common part of all rows first, and every one of the AMAX loads costs a 64-bit vector add and a
// register pair.  `base` MUST be the same in every lane of the wave: the scalar constraint takes one lane's value for all.
template <typename T, typename U>
__device__ __forceinline__ T *lane_at(U *base, unsigned lane_bytes)
{
    asm("" : "+s"(base));
    asm("" : "+v"(lane_bytes));
    using GlobalByte = __attribute__((address_space(1))) unsigned char;
    return (T *)(unsigned char *)((GlobalByte *)(unsigned char *)base + lane_bytes);
}

// grid = (G groups, 16384 / (256 BINS) tiles of bins) workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD, int AMAX>
__global__ __launch_bounds__(kHoldThreads) void hold_f32_kernel(const unsigned *__restrict__ in, unsigned *__restrict__ out,
                                                                int group, int q, HoldRanks ranks)
{
    constexpr int BINS = hold_bins(AMAX, FIELD);                   // adjacent bins of this thread
    constexpr int WORDS = FIELD == 0 ? 1 : 2;                      // 32-bit words of a point in the input
    constexpr size_t kRowWords = (size_t)SA_N * WORDS;
    const size_t g = blockIdx.x;
    const unsigned unit = blockIdx.y * kHoldThreads + threadIdx.x; // the thread's 16-byte unit, or its bin where it owns one
    const unsigned at_in = BINS == 1 ? unit * (4u * WORDS) + (FIELD == 2 ? 4u : 0u) : unit * 16u;      // bytes into a row
    const unsigned *rows = in + g * (size_t)group * kRowWords;
    // the group's size once more, as a lane's value: a row's key is then chosen by a vector compare where the key is made.
    // Chosen on the scalar `group`, the AMAX / 2 conditions are formed ahead of the loads and wait for them, a register pair each
    int group_lane = group;
    asm("" : "+v"(group_lane));

    unsigned key[BINS][AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
        // a class above the smallest holds groups of more than half its keys: those rows are always there
        const bool there = (AMAX > kHoldClassMin && a < AMAX / 2) || a < group;
        const unsigned *row = rows + (size_t)(there ? a : group - 1) * kRowWords;
        unsigned w[BINS];
        if constexpr (BINS == 1) {
            w[0] = *lane_at<const unsigned>(row, at_in);
        } else {
            uint4 v = *lane_at<const uint4>(row, at_in);
            // all four words stay wanted: one 16-byte load, not a 4-byte load per word that is used
            if constexpr (FIELD != 0) asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
            if constexpr (FIELD == 0) {
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            } else if constexpr (FIELD == 1) {
                w[0] = v.x, w[1] = v.z;
            } else {
                w[0] = v.y, w[1] = v.w;
            }
        }
#pragma unroll
        for (int e = 0; e < BINS; ++e) {
            const bool mine = (AMAX > kHoldClassMin && a < AMAX / 2) || a < group_lane;
            key[e][a] = mine ? w[e] & kSignOff : kNoKey;
        }
    }

#ifndef SA_HOLD_SELECT
#pragma unroll
    for (int e = 0; e < BINS; ++e) sort_keys(key[e], std::make_integer_sequence<int, Network<AMAX>::kSteps>());
#endif

#pragma unroll
    for (int j = 0; j < SA_HOLD_Q_MAX; ++j) {
        if (j < q) {
            const int rank = ranks.r[j];
            unsigned v[BINS];
#pragma unroll
            for (int e = 0; e < BINS; ++e) {
                v[e] = 0u;
#ifndef SA_HOLD_SELECT
#pragma unroll
                for (int i = 0; i < AMAX; ++i) v[e] = rank == i ? key[e][i] : v[e];
#else
                // the other form, for measurement only: the answer from bit 30 down, the bit stays
                // when the number of keys below the threshold does not exceed the rank
#pragma unroll 1
                for (int b = 30; b >= 0; --b) {
                    const unsigned thr = v[e] | 1u << b;
                    int below = 0;
#pragma unroll
                    for (int i = 0; i < AMAX; ++i) below += key[e][i] < thr;
                    v[e] = below <= rank ? thr : v[e];
                }
#endif
            }
            unsigned *dst = out + (g * (size_t)q + (size_t)j) * (size_t)SA_N;
            if constexpr (BINS == 4)
                *lane_at<uint4>(dst, unit * 16u) = make_uint4(v[0], v[1], v[2], v[3]);
            else if constexpr (BINS == 2)
                *lane_at<uint2>(dst, unit * 8u) = make_uint2(v[0], v[1]);
            else
                *lane_at<unsigned>(dst, unit * 4u) = v[0];
        }
    }
}

template <int FIELD, int AMAX>
void launch(const void *in, float *out, int rows, int group, int q, const HoldRanks &ranks, hipStream_t stream)
{
    const dim3 grid((unsigned)(rows / group), (unsigned)(SA_N / (kHoldThreads * hold_bins(AMAX, FIELD))));
    hipLaunchKernelGGL((hold_f32_kernel<FIELD, AMAX>), grid, dim3(kHoldThreads), 0, stream, static_cast<const unsigned *>(in),
                       reinterpret_cast<unsigned *>(out), group, q, ranks);
}

template <int FIELD>
void launch_class(const void *in, float *out, int rows, int group, int q, const HoldRanks &ranks, hipStream_t stream)
{
    switch (hold_class(group)) {
        case 8: launch<FIELD, 8>(in, out, rows, group, q, ranks, stream); break;
        case 16: launch<FIELD, 16>(in, out, rows, group, q, ranks, stream); break;
        case 32: launch<FIELD, 32>(in, out, rows, group, q, ranks, stream); break;
        case 64: launch<FIELD, 64>(in, out, rows, group, q, ranks, stream); break;
        default: launch<FIELD, 128>(in, out, rows, group, q, ranks, stream); break;
    }
}

}  // namespace

extern "C" int sa_hold_version(void)
{
    return SA_HOLD_VERSION;
}

extern "C" int sa_hold_f32(const void *in, int field, float *out, int rows, int group, int q, const int32_t *ranks, void *stream)
{
    const char *why;
    const int rc = sa_hold_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, rows, group, q, ranks, &why);
    sa_hold_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    HoldRanks set = {};
    for (int j = 0; j < q; ++j) set.r[j] = ranks[j];
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_HOLD_IN_MAG: launch_class<0>(in, out, rows, group, q, set, st); break;
        case SA_HOLD_IN_POINT_PEAK: launch_class<1>(in, out, rows, group, q, set, st); break;
        default: launch_class<2>(in, out, rows, group, q, set, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_hold_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
