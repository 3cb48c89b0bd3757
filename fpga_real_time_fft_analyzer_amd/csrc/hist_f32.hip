// hist_f32.hip -- sa_hist_f32 (include/specan_hist.h): for every group of A rows of 16384 float32
// points, every column of W bins of [lo, hi) and every one of L levels, the number of points of that cell.  The kernel of
// libspecan_hist.so; it stands beside the chains, the fold, the peak table and the rank library and shares no text with them.
//
// A workgroup owns one group and one tile of 256 adjacent bins over ALL A rows of the group, so the tile's counters are its
// own: they live in LDS, the launch zeroes them, and at the end the workgroup stores them -- one contiguous block of the
// output, every counter once, with plain stores.  In this form: no global atomic, no workspace, nothing written twice.
// Wave w of the n waves takes the rows w, w + n, w + 2n, ... of the group; a lane holds a quad of bins per row (one 16-byte
// unit, so that the lanes of a wave read 1 KiB of adjacent bytes per instruction) and a wave asks for eight rows at a time.
//
// G x 64 owners are too few for 256 compute units when G is 1 or 2 (measured: 262 us for 256 MiB at G = 1 against 72 us at
// G = 16).  There, and only where a group has 64 rows or more, the group's rows are cut into S slices,
// one workgroup each, which add their counters that are not zero to the output with global_atomic_add_u32, behind
// hist_zero_kernel on the same stream, which zeroes the output (a launch of the library's own: it is captured and replayed
// like the count).  Integer sums: the result is the same bits in any order.
//
// The level of a key is a search, not arithmetic: the L - 1 edge keys, padded with 0xFFFFFFFF to 2^STEPS - 1, arrive by value
// as a complete binary tree in level order (node i has the children 2i and 2i + 1), are put into LDS once, and a point walks
// down STEPS = ceil(log2 L) nodes: i = 2i + (node[i] <= key).  The leaf it falls off at is 2^STEPS + level.  The nodes of
// one depth are adjacent words, so the lanes of a step read distinct banks or the same word.
//
// Counters: word level * (Ct + 1) + slot, Ct = 256 / W columns in the tile.  The slot of a column is chosen so that the lanes
// of one ds_add sit on consecutive words when their levels agree: at W = 1 the column 4 lane + e has the slot 64 e + lane, at
// W = 2 the column 2 lane + (e >> 1) the slot 64 (e >> 1) + lane, at W >= 4 the slot is the column.  The odd stride lets the
// store phase, which walks the levels of a column, read distinct banks as well.  At W >= 8, W / 4 adjacent lanes share a
// column: where their levels agree too they add to one word, and the LDS takes those adds one after the other.
// Integer counts only: nothing depends on an order.  No FP-mode change, no scratch; every LDS word that is read is written
// by the launch first, and nothing outside the tensors is touched.
#include <hip/hip_runtime.h>

#include "sa_hist.hpp"

namespace {

constexpr unsigned kSignOff = 0x7FFFFFFFu;                     // a key: the float's bits without the sign
constexpr unsigned kNoEdge = 0xFFFFFFFFu;                      // pads the edge tree: above every key
constexpr int kHistFlight = 8;                                 // 16-byte loads a lane has in flight
constexpr int kHistUnits = SA_N / 4;                           // 16-byte units of a row
constexpr int kHistWords = SA_HIST_LEVELS_MAX * (kHistTile + 1);       // the counters at W = 1, L = 64: 65792 bytes
static_assert(kHistWords % 4 == 0, "the counters are zeroed in 16-byte units");

// the edge keys as a tree in level order, by value among the kernel's arguments: stream-ordered with the launch, and part of
// a captured graph's node.  node[0] is not used.
struct EdgeTree {
    unsigned node[SA_HIST_LEVELS_MAX];
};

// where the counters of local column `lc` of the tile stand within a level's Ct words
__device__ __forceinline__ unsigned slot_of(unsigned lc, int log2w)
{
    if (log2w >= 2) return lc;
    const int k = 2 - log2w;
    return ((lc & ((1u << k) - 1u)) << 6) + (lc >> k);
}

// One unit of four bins: `one[e]` is 1 for a bin inside [lo, hi) and 0 for one outside, which then adds nothing to a counter of
// its own tile -- no branch and no lane mask around the four searches or the adds.  The walk keeps a = 4 i, the node's byte
// offset, so that a step is a read, a compare, a select and one shift-or; it ends at a = 4 (2^STEPS + level), and the
// counter's byte offset is a stride + at[e], at[e] = 4 slot - 4 2^STEPS stride (modulo 2^32: the sum is never negative).
template <int STEPS>
__device__ __forceinline__ void count_unit(const uint4 v, unsigned *s_cnt, const unsigned *s_edge, const unsigned (&at)[4],
                                           const unsigned (&one)[4], int log2ct)
{
    const unsigned key[4] = {v.x & kSignOff, v.y & kSignOff, v.z & kSignOff, v.w & kSignOff};
    const char *edge = reinterpret_cast<const char *>(s_edge);
    unsigned a[4] = {4u, 4u, 4u, 4u};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned node = *reinterpret_cast<const unsigned *>(edge + a[e]);
            a[e] = (a[e] << 1) | (node <= key[e] ? 4u : 0u);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned at_level = (a[e] << log2ct) + a[e];        // a (Ct + 1): a shift and an add, Ct being a power of two
        unsigned *cell = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(s_cnt) + (at_level + at[e]));
        __hip_atomic_fetch_add(cell, one[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// grid = (G, tiles that meet [lo, hi), slices) workgroups of 64 n threads, n = 4..16 waves; slice s of S has the rows
// [A s / S, A (s + 1) / S) of its group.  With S = 1 the workgroup stores its counters; with S > 1 it adds those that are not
// zero to an output that hist_zero_kernel zeroed on the same stream.  Every offset into the tensors is a size_t.
// Eight waves per SIMD (64 VGPRs): two workgroups of 16 waves on a compute unit, whose 160 KiB of LDS hold two sets of counters.
template <int STEPS>
__global__ __launch_bounds__(64 * kHistWavesMax, 8) void hist_f32_kernel(const uint4 *__restrict__ in, unsigned *__restrict__ out,
                                                                      int group, int log2w, int nlev, unsigned inv_nlev, int lo,
                                                                      int hi, EdgeTree tree)
{
    __shared__ alignas(16) unsigned s_cnt[kHistWords];
    __shared__ unsigned s_edge[SA_HIST_LEVELS_MAX];
    const int t = threadIdx.x, lane = t & 63, threads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), waves = threads >> 6;
    const size_t g = blockIdx.x;
    const int slices = (int)gridDim.z;
    const int row0 = (int)((long long)group * (long long)blockIdx.z / slices);
    const int row1 = (int)((long long)group * ((long long)blockIdx.z + 1) / slices);
    const int tile = (lo / kHistTile) + (int)blockIdx.y;
    const int ct = kHistTile >> log2w;                             // columns of a whole tile
    const unsigned stride = (unsigned)ct + 1u;
    const int used = nlev * (int)stride;

    // the launch zeroes its counters itself and plants the edge tree
    for (int u = t; 4 * u < used; u += threads) reinterpret_cast<uint4 *>(s_cnt)[u] = make_uint4(0u, 0u, 0u, 0u);
    if (t < SA_HIST_LEVELS_MAX) s_edge[t] = tree.node[t];
    __syncthreads();

    const int bin0 = tile * kHistTile + 4 * lane;                  // the lane's quad of bins
    const unsigned width = (unsigned)(hi - lo);                    // lo <= bin < hi as one unsigned compare
    unsigned at[4], one[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        at[e] = 4u * slot_of((unsigned)(4 * lane + e) >> log2w, log2w) - (4u << STEPS) * stride;
        one[e] = (unsigned)(bin0 + e - lo) < width ? 1u : 0u;
    }
    const uint4 *src = in + g * (size_t)group * (size_t)kHistUnits + (size_t)(tile * (kHistTile / 4) + lane);
    int r = row0 + wave;
    // eight rows of the wave at a time while it has eight left, then one at a time
    for (; r + (kHistFlight - 1) * waves < row1; r += kHistFlight * waves) {
        uint4 got[kHistFlight];
#pragma unroll
        for (int b = 0; b < kHistFlight; ++b) got[b] = src[(size_t)(r + b * waves) * (size_t)kHistUnits];
#pragma unroll
        for (int b = 0; b < kHistFlight; ++b) count_unit<STEPS>(got[b], s_cnt, s_edge, at, one, 8 - log2w);
    }
    for (; r < row1; r += waves) count_unit<STEPS>(src[(size_t)r * (size_t)kHistUnits], s_cnt, s_edge, at, one, 8 - log2w);
    __syncthreads();

    // the tile's columns inside [lo, hi) are one contiguous block of the output: with one slice every counter is stored once
    const int first = max(lo - tile * kHistTile, 0) >> log2w, last = min(hi - tile * kHistTile, kHistTile) >> log2w;
    const int n_out = (last - first) * nlev;
    const size_t columns = (size_t)((hi - lo) >> log2w);
    const size_t column0 = (size_t)((tile * kHistTile + (first << log2w) - lo) >> log2w);
    unsigned *dst = out + (g * columns + column0) * (size_t)nlev;
    for (int o = t; o < n_out; o += threads) {
        const unsigned c = __umulhi((unsigned)o, inv_nlev);        // o / nlev: exact for o < 2^14 with inv = 2^32 / nlev + 1
        const unsigned l = (unsigned)o - c * (unsigned)nlev;
        const unsigned count = s_cnt[l * stride + slot_of((unsigned)first + c, log2w)];
        if (slices == 1)
            dst[o] = count;
        else if (count != 0u)
            __hip_atomic_fetch_add(&dst[o], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the output of the sliced form, zeroed on the call's stream ahead of the count: one word per thread
constexpr int kHistZeroThreads = 256;
__global__ __launch_bounds__(kHistZeroThreads) void hist_zero_kernel(unsigned *__restrict__ out, size_t words)
{
    const size_t i = (size_t)blockIdx.x * (size_t)kHistZeroThreads + (size_t)threadIdx.x;
    if (i < words) out[i] = 0u;
}

// the sorted keys a[0..n), n = 2^steps - 1, as the in-order walk of the complete tree whose node i has the children 2i, 2i + 1
void plant(EdgeTree &tree, const unsigned *a, int n, int i, int &next)
{
    if (i > n) return;
    plant(tree, a, n, 2 * i, next);
    tree.node[i] = a[next++];
    plant(tree, a, n, 2 * i + 1, next);
}

template <int STEPS>
void launch(const float *in, uint32_t *out, dim3 grid, int threads, int group, int log2w, int nlev, int lo, int hi,
            const EdgeTree &tree, hipStream_t stream)
{
    const unsigned inv = (unsigned)(0x100000000ull / (unsigned)nlev) + 1u;
    hipLaunchKernelGGL(hist_f32_kernel<STEPS>, grid, dim3((unsigned)threads), 0, stream, reinterpret_cast<const uint4 *>(in), out,
                       group, log2w, nlev, inv, lo, hi, tree);
}

}  // namespace

extern "C" int sa_hist_version(void)
{
    return SA_HIST_VERSION;
}

extern "C" int sa_hist_f32(const float *in, uint32_t *out, int rows, int group, int log2w, int nlev, const float *edges, int lo,
                           int hi, void *stream)
{
    const char *why;
    const int rc = sa_hist_check_call((uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, rows, group, log2w, nlev, edges, lo, hi, &why);
    sa_hist_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    int steps = 1;
    while ((1 << steps) < nlev) ++steps;
    unsigned sorted[SA_HIST_LEVELS_MAX];
    const int n = (1 << steps) - 1;
    for (int j = 0; j < n; ++j) {
        unsigned u = kNoEdge;
        if (j < nlev - 1) __builtin_memcpy(&u, &edges[j], sizeof u);
        sorted[j] = u;
    }
    EdgeTree tree;
    for (int j = 0; j < SA_HIST_LEVELS_MAX; ++j) tree.node[j] = kNoEdge;
    int next = 0;
    plant(tree, sorted, n, 1, next);
    const int tiles = (hi - 1) / kHistTile - lo / kHistTile + 1;
    // G x tiles workgroups that own their counters; where those are too few to fill the device and the groups are long, each
    // group's rows are cut into slices that merge into a zeroed output (include/specan_hist.h: the two operations of the call)
    const long long owners = (long long)(rows / group) * tiles;
    int slices = 1;
    if (owners < kHistOwnersFew) {
        const int aim = (int)((kHistOwnersAim + owners - 1) / owners), most = group / kHistSliceRowsMin;
        slices = aim < most ? aim : most;
        if (slices < 2) slices = 1;
    }
    const dim3 grid((unsigned)(rows / group), (unsigned)tiles, (unsigned)slices);
    const int per = group / slices;                               // rows of the shortest slice
    const int waves = per < kHistWavesMin ? kHistWavesMin : per > kHistWavesMax ? kHistWavesMax : per;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (slices > 1) {
        // fewer than 256 tiles of at most 16384 counters: at most 2^22 words, 2^14 workgroups
        const size_t words = (size_t)(rows / group) * (size_t)((hi - lo) >> log2w) * (size_t)nlev;
        hipLaunchKernelGGL(hist_zero_kernel, dim3((unsigned)((words + kHistZeroThreads - 1) / kHistZeroThreads)),
                           dim3(kHistZeroThreads), 0, st, out, words);
    }
    switch (steps) {
        case 1: launch<1>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
        case 2: launch<2>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
        case 3: launch<3>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
        case 4: launch<4>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
        case 5: launch<5>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
        default: launch<6>(in, out, grid, 64 * waves, group, log2w, nlev, lo, hi, tree, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_hist_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
