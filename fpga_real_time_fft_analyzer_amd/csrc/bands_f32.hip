// bands_f32.hip -- sa_bands_f32 (include/specan_bands.h): the float64 power of up to 16 bands of each
// row of 16384 points, float32 magnitudes or one float of 8-byte (peak, power) records, summed by the balanced pair tree of
// the header, and the bins at which a band's cumulative power crosses up to 4 fractions of it, found by descending that tree.
// The kernel of libspecan_bands.so; it stands beside the chains and the other reductions and shares no text with them.
//
// One workgroup of 256 threads per row, and the row is read from memory once and held in registers: in round r a thread takes
// the four adjacent bins 1024 r + 4 t .. + 3 (one 16-byte load of magnitudes, two adjacent ones of records), so the lanes of a
// wave read adjacent bytes and the 256 bins of a wave in one round are one node of tree level 8: tile 4 r + wave.  Levels 0-1
// are two adds in the thread; levels 2-7 an xor-butterfly over the wave on the two halves of a double -- partner 1 and 2 by
// quad permutation, 4 and 8 by the mirrored half row and row (after the earlier levels every lane of a mirrored block holds
// the same sum, so lane i ^ 7 stands for lane i ^ 4 and lane i ^ 15 for lane i ^ 8), 16 and 32 by a lane permute.  IEEE
// addition is commutative, so every lane of a group ends with the bits of the group's node (a NaN may differ in its payload;
// only isnan is specified).
//
//   A  every wave sums its 16 tiles unmasked, once for all bands                                     -> s_tile[64]
//   B  a band's first and last tile are summed again under the band's mask by the wave that owns them  -> s_edge[band][2]
//      (a tile wholly inside a band masks nothing and gives the bits of A; which tile is an edge is wave-uniform)
//   C  wave j & 3 sums levels 8..13 of band j: lane l holds tile l's node -- the edge sums, the unmasked sum between them,
//      +0.0 outside -- and the butterfly leaves every node of levels 8..14 in the lanes; lane 0 stores the root, and the
//      descent of levels 13..8 reads its left children with v_readlane                                -> s_e, s_t, s_k
//   D  the wave that owns the tile a descent arrived at sums it under the band's mask, keeping the nodes of levels 2..7 in
//      its lanes, descends them and the two levels inside a lane, and one lane stores the bin
// with a barrier in front of C and of D.  The round that holds a tile is chosen by an unrolled wave-uniform compare: no
// register is indexed dynamically.  Static LDS of 2 KiB (768 bytes without crossings), every word written by the launch
// before it is read; no workspace, no atomics, no FP-mode change; every output element is stored exactly once, and nothing
// outside the row is read.
#include <hip/hip_runtime.h>

#include "sa_bands.hpp"

// the header fixes every rounding: t = fracs[q] * S is rounded before it is compared
#pragma clang fp contract(off)

namespace {

constexpr int kBandsWaves = kBandsThreads / 64;
static_assert(kBandsWaves == 4, "tile 4 r + wave");

// the bands and the fractions, by value among the kernel's arguments: stream-ordered with the launch, and part of a captured
// graph's node
struct BandSet {
    sa_band b[SA_BANDS_MAX];
};
struct FracSet {
    double f[SA_BANDS_Q_MAX];
};

template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// the double lane `lane` (wave-uniform) holds
__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// Six levels of the tree over the 64 lanes of a wave: n[s] is the node of the 2^s adjacent lanes this lane is in, the same
// bits in each of them; n[6] is the wave's total.  Every lane of the wave is active.
struct Nodes {
    double n[7];
};

__device__ __forceinline__ Nodes wave_tree(double mine)
{
    Nodes x;
    x.n[0] = mine;
    x.n[1] = x.n[0] + dpp_f64<0xB1>(x.n[0]);                       // quad_perm [1,0,3,2]: lane ^ 1
    x.n[2] = x.n[1] + dpp_f64<0x4E>(x.n[1]);                       // quad_perm [2,3,0,1]: lane ^ 2
    x.n[3] = x.n[2] + dpp_f64<0x141>(x.n[2]);                      // row_half_mirror: lane ^ 7, the bits of lane ^ 4
    x.n[4] = x.n[3] + dpp_f64<0x140>(x.n[3]);                      // row_mirror: lane ^ 15, the bits of lane ^ 8
    x.n[5] = x.n[4] + __shfl_xor(x.n[4], 16);
    x.n[6] = x.n[5] + __shfl_xor(x.n[5], 32);
    return x;
}

// Six steps of the header's descent through the nodes a wave_tree left in the lanes: from node k of the level above n[5] to
// one of its 64 descendants at the level of n[0].  All operands are wave-uniform.
__device__ __forceinline__ int descend(const Nodes &x, double t, double &E)
{
    int k = 0;
#pragma unroll
    for (int s = 5; s >= 0; --s) {
        const double L = readlane_f64(x.n[s], (2 * k) << s);
        const double EL = E + L;
        const bool left = EL >= t;
        E = left ? E : EL;
        k = __builtin_amdgcn_readfirstlane(left ? 2 * k : 2 * k + 1);
    }
    return k;
}

// the point's value: the float with its sign cleared, widened (exact, denormals kept), squared unless it is a power already
template <int FIELD> __device__ __forceinline__ double value(unsigned bits)
{
    const double a = (double)__builtin_bit_cast(float, bits & 0x7FFFFFFFu);
    return FIELD == SA_BANDS_IN_POINT_POWER ? a : a * a;
}

struct Quad {
    double w[4];
};

// the four values of round `r` (wave-uniform) of this thread under the band's mask; `first` is the bin of w[0]
template <int FIELD>
__device__ __forceinline__ Quad masked_quad(const unsigned (&pt)[kBandsRounds][4], int r, int first, int lo, int hi)
{
    unsigned p[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kBandsRounds; ++i)
        if (i == r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = pt[i][e];
        }
    const unsigned width = (unsigned)(hi - lo);                    // lo <= bin < hi as one unsigned compare
    Quad q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q.w[e] = (unsigned)(first + e - lo) < width ? value<FIELD>(p[e]) : 0.0;
    return q;
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD, bool CROSS>
__global__ __launch_bounds__(kBandsThreads) void bands_f32_kernel(const uint4 *__restrict__ in, double *__restrict__ power,
                                                                  int *__restrict__ cross, int nb, int nq, BandSet bands, FracSet fracs)
{
    __shared__ double s_tile[kBandsTiles];                         // A: the unmasked sum of every tile
    __shared__ double s_edge[SA_BANDS_MAX][2];                     // B: a band's first and (where it is another) last tile, masked
    __shared__ double s_e[SA_BANDS_MAX][SA_BANDS_Q_MAX];           // C: the power left of the tile a descent arrived at ...
    __shared__ double s_t[SA_BANDS_MAX][SA_BANDS_Q_MAX];           // ... its target ...
    __shared__ int s_k[SA_BANDS_MAX][SA_BANDS_Q_MAX];              // ... and the tile
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    constexpr int UNITS = FIELD == SA_BANDS_IN_MAG ? 1 : 2;        // 16-byte loads per thread and round
    const uint4 *src = in + row * (size_t)(SA_N / 4 * UNITS);

    unsigned pt[kBandsRounds][4];
#pragma unroll
    for (int r = 0; r < kBandsRounds; ++r) {
        const size_t u = (size_t)UNITS * ((size_t)t + (size_t)kBandsThreads * r);
        if constexpr (FIELD == SA_BANDS_IN_MAG) {
            const uint4 v = src[u];
            pt[r][0] = v.x, pt[r][1] = v.y, pt[r][2] = v.z, pt[r][3] = v.w;
        } else {
            const uint4 v0 = src[u], v1 = src[u + 1];
            if constexpr (FIELD == SA_BANDS_IN_POINT_PEAK) {
                pt[r][0] = v0.x, pt[r][1] = v0.z, pt[r][2] = v1.x, pt[r][3] = v1.z;
            } else {
                pt[r][0] = v0.y, pt[r][1] = v0.w, pt[r][2] = v1.y, pt[r][3] = v1.w;
            }
        }
    }

    // A
#pragma unroll
    for (int r = 0; r < kBandsRounds; ++r) {
        const double q = (value<FIELD>(pt[r][0]) + value<FIELD>(pt[r][1])) + (value<FIELD>(pt[r][2]) + value<FIELD>(pt[r][3]));
        const Nodes x = wave_tree(q);
        if (lane == 0) s_tile[4 * r + wave] = x.n[6];
    }

    // B
#pragma unroll 1
    for (int j = 0; j < nb; ++j) {
        const int lo = bands.b[j].lo, hi = bands.b[j].hi;
        const int tl = lo >> 8, th = (hi - 1) >> 8;
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
            const int tile = e ? th : tl;
            if ((e == 0 || th != tl) && (tile & 3) == wave) {
                const Quad q = masked_quad<FIELD>(pt, tile >> 2, kBandsTile * tile + 4 * lane, lo, hi);
                const Nodes x = wave_tree((q.w[0] + q.w[1]) + (q.w[2] + q.w[3]));
                if (lane == 0) s_edge[j][e] = x.n[6];
            }
        }
    }
    __syncthreads();

    // C
#pragma unroll 1
    for (int j = wave; j < nb; j += kBandsWaves) {
        const int lo = bands.b[j].lo, hi = bands.b[j].hi;
        const int tl = lo >> 8, th = (hi - 1) >> 8;
        double mine = 0.0;
        if (lane > tl && lane < th) mine = s_tile[lane];
        if (lane == th && th != tl) mine = s_edge[j][1];           // with tl == th the one sum is in slot 0, slot 1 unwritten
        if (lane == tl) mine = s_edge[j][0];
        const Nodes x = wave_tree(mine);
        const double S = x.n[6];
        if (lane == 0) power[row * (size_t)nb + (size_t)j] = S;
        if constexpr (CROSS) {
#pragma unroll
            for (int q = 0; q < SA_BANDS_Q_MAX; ++q)
                if (q < nq) {
                    const double target = fracs.f[q] * S;
                    double E = 0.0;
                    const int k = descend(x, target, E);
                    if (lane == 0) s_e[j][q] = E, s_t[j][q] = target, s_k[j][q] = k;
                }
        }
    }

    // D
    if constexpr (CROSS) {
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < nb; ++j) {
            const int lo = bands.b[j].lo, hi = bands.b[j].hi;
            int have = -1;                                         // the tile whose nodes under this band's mask are in x
            Quad w = {};
            Nodes x = {};
#pragma unroll
            for (int q = 0; q < SA_BANDS_Q_MAX; ++q)
                if (q < nq) {
                    const int tile = __builtin_amdgcn_readfirstlane(s_k[j][q]);
                    if ((tile & 3) == wave) {
                        if (tile != have) {
                            w = masked_quad<FIELD>(pt, tile >> 2, kBandsTile * tile + 4 * lane, lo, hi);
                            x = wave_tree((w.w[0] + w.w[1]) + (w.w[2] + w.w[3]));
                            have = tile;
                        }
                        const double target = s_t[j][q];
                        double E = s_e[j][q];
                        const int c = descend(x, target, E);       // levels 7..2: the lane whose quad holds the bin
                        const double w0 = readlane_f64(w.w[0], c), w1 = readlane_f64(w.w[1], c);
                        const double w2 = readlane_f64(w.w[2], c), w3 = readlane_f64(w.w[3], c);
                        const double pair = E + (w0 + w1);         // level 1
                        const bool lower = pair >= target;
                        E = lower ? E : pair;
                        const double first = lower ? w0 : w2, second = lower ? w1 : w3;
                        const double one = E + first;              // level 0
                        const bool even = one >= target;
                        E = even ? E : one;
                        const int k = kBandsTile * tile + 4 * c + (lower ? 0 : 2) + (even ? 0 : 1);
                        const bool reached = E + (even ? first : second) >= target;
                        const int bin = k < lo ? lo : k > hi - 1 ? hi - 1 : k;
                        if (lane == 0) cross[(row * (size_t)nb + (size_t)j) * (size_t)nq + (size_t)q] = reached ? bin : -1;
                    }
                }
        }
    }
}

template <int FIELD>
void launch(const void *in, double *power, int32_t *cross, int rows, int nb, int nq, const BandSet &bands, const FracSet &fracs,
            hipStream_t stream)
{
    if (nq > 0)
        hipLaunchKernelGGL((bands_f32_kernel<FIELD, true>), dim3((unsigned)rows), dim3(kBandsThreads), 0, stream,
                           static_cast<const uint4 *>(in), power, cross, nb, nq, bands, fracs);
    else
        hipLaunchKernelGGL((bands_f32_kernel<FIELD, false>), dim3((unsigned)rows), dim3(kBandsThreads), 0, stream,
                           static_cast<const uint4 *>(in), power, cross, nb, nq, bands, fracs);
}

}  // namespace

extern "C" int sa_bands_version(void)
{
    return SA_BANDS_VERSION;
}

extern "C" int sa_bands_f32(const void *in, int field, double *power, int32_t *cross, int rows, int nb, const sa_band *bands, int nq,
                            const double *fracs, void *stream)
{
    const char *why;
    const int rc = sa_bands_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)power, (uint64_t)(uintptr_t)cross, rows,
                                       nb, bands, nq, fracs, &why);
    sa_bands_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    BandSet bs = {};
    FracSet fs = {};
    for (int j = 0; j < SA_BANDS_MAX; ++j) bs.b[j] = bands[j < nb ? j : 0];          // the unused slots repeat band 0
    for (int q = 0; q < nq; ++q) fs.f[q] = fracs[q];
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_BANDS_IN_MAG: launch<0>(in, power, cross, rows, nb, nq, bs, fs, st); break;
        case SA_BANDS_IN_POINT_PEAK: launch<1>(in, power, cross, rows, nb, nq, bs, fs, st); break;
        default: launch<2>(in, power, cross, rows, nb, nq, bs, fs, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_bands_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
