// harm_f32.hip -- sa_harm_f32 (include/specan_harm.h): per row of 16384 points the fundamental, the
// bins its harmonics alias to, the float64 power of the band of each, of their union, of everything but the fundamental and of
// everything but both, and the largest point outside the fundamental's band and outside all of them.  The kernel of
// libspecan_harm.so; it stands beside the chains and the other reductions and shares no text with them.
//
// One workgroup of 256 threads per row.  No set of the definition reaches past bin 8192, so a point above it is +0.0 in every
// sum and in no maximum: the kernel reads bins 0..8447 of a row, once, and holds them in registers.  In round r a thread takes
// the four adjacent bins 1024 r + 4 t .. + 3 (one 16-byte load of magnitudes, two adjacent ones of records), so the 256 bins of
// a wave in one round are one node of tree level 8: tile 4 r + wave.  Rounds 0..7 are tiles 0..31; round 8 is wave 0's alone,
// tile 32, of which bin 8192 is the one bin that can count.  Levels 0-1 of a sum are two adds in the thread, levels 2-7 an
// xor-butterfly over the wave (partner 1 and 2 by quad permutation, 4 and 8 by the mirrored half row and row -- after the
// earlier levels every lane of a mirrored block holds the same value, so lane i ^ 7 stands for lane i ^ 4 and lane i ^ 15 for
// lane i ^ 8 -- 16 and 32 by a lane permute); a maximum and a count go through the same butterfly.
//
//   A  per thread the largest (key << 32 | ~bin) of the search range, over the wave                   -> s_max[wave]
//      every wave sums its tiles unmasked                                                              -> s_tile[33]
//   -- barrier; every wave reads the fundamental and works out the ten bands in wave-uniform integers
//   B  the first and last tile of the band of the fundamental and of each harmonic are summed under the band's mask (less the
//      fundamental's band) by the wave that owns them                                                  -> s_edge[10][2]
//      every tile that holds an end of [dc, top) or of a band is classed bin by bin by its wave and summed three times, as
//      part of U, of A - F and of A - F - U                                                            -> s_part[3][33]
//      a tile that holds no end is in a set whole or not at all, which its first bin tells; either way the thread keeps the
//      two masked maxima and the count of its bins, then the wave's                                    -> s_top[2][wave], s_cnt[wave]
//   -- barrier
//   C  wave s & 3 sums levels 8..13 of set s: lane l holds tile l's node -- a masked sum of B, the unmasked sum of A where the
//      whole tile is in the set, +0.0 otherwise -- and lane 0 stores the root; wave 3 stores the sixteen words of the record
// The round that holds a band's tile is chosen by an unrolled wave-uniform compare: no register is indexed dynamically.
// Static LDS, every word written by the launch before it is read; no workspace, no atomics, no FP-mode change; every byte of
// a record is stored exactly once, and nothing outside the row is read.
#include <hip/hip_runtime.h>

#include "sa_harm.hpp"

// every sum is an addition of float64 values in the header's order
#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

constexpr int kHarmWaves = kHarmThreads / 64;
static_assert(kHarmWaves == 4, "tile 4 r + wave");

template <int CTRL> __device__ __forceinline__ u64 dpp_u64(u64 b)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, true);
    return (u64)hi << 32 | lo;
}

template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    return __builtin_bit_cast(double, dpp_u64<CTRL>(__builtin_bit_cast(u64, v)));
}

// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
constexpr int kX1 = 0xB1, kX2 = 0x4E, kX4 = 0x141, kX8 = 0x140;

// the node of level 6 above the 64 values of a wave, in every lane; every lane of the wave is active
__device__ __forceinline__ double wave_sum(double v)
{
    v = v + dpp_f64<kX1>(v);
    v = v + dpp_f64<kX2>(v);
    v = v + dpp_f64<kX4>(v);
    v = v + dpp_f64<kX8>(v);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ u64 umax(u64 a, u64 b)
{
    return a > b ? a : b;
}

__device__ __forceinline__ u64 wave_max(u64 v)
{
    v = umax(v, dpp_u64<kX1>(v));
    v = umax(v, dpp_u64<kX2>(v));
    v = umax(v, dpp_u64<kX4>(v));
    v = umax(v, dpp_u64<kX8>(v));
    v = umax(v, __shfl_xor(v, 16));
    v = umax(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ int wave_count(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, kX1, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, kX2, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, kX4, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, kX8, 0xF, 0xF, true);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// the point's value: the key as a float, widened (exact, denormals kept), squared unless it is a power already
template <int FIELD> __device__ __forceinline__ double value(unsigned key)
{
    const double a = (double)__builtin_bit_cast(float, key);
    return FIELD == SA_HARM_IN_POINT_POWER ? a : a * a;
}

// a key and its bin as one number whose order is the header's: the larger key, then the lower bin.  0 is below every one of
// them, and reads back as (+0.0, bin -1): the answer of an empty set.
__device__ __forceinline__ u64 pack(unsigned key, int bin)
{
    return (u64)key << 32 | (unsigned)~bin;
}

// lo <= i < lo + width as one unsigned compare; an empty band has width 0
__device__ __forceinline__ bool within(int i, int lo, int width)
{
    return (unsigned)(i - lo) < (unsigned)width;
}

// the bin harmonic h of the fundamental k1 aliases to
__device__ __forceinline__ int alias_bin(int h, int k1)
{
    const int m = (h * k1) & (SA_N - 1);
    return m <= SA_N / 2 ? m : SA_N - m;
}

// The sets of a row, in wave-uniform integers.  Band 0 is F, band h - 1 that of harmonic h before F is taken out; a band that
// is empty or beyond `order` is [0, 0).  `ends` has a bit for every tile that holds the first or the last bin of [dc, top) or
// of a band: in any other tile every one of these ranges lies whole or not at all.
struct Sets {
    int dc, wide;                                                  // A = [dc, dc + wide)
    int lo[SA_HARM_MAX], width[SA_HARM_MAX];
    u64 ends;
};

__device__ __forceinline__ u64 end_tiles(int lo, int width)
{
    return width > 0 ? 1ull << (lo >> 8) | 1ull << ((lo + width - 1) >> 8) : 0ull;
}

__device__ __forceinline__ Sets make_sets(const sa_harm_cfg &c, int k1)
{
    Sets s;
    s.dc = c.dc, s.wide = c.top - c.dc;
    s.ends = end_tiles(s.dc, s.wide);
#pragma unroll
    for (int j = 0; j < SA_HARM_MAX; ++j) {
        const int k = alias_bin(j + 1, k1);
        const int lo = max(k - c.span, c.dc), hi = min(k + c.span + 1, c.top);
        const bool some = j < c.order && lo < hi;
        s.lo[j] = some ? lo : 0, s.width[j] = some ? hi - lo : 0;
        s.ends |= end_tiles(s.lo[j], s.width[j]);
    }
    return s;
}

// which of the three wide sets bin i is in: bit 0 U, bit 1 A - F, bit 2 A - F - U
__device__ __forceinline__ int classes(const Sets &s, int i)
{
    const bool f = within(i, s.lo[0], s.width[0]);
    bool u = false;
#pragma unroll
    for (int j = 1; j < SA_HARM_MAX; ++j) u = u || within(i, s.lo[j], s.width[j]);
    u = u && !f;
    const bool rest = within(i, s.dc, s.wide) && !f;
    return (u ? 1 : 0) | (rest ? 2 : 0) | (rest && !u ? 4 : 0);
}

// the four keys of round `r` (wave-uniform) of this thread
__device__ __forceinline__ void pick(const unsigned (&pt)[kHarmRounds][4], int r, unsigned (&p)[4])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = 0u;
#pragma unroll
    for (int i = 0; i < kHarmRounds; ++i)
        if (i == r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = pt[i][e];
        }
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD>
__global__ __launch_bounds__(kHarmThreads) void harm_f32_kernel(const uint4 *__restrict__ in, unsigned char *__restrict__ out, sa_harm_cfg cfg)
{
    __shared__ u64 s_max[kHarmWaves];                              // A: the wave's largest of the search range
    __shared__ double s_tile[kHarmTiles];                          // A: the unmasked sum of every tile
    __shared__ double s_edge[SA_HARM_MAX][2];                      // B: a band's first and (where it is another) last tile, masked
    __shared__ double s_part[3][kHarmTiles];                       // B: the tiles with an end in them, as part of the three wide sets
    __shared__ u64 s_top[2][kHarmWaves];                           // B: the wave's largest of A - F and of A - F - U
    __shared__ int s_cnt[kHarmWaves];                              // B: the wave's bins of A - F - U
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    constexpr int UNITS = FIELD == SA_HARM_IN_MAG ? 1 : 2;         // 16-byte loads per thread and round
    const uint4 *src = in + row * (size_t)(SA_N / 4 * UNITS);

    // the keys: the sign is cleared once, here
    unsigned pt[kHarmRounds][4];
#pragma unroll
    for (int r = 0; r < kHarmRounds; ++r) {
        pt[r][0] = pt[r][1] = pt[r][2] = pt[r][3] = 0u;
        if (r < kHarmRounds - 1 || wave == 0) {
            const size_t u = (size_t)UNITS * ((size_t)t + (size_t)kHarmThreads * r);
            if constexpr (FIELD == SA_HARM_IN_MAG) {
                const uint4 v = src[u];
                pt[r][0] = v.x, pt[r][1] = v.y, pt[r][2] = v.z, pt[r][3] = v.w;
            } else {
                const uint4 v0 = src[u], v1 = src[u + 1];
                if constexpr (FIELD == SA_HARM_IN_POINT_PEAK) {
                    pt[r][0] = v0.x, pt[r][1] = v0.z, pt[r][2] = v1.x, pt[r][3] = v1.z;
                } else {
                    pt[r][0] = v0.y, pt[r][1] = v0.w, pt[r][2] = v1.y, pt[r][3] = v1.w;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) pt[r][e] &= 0x7FFFFFFFu;
        }
    }

    // A: a given fundamental is a search range of one bin
    {
        const int lo = cfg.fund >= 0 ? cfg.fund : cfg.lo, width = cfg.fund >= 0 ? 1 : cfg.hi - cfg.lo;
        u64 best = 0;
#pragma unroll
        for (int r = 0; r < kHarmRounds; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bin = 4 * kHarmThreads * r + 4 * t + e;
                if (within(bin, lo, width)) best = umax(best, pack(pt[r][e], bin));
            }
        best = wave_max(best);
        if (lane == 0) s_max[wave] = best;
    }
#pragma unroll
    for (int r = 0; r < kHarmRounds; ++r)
        if (r < kHarmRounds - 1 || wave == 0) {
            const double q = (value<FIELD>(pt[r][0]) + value<FIELD>(pt[r][1])) + (value<FIELD>(pt[r][2]) + value<FIELD>(pt[r][3]));
            const double s = wave_sum(q);
            if (lane == 0) s_tile[4 * r + wave] = s;
        }
    __syncthreads();

    const u64 first = umax(umax(s_max[0], s_max[1]), umax(s_max[2], s_max[3]));
    const unsigned key1 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(first >> 32));
    const int k1 = __builtin_amdgcn_readfirstlane((int)~(unsigned)first);
    const Sets sets = make_sets(cfg, k1);

    // B: the bands
#pragma unroll
    for (int j = 0; j < SA_HARM_MAX; ++j)
        if (sets.width[j] > 0) {
            const int tl = sets.lo[j] >> 8, th = (sets.lo[j] + sets.width[j] - 1) >> 8;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int tile = e ? th : tl;
                if ((e == 0 || th != tl) && (tile & 3) == wave) {
                    unsigned p[4];
                    pick(pt, tile >> 2, p);
                    double w[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int bin = kHarmTile * tile + 4 * lane + i;
                        const bool in_it = within(bin, sets.lo[j], sets.width[j]) && (j == 0 || !within(bin, sets.lo[0], sets.width[0]));
                        w[i] = in_it ? value<FIELD>(p[i]) : 0.0;
                    }
                    const double s = wave_sum((w[0] + w[1]) + (w[2] + w[3]));
                    if (lane == 0) s_edge[j][e] = s;
                }
            }
        }

    // B: the wide sets, the maxima and the count
    {
        u64 spur = 0, other = 0;
        int count = 0;
#pragma unroll
        for (int r = 0; r < kHarmRounds; ++r)
            if (r < kHarmRounds - 1 || wave == 0) {
                const int tile = 4 * r + wave;
                const int bin0 = kHarmTile * tile + 4 * lane;
                if (sets.ends >> tile & 1) {
                    double w[3][4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = classes(sets, bin0 + e);
                        const double v = value<FIELD>(pt[r][e]);
#pragma unroll
                        for (int a = 0; a < 3; ++a) w[a][e] = c >> a & 1 ? v : 0.0;
                        if (c & 2) spur = umax(spur, pack(pt[r][e], bin0 + e));
                        if (c & 4) other = umax(other, pack(pt[r][e], bin0 + e)), ++count;
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const double s = wave_sum((w[a][0] + w[a][1]) + (w[a][2] + w[a][3]));
                        if (lane == 0) s_part[a][tile] = s;
                    }
                } else {
                    const int c = __builtin_amdgcn_readfirstlane(classes(sets, kHarmTile * tile));
                    if (c & 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) spur = umax(spur, pack(pt[r][e], bin0 + e));
                    }
                    if (c & 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) other = umax(other, pack(pt[r][e], bin0 + e));
                        count += 4;
                    }
                }
            }
        spur = wave_max(spur), other = wave_max(other), count = wave_count(count);
        if (lane == 0) s_top[0][wave] = spur, s_top[1][wave] = other, s_cnt[wave] = count;
    }
    __syncthreads();

    // C
    unsigned char *rec = out + row * sizeof(sa_harm_row);
    double *sums = reinterpret_cast<double *>(rec);
#pragma unroll
    for (int j = 0; j < SA_HARM_MAX; ++j)
        if ((j & 3) == wave) {
            double root = 0.0;
            if (sets.width[j] > 0) {
                const int tl = sets.lo[j] >> 8, th = (sets.lo[j] + sets.width[j] - 1) >> 8;
                double mine = 0.0;
                if (lane == th && th != tl) mine = s_edge[j][1];   // with tl == th the one sum is in slot 0, slot 1 unwritten
                if (lane == tl) mine = s_edge[j][0];
                root = wave_sum(mine);
            }
            if (lane == 0) sums[j] = root;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (((SA_HARM_MAX + a) & 3) == wave) {
            double mine = 0.0;
            if (lane < kHarmTiles) {
                if (sets.ends >> lane & 1)
                    mine = s_part[a][lane];
                else if (classes(sets, kHarmTile * lane) >> a & 1)
                    mine = s_tile[lane];
            }
            const double root = wave_sum(mine);
            if (lane == 0) sums[SA_HARM_MAX + a] = root;
        }
    if (wave == kHarmWaves - 1 && lane < 16) {
        const u64 spur = umax(umax(s_top[0][0], s_top[0][1]), umax(s_top[0][2], s_top[0][3]));
        const u64 other = umax(umax(s_top[1][0], s_top[1][1]), umax(s_top[1][2], s_top[1][3]));
        const int count = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        unsigned word = lane < cfg.order ? (unsigned)alias_bin(lane + 1, k1) : ~0u;       // bin[10]
        if (lane == 10) word = key1;                               // fund
        if (lane == 11) word = (unsigned)(spur >> 32);             // spur
        if (lane == 12) word = (unsigned)(other >> 32);            // nonharm
        if (lane == 13) word = ~(unsigned)spur;                    // spur_bin
        if (lane == 14) word = ~(unsigned)other;                   // nonharm_bin
        if (lane == 15) word = (unsigned)count;                    // n_noise
        reinterpret_cast<unsigned *>(rec + offsetof(sa_harm_row, bin))[lane] = word;
    }
}

template <int FIELD> void launch(const void *in, sa_harm_row *out, int rows, const sa_harm_cfg &cfg, hipStream_t stream)
{
    hipLaunchKernelGGL((harm_f32_kernel<FIELD>), dim3((unsigned)rows), dim3(kHarmThreads), 0, stream, static_cast<const uint4 *>(in),
                       reinterpret_cast<unsigned char *>(out), cfg);
}

}  // namespace

extern "C" int sa_harm_version(void)
{
    return SA_HARM_VERSION;
}

extern "C" int sa_harm_f32(const void *in, int field, sa_harm_row *out, int rows, const sa_harm_cfg *cfg, void *stream)
{
    const char *why;
    const int rc = sa_harm_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, rows, cfg, &why);
    sa_harm_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_HARM_IN_MAG: launch<0>(in, out, rows, *cfg, st); break;
        case SA_HARM_IN_POINT_PEAK: launch<1>(in, out, rows, *cfg, st); break;
        default: launch<2>(in, out, rows, *cfg, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_harm_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
