// signals_f32.hip -- sa_signals_f32 (include/specan_signals.h): per row of 16384 points the runs of
// bins that stand above the row's threshold, runs at most `gap` bins apart joined, runs narrower than `min_width` dropped; of
// the first k the bounds, the largest point with its bin and the float64 power, and the row's counts.  The kernel of
// libspecan_signals.so; it stands beside the chains and the other reductions and shares no text with them.
//
// One workgroup of 256 threads per row, which it reads once and holds in registers.  In round r a thread takes the four
// adjacent bins 1024 r + 4 t .. + 3 (one 16-byte load of magnitudes, two adjacent ones of records), so the 256 bins of a wave
// in one round are one node of tree level 8: tile 4 r + wave, and the 64 tiles of a row are the 64 lanes of a wave.  Levels
// 0-1 of a sum are two adds in the thread, levels 2-7 an xor-butterfly over the wave (partner 1 and 2 by quad permutation, 4
// and 8 by the mirrored half row and row -- after the earlier levels every lane of a mirrored block holds the same value, so
// lane i ^ 7 stands for lane i ^ 4 and lane i ^ 15 for lane i ^ 8 -- 16 and 32 by a lane permute); a maximum goes through
// the same butterfly, and so does the OR that gathers the on-bits of 16 lanes into a word.
//
//   A  the on-mask: a thread's four bits, shifted to their place and ORed over the 16 lanes of a row, are the word of 64
//      adjacent bins in natural order                                                                  -> s_on[256]
//      every wave sums and maximises its tiles unmasked                                                -> s_tile[64], s_tmax[64]
//   -- barrier; from here thread t owns word t, the bins 64 t .. 64 t + 63
//   B  the last on bin below the word (a max-scan over the 256 words) and the first above it (a min-scan): with them the
//      word's off runs are closed where they are short enough, those that reach over its ends included -> s_closed[256]
//      the first bin that is not closed above the word (a min-scan): a run's start is a closed bit above one that is not,
//      its stop the next bit that is not closed; the thread walks its starts, keeps the wide enough, and a prefix count of
//      the kept gives each its rank; the first k go to the list                                         -> s_seg[k]
//   C  per segment the tile that holds `start` and the tile that holds `stop - 1` are summed and maximised under the
//      segment's mask by the wave that owns them                                                       -> s_edge, s_emax
//   -- barrier
//      wave j & 3 finishes segment j: lane l holds tile l's node -- a masked one of C, the unmasked one of A where the whole
//      tile is in the segment, +0.0 otherwise -- and levels 8..13 are the butterfly once more; lanes 0..5 store the record
// A scan is a wave scan by lane permutes and four LDS slots.  The round that holds a tile is chosen by an unrolled
// wave-uniform compare: no register is indexed dynamically.  Static LDS, every word written by the launch before it is read;
// no workspace, no atomics, no FP-mode change; every byte of the records and the counts is stored exactly once, and nothing
// but the row and thr[row] is read.
#include <hip/hip_runtime.h>

#include "sa_signals.hpp"

// every sum is an addition of float64 values in the header's order
#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

constexpr int kSigWaves = kSigThreads / 64;
static_assert(kSigWaves == 4, "tile 4 r + wave");
constexpr int kNone = 1 << 20;                                     // "no such bin above": beyond every bin

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

// the OR over the 16 lanes of a row, in every one of them
__device__ __forceinline__ u64 row_or(u64 v)
{
    v |= dpp_u64<kX1>(v);
    v |= dpp_u64<kX2>(v);
    v |= dpp_u64<kX4>(v);
    v |= dpp_u64<kX8>(v);
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

// the scans of a wave, inclusive: the largest of lanes 0..lane, the smallest of lanes lane..63, the sum of lanes 0..lane
__device__ __forceinline__ int scan_max_up(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v = max(v, o);
    }
    return v;
}

__device__ __forceinline__ int scan_min_down(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d);
        if (lane + d < 64) v = min(v, o);
    }
    return v;
}

__device__ __forceinline__ int scan_add_up(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// the point's value: the key as a float, widened (exact, denormals kept), squared unless it is a power already
template <int FIELD> __device__ __forceinline__ double value(unsigned key)
{
    const double a = (double)__builtin_bit_cast(float, key);
    return FIELD == SA_SIGNALS_IN_POINT_POWER ? a : a * a;
}

// a key and its bin as one number whose order is the header's: the larger key, then the lower bin
__device__ __forceinline__ u64 pack(unsigned key, int bin)
{
    return (u64)key << 32 | (unsigned)~bin;
}

// lo <= i < lo + width as one unsigned compare
__device__ __forceinline__ bool within(int i, int lo, int width)
{
    return (unsigned)(i - lo) < (unsigned)width;
}

__device__ __forceinline__ int ctz64(u64 v)
{
    return __builtin_ctzll(v);
}

// the four keys of round `r` (wave-uniform) of this thread
__device__ __forceinline__ void pick(const unsigned (&pt)[kSigRounds][4], int r, unsigned (&p)[4])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = 0u;
#pragma unroll
    for (int i = 0; i < kSigRounds; ++i)
        if (i == r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = pt[i][e];
        }
}

// the word with its off runs of at most `gap` bins closed.  `below` is the last on bin under the word or -1, `above` the
// first over it or kNone; `base` is the word's first bin.
__device__ __forceinline__ u64 close_word(u64 w, int base, int below, int above, int gap)
{
    if (gap == 0) return w;
    if (w == 0) return below >= 0 && above < kNone && above - below - 1 <= gap ? ~0ull : 0ull;
    const int f = ctz64(w), l = 63 - __builtin_clzll(w);
    u64 c = w;
    if (f > 0 && below >= 0 && base + f - below - 1 <= gap) c |= (1ull << f) - 1;
    if (l < 63 && above < kNone && above - (base + l) - 1 <= gap) c |= ~0ull << (l + 1);
    u64 m = ~w & ((1ull << l) - 1) & ~((1ull << f) - 1);          // the off bits between the word's first and last on bit
    while (m) {
        const int s = ctz64(m);
        const int len = ctz64(~(m >> s));                          // at most 62
        const u64 run = ((1ull << len) - 1) << s;
        if (len <= gap) c |= run;
        m &= ~run;
    }
    return c;
}

// the stop of the run that starts at bit `s` of the closed word `c`: the next bit that is not closed, in the word or, with
// `next` the first such bin above the word, beyond it
__device__ __forceinline__ int stop_of(u64 c, int s, int base, int next)
{
    const u64 z = ~c & (~0ull << s);
    return z ? base + ctz64(z) : min(next, SA_N);
}

// grid = rows workgroups of 256 threads.  Every offset into the tensors is a size_t.
template <int FIELD>
__global__ __launch_bounds__(kSigThreads) void signals_f32_kernel(const uint4 *__restrict__ in, const unsigned *__restrict__ thr,
                                                                  unsigned tkey, unsigned char *__restrict__ out,
                                                                  int *__restrict__ stats, int k, int lo, int hi, int gap,
                                                                  int min_width)
{
    __shared__ u64 s_on[kSigWords];                                // A: the on-mask
    __shared__ double s_tile[kSigTiles];                           // A: the unmasked sum of every tile
    __shared__ u64 s_tmax[kSigTiles];                              // A: the unmasked largest of every tile
    __shared__ u64 s_closed[kSigWords];                            // B: the closed mask
    __shared__ int s_below[kSigWaves], s_above[kSigWaves], s_open[kSigWaves];     // B: the scans' wave totals
    __shared__ int s_cnt[kSigWaves], s_occ[kSigWaves], s_cov[kSigWaves];
    __shared__ int2 s_seg[SA_SIGNALS_K_MAX];                       // B: the first k kept segments
    __shared__ double s_edge[SA_SIGNALS_K_MAX][2];                 // C: a segment's first and (where it is another) last tile, masked
    __shared__ u64 s_emax[SA_SIGNALS_K_MAX][2];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t row = blockIdx.x;
    constexpr int UNITS = FIELD == SA_SIGNALS_IN_MAG ? 1 : 2;      // 16-byte loads per thread and round
    const uint4 *src = in + row * (size_t)(SA_N / 4 * UNITS);

    // the keys: the sign is cleared once, here
    unsigned pt[kSigRounds][4];
#pragma unroll
    for (int r = 0; r < kSigRounds; ++r) {
        const size_t u = (size_t)UNITS * ((size_t)t + (size_t)kSigThreads * r);
        if constexpr (FIELD == SA_SIGNALS_IN_MAG) {
            const uint4 v = src[u];
            pt[r][0] = v.x, pt[r][1] = v.y, pt[r][2] = v.z, pt[r][3] = v.w;
        } else {
            const uint4 v0 = src[u], v1 = src[u + 1];
            if constexpr (FIELD == SA_SIGNALS_IN_POINT_PEAK) {
                pt[r][0] = v0.x, pt[r][1] = v0.z, pt[r][2] = v1.x, pt[r][3] = v1.z;
            } else {
                pt[r][0] = v0.y, pt[r][1] = v0.w, pt[r][2] = v1.y, pt[r][3] = v1.w;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) pt[r][e] &= 0x7FFFFFFFu;
    }
    // on: u > 0 and u >= T, which is u >= max(T, 1)
    const unsigned T = thr != nullptr ? thr[row] & 0x7FFFFFFFu : tkey;
    const unsigned least = T > 1u ? T : 1u;

    // A
#pragma unroll
    for (int r = 0; r < kSigRounds; ++r) {
        const int tile = 4 * r + wave;
        const int bin0 = kSigTile * tile + 4 * lane;
        unsigned nib = 0;
        u64 best = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (within(bin0 + e, lo, hi - lo) && pt[r][e] >= least) nib |= 1u << e;
            best = umax(best, pack(pt[r][e], bin0 + e));
        }
        const u64 word = row_or((u64)nib << (4 * (lane & 15)));
        if ((lane & 15) == 0) s_on[4 * tile + (lane >> 4)] = word;
        const double q = (value<FIELD>(pt[r][0]) + value<FIELD>(pt[r][1])) + (value<FIELD>(pt[r][2]) + value<FIELD>(pt[r][3]));
        const double s = wave_sum(q);
        best = wave_max(best);
        if (lane == 0) s_tile[tile] = s, s_tmax[tile] = best;
    }
    __syncthreads();

    // B: the word of this thread, and the on bins next to it
    const int base = 64 * t;
    const u64 w = s_on[t];
    {
        const int up = scan_max_up(w ? base + 63 - __builtin_clzll(w) : -1, lane);
        const int down = scan_min_down(w ? base + ctz64(w) : kNone, lane);
        if (lane == 63) s_below[wave] = up;
        if (lane == 0) s_above[wave] = down;
        int below = __shfl_up(up, 1), above = __shfl_down(down, 1);
        if (lane == 0) below = -1;
        if (lane == 63) above = kNone;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < kSigWaves; ++v) {
            if (v < wave) below = max(below, s_below[v]);
            if (v > wave) above = min(above, s_above[v]);
        }
        const u64 c = close_word(w, base, below, above, gap);
        s_closed[t] = c;
        const int down2 = scan_min_down(c != ~0ull ? base + ctz64(~c) : kNone, lane);
        if (lane == 0) s_open[wave] = down2;
        int next = __shfl_down(down2, 1);
        if (lane == 63) next = kNone;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < kSigWaves; ++v)
            if (v > wave) next = min(next, s_open[v]);
        const u64 carry = t > 0 ? s_closed[t - 1] >> 63 : 0ull;
        const u64 starts = c & ~(c << 1 | carry);

        // the kept of this word's runs
        u64 kept = 0;
        int n_kept = 0, cover = 0;
        for (u64 m = starts; m; m &= m - 1) {
            const int s = ctz64(m);
            const int width = stop_of(c, s, base, next) - (base + s);
            if (width >= min_width) kept |= 1ull << s, ++n_kept, cover += width;
        }
        const int incl = scan_add_up(n_kept, lane);
        const int occ = wave_count(__builtin_popcountll(w));
        cover = wave_count(cover);
        if (lane == 63) s_cnt[wave] = incl;
        if (lane == 0) s_occ[wave] = occ, s_cov[wave] = cover;
        __syncthreads();
        int rank = incl - n_kept;
#pragma unroll
        for (int v = 0; v < kSigWaves; ++v)
            if (v < wave) rank += s_cnt[v];
        for (u64 m = kept; m && rank < k; m &= m - 1, ++rank) {
            const int s = ctz64(m);
            s_seg[rank] = make_int2(base + s, stop_of(c, s, base, next));
        }
    }
    const int count = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    const int n_seg = __builtin_amdgcn_readfirstlane(min(count, k));
    if (t < 3) {
        const int occupied = (s_occ[0] + s_occ[1]) + (s_occ[2] + s_occ[3]);
        const int covered = (s_cov[0] + s_cov[1]) + (s_cov[2] + s_cov[3]);
        stats[row * 3 + t] = t == 0 ? count : t == 1 ? occupied : covered;
    }
    // the unused slots: (-1, -1, +0.0f, -1, +0.0), a word per thread
    if (t < 6 * k) {
        const int slot = t / 6, word = t - 6 * slot;
        if (slot >= n_seg)
            reinterpret_cast<unsigned *>(out + (row * (size_t)k + (size_t)slot) * sizeof(sa_signal))[word] =
                word == 2 || word >= 4 ? 0u : ~0u;
    }
    __syncthreads();

    // C: the tiles that hold an end of a segment
    for (int j = 0; j < n_seg; ++j) {
        const int2 sg = s_seg[j];
        const int start = __builtin_amdgcn_readfirstlane(sg.x), stop = __builtin_amdgcn_readfirstlane(sg.y);
        const int tl = start >> 8, th = (stop - 1) >> 8;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int tile = e ? th : tl;
            if ((e == 0 || th != tl) && (tile & 3) == wave) {
                unsigned p[4];
                pick(pt, tile >> 2, p);
                double v[4];
                u64 best = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int bin = kSigTile * tile + 4 * lane + i;
                    const bool in_it = within(bin, start, stop - start);
                    v[i] = in_it ? value<FIELD>(p[i]) : 0.0;
                    if (in_it) best = umax(best, pack(p[i], bin));
                }
                const double s = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
                best = wave_max(best);
                if (lane == 0) s_edge[j][e] = s, s_emax[j][e] = best;
            }
        }
    }
    __syncthreads();

    // levels 8..13 and the record
    for (int j = wave; j < n_seg; j += kSigWaves) {
        const int2 sg = s_seg[j];
        const int start = __builtin_amdgcn_readfirstlane(sg.x), stop = __builtin_amdgcn_readfirstlane(sg.y);
        const int tl = start >> 8, th = (stop - 1) >> 8;
        double mine = 0.0;
        u64 best = 0;
        if (lane > tl && lane < th) mine = s_tile[lane], best = s_tmax[lane];
        if (lane == th && th != tl) mine = s_edge[j][1], best = s_emax[j][1];      // with tl == th the one is in slot 0
        if (lane == tl) mine = s_edge[j][0], best = s_emax[j][0];
        const u64 root = __builtin_bit_cast(u64, wave_sum(mine));
        best = wave_max(best);
        if (lane < 6) {
            unsigned word = (unsigned)start;
            if (lane == 1) word = (unsigned)stop;
            if (lane == 2) word = (unsigned)(best >> 32);          // peak
            if (lane == 3) word = ~(unsigned)best;                 // peak_bin
            if (lane == 4) word = (unsigned)root;
            if (lane == 5) word = (unsigned)(root >> 32);
            reinterpret_cast<unsigned *>(out + (row * (size_t)k + (size_t)j) * sizeof(sa_signal))[lane] = word;
        }
    }
}

template <int FIELD>
void launch(const void *in, const float *thr, unsigned tkey, sa_signal *out, int32_t *stats, int rows, int k, int lo, int hi, int gap,
            int min_width, hipStream_t stream)
{
    hipLaunchKernelGGL((signals_f32_kernel<FIELD>), dim3((unsigned)rows), dim3(kSigThreads), 0, stream,
                       static_cast<const uint4 *>(in), reinterpret_cast<const unsigned *>(thr), tkey,
                       reinterpret_cast<unsigned char *>(out), stats, k, lo, hi, gap, min_width);
}

}  // namespace

extern "C" int sa_signals_version(void)
{
    return SA_SIGNALS_VERSION;
}

extern "C" int sa_signals_f32(const void *in, int field, const float *thr, float threshold, sa_signal *out, int32_t *stats, int rows,
                              int k, int lo, int hi, int gap, int min_width, void *stream)
{
    const unsigned tkey = __builtin_bit_cast(unsigned, threshold);
    const char *why;
    const int rc = sa_signals_check_call(field, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)thr, tkey, (uint64_t)(uintptr_t)out,
                                         (uint64_t)(uintptr_t)stats, rows, k, lo, hi, gap, min_width, &why);
    sa_signals_set_error(why);
    if (rc != SA_OK || rows == 0) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (field) {
        case SA_SIGNALS_IN_MAG: launch<0>(in, thr, tkey, out, stats, rows, k, lo, hi, gap, min_width, st); break;
        case SA_SIGNALS_IN_POINT_PEAK: launch<1>(in, thr, tkey, out, stats, rows, k, lo, hi, gap, min_width, st); break;
        default: launch<2>(in, thr, tkey, out, stats, rows, k, lo, hi, gap, min_width, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sa_signals_set_error(hipGetErrorString(e));
        return SA_EHIP;
    }
    return SA_OK;
}
