// cascade_q15.hip -- bit-exact integer cascades for gfx950 (MI355X).
//
//   Q15 window (new/hann8192.vhd:36-39) + 6-stage integer biquad cascade, in the FPGA-exact Q7 form (filter_q7_kernel:
//   new/filter_iir_cust.vhd:96-117, new/filter_iir12_cust.vhd:68-240) and in the wide Q2.14 form (filter_w14_kernel: six
//   independent sections, the build's own spec, oracle/specan_oracle.c:or_iir_sos_q14).  Both recursions are non-linear
//   (per-product truncation and 16-bit wrap; rounding and saturation), so a frame cannot be cut in time; the parallelism
//   is batch x section: one frame per 16-lane DPP row, the six sections a systolic pipeline along the lanes (lane s works
//   on sample n-s).  One cascade wave per SIMD (a lone wave: one instruction per ~2.5 ns), one helper wave beside it for
//   staging and flushing.  The text of the pinned loops is in q15_steps.hpp, the FFT that follows in fft_q15.hip.
#include "q15_dev.hpp"
#include "q15_steps.hpp"
#include "p12_dev.hpp"
#include "../../include/specan.h"

#if defined(SA_STAMPS)
// diagnostic build only: per wave {s_memrealtime at start, at end, HW_ID | XCC_ID << 32} (tools/q15_placement.py)
__device__ unsigned long long *g_q15_stamps = nullptr;
extern "C" int sa_debug_set_q15_stamps(void *p)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_q15_stamps), &p, sizeof(p));
}
#define SA_Q15_STAMP_BEGIN(widx)                                                                      \
    const unsigned long long sa_t0_ = __builtin_amdgcn_s_memrealtime();                               \
    const int sa_widx_ = (widx)
#define SA_Q15_STAMP_END()                                                                            \
    do {                                                                                              \
        if ((threadIdx.x & 63) == 0 && g_q15_stamps) {                                                \
            g_q15_stamps[3 * sa_widx_ + 0] = sa_t0_;                                                  \
            g_q15_stamps[3 * sa_widx_ + 1] = __builtin_amdgcn_s_memrealtime();                        \
            g_q15_stamps[3 * sa_widx_ + 2] =                                                          \
                (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |      \
                ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32); \
        }                                                                                             \
    } while (0)
#else
#define SA_Q15_STAMP_BEGIN(widx) do {} while (0)
#define SA_Q15_STAMP_END() do {} while (0)
#endif

namespace {

// ------------------------------------------------------------------------------------------ IIR
// Tile size: 256 samples.  (Round 3 compiled the cascade a second time with 128-sample tiles for overlapped launches -- half
// the LDS per workgroup, so that two cascades fit beside an FFT workgroup.  With the helper waves the large tiles win at every
// depth -- 10.4 vs 9.9-10.2 M frames/s at depth 2, profiles/r4_q15_helper_waves.txt -- and the second build is gone.)
constexpr int kTile = 256;             // samples per staging tile
constexpr int kRing = 2 * kTile;      // output ring per frame: the pipeline delivers sample T - 5 at step T
constexpr int kRingPitch = kRing + 8;
constexpr int kFramesPerWave = 4;      // one frame per 16-lane row (two frames per wave and two waves per SIMD: 1.47 x slower,
                                       // profiles/r4_int_step_rate.txt)
// moving a tile between memory and LDS: 16 bytes (8 samples) per lane, kTile / 8 lanes per frame row
constexpr int kTileLanes = kTile / 8;                       // lanes that cover one row of a tile
constexpr int kTileRows = 64 / kTileLanes;                  // rows a wave covers per pass
constexpr int kTilePasses = kFramesPerWave / kTileRows;     // passes over the wave's four frames
static_assert(kTile % 32 == 0 && kTileLanes <= 64 && kTileRows * kTilePasses == kFramesPerWave, "tile geometry");

// The eight samples a lane moves, as they come from memory.  int16 samples (sa_process_q15, sa_filter_q15): 16 bytes, the
// four int16-pair words win8 takes.  Packed 12-bit samples (the _p12 entry points; include/specan.h, 24576 bytes per frame,
// 3/2 bytes per sample): samples n .. n+7, n a multiple of 8, are the 12 bytes at byte 3 n / 2 of the frame -- a multiple
// of 12, so three aligned dwords in ONE request, and the last unit of a frame ends with the frame (12 x 2048 = 24576):
// nothing outside [in, in + B * 24576) is read.
struct Q15P12x8 {
    unsigned w0, w1, w2;
};
__device__ __forceinline__ Q15P12x8 q15_load8_p12(const SaP12 *in, size_t byte)
{
    return *reinterpret_cast<const Q15P12x8 *>(in + byte);
}
// ... unpacked and repacked to the four int16-pair words
__device__ __forceinline__ uint4 q15_pairs(Q15P12x8 x)
{
    int s[8];
    p12_unpack8(x.w0, x.w1, x.w2, s);
    return make_uint4(pack2(s[0], s[1]), pack2(s[2], s[3]), pack2(s[4], s[5]), pack2(s[6], s[7]));
}
template <typename InT> constexpr bool kIsP12 = false;
template <> constexpr bool kIsP12<SaP12> = true;
template <typename InT> struct Q15Raw8 { typedef uint4 type; };
template <> struct Q15Raw8<SaP12> { typedef Q15P12x8 type; };

// one tile of the wave's four frames (and the matching ROM words) on its way from HBM to the input ring: 16 B per lane and
// pass (12 B of packed samples)
template <typename InT>
struct Q15TileRegs {
    typename Q15Raw8<InT>::type x[kTilePasses];
    uint4 c[kTilePasses];
};

// issue the global loads of one tile (4 frames x 256 samples and the matching ROM words), 16 B per lane.  HOP (the kernels
// with a hop argument): `in` is one stream and frame f begins at sample f hop of it, packed at byte 3 f hop / 2 -- hop is a
// multiple of 8: a 16-byte boundary of int16 samples, a dword boundary of packed ones.  Otherwise the frames lie back to back and `hop` is
// not read (a template parameter, not a stride argument: with a stride that the inliner folds to the constant, the int16
// kernels came out with other registers and one instruction more than they had).
template <bool HOP, typename InT>
__device__ __forceinline__ void q15_load_tile(const InT *__restrict__ in, int hop, const int16_t *__restrict__ rom, int f0,
                                              int batch, int n0, int lane, Q15TileRegs<InT> &r)
{
#pragma unroll
    for (int i = 0; i < kTilePasses; ++i) {
        const int row = kTileRows * i + lane / kTileLanes;
        const int col = (lane % kTileLanes) * 8;
        const int f = f0 + row;
        if constexpr (kIsP12<InT>) {
            r.x[i] = {0u, 0u, 0u};
            if constexpr (HOP) {
                if (f < batch) r.x[i] = q15_load8_p12(in, (size_t)f * (size_t)(3 * hop / 2) + 3 * ((n0 + col) >> 1));
            } else {
                if (f < batch) r.x[i] = q15_load8_p12(in, (size_t)f * SA_P12_FRAME_BYTES + 3 * ((n0 + col) >> 1));
            }
        } else {
            r.x[i] = make_uint4(0, 0, 0, 0);
            if constexpr (HOP) {
                if (f < batch) r.x[i] = *reinterpret_cast<const uint4 *>(in + (size_t)f * (size_t)hop + n0 + col);
            } else {
                if (f < batch) r.x[i] = *reinterpret_cast<const uint4 *>(in + (size_t)f * SA_NPTS + n0 + col);
            }
        }
        r.c[i] = *reinterpret_cast<const uint4 *>(rom + n0 + col);
    }
}

// the eight samples (16 bytes) a lane moves, windowed
__device__ __forceinline__ uint4 win8(uint4 x, uint4 c, int win_mode)
{
    const unsigned xs[4] = {x.x, x.y, x.z, x.w}, cs[4] = {c.x, c.y, c.z, c.w};
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int a, b;
        if (win_mode == SA_WIN_RTL_SIGNED) {
            a = win_rtl(lo16(xs[q]), lo16(cs[q]));
            b = win_rtl(hi16(xs[q]), hi16(cs[q]));
        } else {
            a = win_u16(lo16(xs[q]), lo16(cs[q]));
            b = win_u16(hi16(xs[q]), hi16(cs[q]));
        }
        o[q] = pack2(a, b);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// Every kernel of this file is a template on its input form: InT is int16_t or SaP12 (packed 12-bit samples), and the
// cascades take a trailing pack Hop -- empty on frames back to back, `int` on frames cut from ONE sample stream at a hop
// (SA_Q15_HOP_KIND of include/specan.h): one more kernel argument, the hop in samples, from which
// q15_load_tile takes the frame base.  One kernel per form, not a shared inlined body behind several kernels: that did
// not leave the int16 kernels the code they had before the packed form existed; these instantiations do, instruction
// for instruction.
// q15_cascade's HOP and `hop` of a kernel's pack: false and 0 (never read) for the empty pack
__device__ __forceinline__ int hop_or_zero() { return 0; }
__device__ __forceinline__ int hop_or_zero(int hop) { return hop; }

// Window only (filter mode 0xB1 through sa_filter_q15: the windowed time series, new/hann8192.vhd:36-39): element-wise,
// eight samples of a frame per thread (16 bytes, 12 of packed samples), the ROM words from the L2.
constexpr int kWinThreads = 256;
// samples n .. n + 7 of the batch (n a multiple of 8) as int16-pair words: a frame is 3/2 x 16384 bytes of packed samples, so
// packed sample n of the batch begins at byte 3 n / 2 of the batch
__device__ __forceinline__ uint4 win_load8(const int16_t *in, size_t n) { return *reinterpret_cast<const uint4 *>(in + n); }
__device__ __forceinline__ uint4 win_load8(const SaP12 *in, size_t n) { return q15_pairs(q15_load8_p12(in, 3 * (n >> 1))); }
template <typename InT>
__global__ __launch_bounds__(kWinThreads) void window_q15_kernel(const InT *__restrict__ in, int16_t *__restrict__ out, int batch,
                                                                 SaQ15Params prm, const int16_t *__restrict__ rom)
{
    const size_t chunk = (size_t)blockIdx.x * kWinThreads + threadIdx.x;      // 16-byte chunk of the batch
    if (chunk >= (size_t)batch * (SA_NPTS / 8)) return;
    const int col = (int)(chunk % (SA_NPTS / 8)) * 8;
    const uint4 xv = win_load8(in, chunk * 8);
    const uint4 cv = *reinterpret_cast<const uint4 *>(rom + col);
    *reinterpret_cast<uint4 *>(out + chunk * 8) = win8(xv, cv, prm.win_mode);
}

// ------------------------------------------------------------------------------------------ the cascade frame
// The cascade is organised around what bounds it: the recursion is serial in time, there is one wave per SIMD at
// B = 4096, and a lone wave issues one vector instruction per ~2.5 ns whatever the instruction is
// (profiles/r4_int_step_rate.txt) -- so the time per frame is 16 392 steps x the vector instructions of a step.
//   * the three feed-forward products come straight from the LEFT NEIGHBOUR's output registers
//     (v_mul_i32_i24_dpp row_ror:1): no cross-lane move, no x[n-1] / x[n-2] history registers;
//   * the input travels through the lanes the cascade leaves idle: lanes 9..15 and 0 of the 16-lane row are identity
//     stages forming a shift register, refilled with eight samples by ONE 16-bit LDS read and one select per eight steps;
//   * every step is one asm block in a fixed order, so the DPP read of a register the neighbour has just written always
//     has the two wait states the hardware asks for (the compiler cannot see into an asm block and does not pad);
//   * four cascade waves per workgroup (16 frames): the dispatcher places the waves of one workgroup on the four SIMDs of one
//     CU, 256 workgroups = one per CU at B = 4096.  (1 024 one-wave workgroups land two to a SIMD on part of the chip whenever
//     another kernel ran before: 673 us back to back, 943 us after anything else -- profiles/r2_q15_placement.txt.)
//   * four HELPER waves per workgroup (waves 4..7, one beside each cascade wave) do the staging and the flushing
//     (q15_helper_wave): a lone wave's unused issue turns are the only place where that work costs nothing.
constexpr int kV2Waves = 4;                       // cascade waves per workgroup: one per SIMD of the CU
constexpr int kWgWaves = 2 * kV2Waves;            // + one helper wave per cascade wave (staging and flushing, see q15_helper_wave)
constexpr int kInRing = 2 * kTile;                // input ring per frame: the tile in use + the one before it
constexpr int kInPitch = kInRing + 8;

// Lanes of a row: 0 = input, 1..6 = sections 0..5, 7..8 = delay (lane 8 emits sample T - 8 at step T: every group of 8
// steps ends with 8 consecutive, 16-byte aligned outputs), 9..15 = input shift register: lanes 0, 15, 14, .., 9 take
// samples T0, T0+1, .., T0+7 at the start of the group that begins at step T0.
constexpr int kRowLanes = 16;
constexpr int kGroup = 8;                         // steps per group = samples per refill = delay at the output lane
constexpr int kLaneSec0 = 1;                      // section s works in lane kLaneSec0 + s
constexpr int kLaneOut = kGroup;
constexpr int kTileIters = kTile / (4 * kGroup);  // passes of a tile loop (four groups each) per tile
constexpr int row_kin(int l16) { return (kRowLanes - l16) & (kRowLanes - 1); }      // which sample of the group the lane takes
constexpr bool row_is_in(int l16) { return row_kin(l16) < kGroup; }
constexpr bool row_is_out(int l16) { return l16 == kLaneOut; }
constexpr unsigned long long wave_mask(bool (*role)(int))
{
    unsigned long long m = 0;
    for (int lane = 0; lane < 64; ++lane) m |= (unsigned long long)role(lane % kRowLanes) << lane;
    return m;
}
constexpr unsigned long long kOutMask = wave_mask(row_is_out);     // exec of the stores: lane 8 of every row
constexpr unsigned long long kInMask = wave_mask(row_is_in);       // select of the refill: lanes 0 and 9..15
static_assert(kOutMask == 0x0100010001000100ull && kInMask == 0xFE01FE01FE01FE01ull, "row geometry");
static_assert(kLaneSec0 + SA_MAXSEC < kLaneOut && !row_is_in(kLaneOut) && kRowLanes * kFramesPerWave == 64, "row geometry");

// window the loaded tile and put it into its half (col0 = 0 or kTile) of the wave's input ring: 16 bytes per lane
template <typename InT>
__device__ __forceinline__ void q15_window_into_ring(const Q15TileRegs<InT> &r, int16_t (*dst)[kInPitch], int col0, int lane, int win_mode)
{
#pragma unroll
    for (int i = 0; i < kTilePasses; ++i) {
        const int row = kTileRows * i + lane / kTileLanes;
        const int col = col0 + (lane % kTileLanes) * 8;
        if constexpr (kIsP12<InT>) *reinterpret_cast<uint4 *>(&dst[row][col]) = win8(q15_pairs(r.x[i]), r.c[i], win_mode);
        else *reinterpret_cast<uint4 *>(&dst[row][col]) = win8(r.x[i], r.c[i], win_mode);
    }
}

// flush ncols samples of one tile of the output ring, from slot src_col on, to sample n0 on: 8 samples per lane, stored
// as 16 bytes.  A ring of dwords (the Q7 cascade) is packed to int16 with saturation (exact: the values are sign-extended
// 16-bit numbers).  n0 may be -8 (the helper's spans start eight samples early) and ncols may be 8 (the tail).
template <typename T>
__device__ __forceinline__ void flush_tile(int16_t *__restrict__ out, const T (*src)[kRingPitch], int src_col, int f0, int batch,
                                           int n0, int lane, int ncols)
{
#pragma unroll
    for (int i = 0; i < kTilePasses; ++i) {
        const int row = kTileRows * i + lane / kTileLanes;
        const int col = (lane % kTileLanes) * 8;
        const int f = f0 + row;
        const int sc = (src_col + col) & (kRing - 1);       // 8-sample chunks: the ring wraps between chunks only
        uint4 ov;
        if constexpr (sizeof(T) == 4) {
            const int4 a = *reinterpret_cast<const int4 *>(&src[row][sc]);
            const int4 b = *reinterpret_cast<const int4 *>(&src[row][sc + 4]);
            ov = make_uint4(sat_pack2(a.x, a.y), sat_pack2(a.z, a.w), sat_pack2(b.x, b.y), sat_pack2(b.z, b.w));
        } else {
            ov.x = *reinterpret_cast<const unsigned *>(&src[row][sc + 0]);
            ov.y = *reinterpret_cast<const unsigned *>(&src[row][sc + 2]);
            ov.z = *reinterpret_cast<const unsigned *>(&src[row][sc + 4]);
            ov.w = *reinterpret_cast<const unsigned *>(&src[row][sc + 6]);
        }
        if (f < batch && n0 + col >= 0 && col < ncols) *reinterpret_cast<uint4 *>(out + (size_t)f * SA_NPTS + n0 + col) = ov;
    }
}

// workgroup barrier that waits for the wave's LDS traffic only (__syncthreads would also wait for the global loads of the
// tile after next and for the stores of the tile before: exactly what is meant to stay in flight)
__device__ __forceinline__ void wg_lds_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The helper wave of a cascade wave (same frames, same SIMD): everything that is not the recursion.  A lone wave issues one
// vector instruction per ~2.5 ns and leaves the rest of its SIMD's turns unused; staging and flushing on the cascade wave
// itself cost 0.6 instructions per step = 7-9 % of the kernel (filter_q7_kernel<true> 349 -> 325-331 us with this wave,
// profiles/r4_q15_helper_waves.txt).  During the cascade's tile k the helper windows tile k + 1 into the other half of the
// input ring, requests tile k + 2 from HBM and flushes the outputs of the tile before -- shifted by the pipeline's eight
// samples of delay, so that a flush covers exactly one half of the output ring (samples [kTile j - 8, kTile (j+1) - 8) live in
// slots [kTile j, kTile (j+1)) mod kRing) while the cascade writes the other half.  One workgroup barrier per tile (both sides
// wait for their LDS traffic only); the cascade side runs nt tiles, the drain, and the same nt + 2 barriers.
template <typename T, bool HOP, typename InT>
__device__ __forceinline__ void q15_helper_wave(const InT *__restrict__ in, int hop, int16_t *__restrict__ out, const int16_t *__restrict__ rom,
                                                int16_t (*tin)[kInPitch], const T (*ring)[kRingPitch], int f0, int batch, int lane,
                                                int win_mode, bool idle)
{
    constexpr int nt = SA_NPTS / kTile;
    Q15TileRegs<InT> pre;
    if (!idle) {
        q15_load_tile<HOP>(in, hop, rom, f0, batch, 0, lane, pre);
        q15_window_into_ring(pre, tin, 0, lane, win_mode);
        q15_load_tile<HOP>(in, hop, rom, f0, batch, kTile, lane, pre);
    }
    wg_lds_sync();
    for (int k = 0; k <= nt; ++k) {                        // k = nt: the cascade runs its drain
        if (!idle) {
            if (k + 1 < nt) q15_window_into_ring(pre, tin, ((k + 1) & 1) * kTile, lane, win_mode);
            if (k + 2 < nt) q15_load_tile<HOP>(in, hop, rom, f0, batch, (k + 2) * kTile, lane, pre);
            if (k >= 1) flush_tile(out, ring, (k - 1) * kTile, f0, batch, (k - 1) * kTile - 8, lane, kTile);
        }
        wg_lds_sync();
    }
    if (!idle) flush_tile(out, ring, nt * kTile, f0, batch, nt * kTile - 8, lane, 8);     // the drain's eight samples
}

// What both cascade kernels are: waves 0..3 run the recursion on four frames each, wave 4 + w stages and flushes for wave
// w.  They differ in the element of the output ring (T), in the taps a lane holds (lane_taps(section), any section
// outside the filter an identity stage), in what a tile hands to the next (Carry, zero = no history), in the tile loop
// (tile(carry, taps, xa, ra): kTileIters x 4 groups x 8 steps; xa: LDS byte address of the lane's refill slot of the
// first group, ra: of the ring slot of lane 8's outputs) and in the drain (drain(carry, taps, xa, ra): the eight steps
// after the last tile, which deliver the frame's last eight samples).
// Sample m lives in ring slot (m + 8) mod kRing (lane 8 holds samples T0 - 8 .. T0 - 1 at the end of the group that
// starts at step T0), so that the groups of one tile store to consecutive slots (the first group of the frame stores
// eight zeros into slots nobody reads).
template <typename T, typename Carry, bool HOP, typename InT, typename LaneTaps, typename Tile, typename Drain>
__device__ __forceinline__ void q15_cascade(const InT *__restrict__ in, int hop, int16_t *__restrict__ out, int batch, int win_mode,
                                            const int16_t *__restrict__ rom, LaneTaps lane_taps, Tile tile, Drain drain)
{
    __shared__ __attribute__((aligned(16))) int16_t tin_all[kV2Waves][kFramesPerWave][kInPitch];
    __shared__ __attribute__((aligned(16))) T ring_all[kV2Waves][kFramesPerWave][kRingPitch];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wid & (kV2Waves - 1);
    const bool helper = wid >= kV2Waves;                   // wave 4 + w stages and flushes for cascade wave w
    const int lane = threadIdx.x & 63;
    int16_t (*tin)[kInPitch] = tin_all[wave];
    T (*ring)[kRingPitch] = ring_all[wave];
    const int fr = lane / kRowLanes;    // frame slot in this wave
    const int l16 = lane % kRowLanes;   // role inside the row
    const int f0 = (blockIdx.x * kV2Waves + wave) * kFramesPerWave;
    constexpr int nt = SA_NPTS / kTile;
    const bool idle = f0 >= batch;      // a pair without frames still takes part in the workgroup's barriers
    if (helper) {
        q15_helper_wave<T, HOP>(in, hop, out, rom, tin, ring, f0, batch, lane, win_mode, idle);
        return;
    }
    SA_Q15_STAMP_BEGIN(blockIdx.x * kV2Waves + wave);

    const auto taps = lane_taps(l16 - kLaneSec0);
    const int16_t *xrow = &tin[fr][0] + (row_is_in(l16) ? row_kin(l16) : 0);
    const unsigned xrow_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const int16_t *)xrow;
    const unsigned ring_addr = (unsigned)(size_t)(__attribute__((address_space(3))) T *)(&ring[fr][0]);
    Carry c = {};
    wg_lds_sync();
    for (int k = 0; k < nt; ++k) {
        const int i0 = (k & 1) * kTile;
        if (!idle) tile(c, taps, xrow_addr + 2 * i0, ring_addr + (unsigned)sizeof(T) * i0);
        wg_lds_sync();
    }
    static_assert(nt % 2 == 0, "the drain continues in the first half of both rings");
    if (!idle) drain(c, taps, xrow_addr, ring_addr);
    wg_lds_sync();
    SA_Q15_STAMP_END();
}
#define SA_TILE_OPERANDS [xa] "+v"(xa), [ra] "+v"(ra), [xin] "=&v"(xin), [cnt] "+s"(iters), [sv] "=&s"(saved)
#define SA_TILE_MASKS [inm] "s"(kInMask), [outm] "s"(kOutMask)
#define SA_TILE_CLOBBERS "memory", "scc", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59"

// ------------------------------------------------------------------------------------------ IIR, Q7 (FPGA-exact)
// One biquad step, FPGA-exact Q7 form (new/filter_iir_cust.vhd:96-117):
//   y = B2*x[n] + B1*x[n-1] + B0*x[n-2] - A0*y[n-2] - A1*y[n-1], each product >> 7 (floor), the sum
//   taken modulo 2^16 (wrapping each term first gives the same residue).
// The two subtracted terms use -floor(v/128) = floor((-v + 127)/128), so all five terms add.
// The taps are held pre-shifted by 9: floor(c v / 128) mod 2^16 is then bits 16..31 of the 32-bit product
// v * (c << 9) (exact: only bits above 31 are lost), i.e. its high word, which the SDWA form of v_add_u32
// reads in place -- no shift instructions -- and whose last add sign-extends the 16-bit result on write.
// The products are v_mul_i32_i24 / v_mad_i32_i24 (samples are 16-bit, shifted taps 17-bit: both fit the 24-bit operands).
// 9 vector instructions per step, 7 when tap B1 is zero in both coefficient sets: the host picks the form per launch
// from the coefficient bytes (sa_launch_filter_q15).  What was tried on this step and did not pay: Appendix B of DESIGN.md.
struct Q7Taps {
    int cB2, cB1, cB0, nA0, nA1;        // pre-shifted by 9, the feedback taps negated
};
// the lane's last eight outputs and what one block hands to the next (zero history = all zero: hi(k) = 0)
struct Q7Carry {
    int y[8];
    int p0, p1, p2, p3, p4, t, u, s2;
};

template <bool NOB1>
__device__ __forceinline__ void q7_tile(Q7Carry &c, const Q7Taps &t, unsigned xa, unsigned ra)
{
    int xin, iters = kTileIters;
    unsigned long long saved;
    const int k127 = 127 << 9;
#define SA_Q7_TILE_Y [y0] "+v"(c.y[0]), [y1] "+v"(c.y[1]), [y2] "+v"(c.y[2]), [y3] "+v"(c.y[3]), [y4] "+v"(c.y[4]), \
                     [y5] "+v"(c.y[5]), [y6] "+v"(c.y[6]), [y7] "+v"(c.y[7])
    if constexpr (NOB1)         // the seven-instruction block: p1, u and cB1 are not touched
        asm volatile(SA_Q7_TILE(SA_Q7_BLOCK7)
                     : SA_Q7_TILE_Y, [s2] "+v"(c.s2), [p0] "+v"(c.p0), [p2] "+v"(c.p2), [p3] "+v"(c.p3), [p4] "+v"(c.p4),
                       [t] "+v"(c.t), SA_TILE_OPERANDS
                     : [cB2] "v"(t.cB2), [cB0] "v"(t.cB0), [nA0] "v"(t.nA0), [nA1] "v"(t.nA1), [k] "s"(k127), SA_TILE_MASKS
                     : SA_TILE_CLOBBERS);
    else
        asm volatile(SA_Q7_TILE(SA_Q7_BLOCK9)
                     : SA_Q7_TILE_Y, [s2] "+v"(c.s2), [p0] "+v"(c.p0), [p1] "+v"(c.p1), [p2] "+v"(c.p2), [p3] "+v"(c.p3),
                       [p4] "+v"(c.p4), [t] "+v"(c.t), [u] "+v"(c.u), SA_TILE_OPERANDS
                     : [cB2] "v"(t.cB2), [cB1] "v"(t.cB1), [cB0] "v"(t.cB0), [nA0] "v"(t.nA0), [nA1] "v"(t.nA1), [k] "s"(k127),
                       SA_TILE_MASKS
                     : SA_TILE_CLOBBERS);
#undef SA_Q7_TILE_Y
}

typedef unsigned q7_u4 __attribute__((ext_vector_type(4)));

// 16-byte LDS store by the lanes of `mask` only, without a branch around it (the compiler's form is a
// saveexec / skip-branch / restore triple laid out of line: two taken branches per eight steps)
__device__ __forceinline__ void lds_store16_masked(unsigned addr, q7_u4 v, unsigned long long mask)
{
    unsigned long long saved;
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t"
                 "ds_write_b128 %[a], %[d]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [sv] "=&s"(saved) : [m] "s"(mask), [a] "v"(addr), [d] "v"(v) : "memory", "scc");
}

// The drain: one group of eight steps in the compiler's hands, one asm statement per block.  Always the nine-instruction
// block: after the seven-instruction tiles p1 is still the zero it started as, and G rebuilds u from p1 and p2 itself, so
// its I forms the s2 the seven-instruction I would.  (Draining with one more pass of the tile loop, as the wide cascade
// does, measured 4-5 us slower on filter_q7_kernel<true>, 336 -> 340-341 us: profiles/r7_q15_refactor.txt.)
__device__ __forceinline__ void q7_drain(Q7Carry &c, const Q7Taps &t, unsigned xa, unsigned ra)
{
    const int xin = *(__attribute__((address_space(3))) const uint16_t *)(size_t)xa;
    if (row_is_in(threadIdx.x % kRowLanes)) c.t = xin;
    const int k127 = 127 << 9;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int y0;
        asm volatile(SA_Q7_BLOCK9("%[y0]", "%[y7]")
                     : [y0] "=&v"(y0), [s2] "+v"(c.s2), [p0] "+v"(c.p0), [p1] "+v"(c.p1), [p2] "+v"(c.p2), [p3] "+v"(c.p3),
                       [p4] "+v"(c.p4), [t] "+v"(c.t), [u] "+v"(c.u)
                     : [y7] "v"(c.y[(e + 7) & 7]), [cB2] "v"(t.cB2), [cB1] "v"(t.cB1), [cB0] "v"(t.cB0), [nA0] "v"(t.nA0),
                       [nA1] "v"(t.nA1), [k] "s"(k127));
        c.y[e] = y0;
    }
    q7_u4 va, vb;
    va.x = c.y[0]; va.y = c.y[1]; va.z = c.y[2]; va.w = c.y[3];
    vb.x = c.y[4]; vb.y = c.y[5]; vb.z = c.y[6]; vb.w = c.y[7];
    lds_store16_masked(ra, va, kOutMask);
    lds_store16_masked(ra + 16, vb, kOutMask);
}

template <typename InT, bool NOB1, typename... Hop>
__global__ __launch_bounds__(64 * kWgWaves) void filter_q7_kernel(const InT *__restrict__ in, int16_t *__restrict__ out, int batch,
                                                                  SaQ15Params prm, const int16_t *__restrict__ rom, Hop... hop)
{
    q15_cascade<int, Q7Carry, sizeof...(Hop) != 0>(in, hop_or_zero(hop...), out, batch, prm.win_mode, rom, [&](int sec) -> Q7Taps {
        if (sec < 0 || sec >= SA_MAXSEC) return {128 << 9, 0, 0, 0, 0};     // identity = (128 x) >> 7
        const int8_t *c = &prm.c12[(sec & 1) ? 6 : 0];                      // stages 1,3,5 = set 0; 2,4,6 = set 1
        return {c[2] << 9, c[1] << 9, c[0] << 9, -(c[3] << 9), -(c[4] << 9)};
    }, [](Q7Carry &c, const Q7Taps &t, unsigned xa, unsigned ra) { q7_tile<NOB1>(c, t, xa, ra); }, q7_drain);
}

// ------------------------------------------------------------------------------------------ IIR, wide Q2.14 form
// Mode 0xA2 (the build's own spec, oracle/specan_oracle.c:or_iir_sos_q14; the six sections scripts/fft_analyzer_gui.py:108-157
// designs and :1186-1192 cuts down to two): per section, direct form I,
//     y[n] = sat16( (b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] + 8192) >> 14 ),
// int16 taps and samples.  The exact sum needs 34 bits.  It is kept in two 32-bit accumulators without a single 64-bit
// instruction: every tap (and every negated feedback tap, -a in [-32767, 32768]) splits as c = 2^14 ch + cl with
// cl in [-8192, 8191] and ch in {-2..2}, so
//     acc_l = 8192 + sum cl v   (|acc_l| <= 5 * 2^13 * 2^15 + 2^13 < 2^31, no wrap at any partial sum)
//     acc_h =        sum ch v   (|acc_h| <= 10 * 2^15)
//     (acc + 8192) >> 14 = acc_h + (acc_l >> 14)            exactly (acc_h is an integer: the floor passes it)
// and the two products a packed-int16 dot product forms per instruction halve the count: with the lane's last two outputs
// and the neighbour's last two outputs held as packed pairs P = (lo: y[n-1], hi: y[n]), one step is
//     acc  = dot2(P_own[n-1], (-a2, -a1), 8192 | 0)          v_dot2_i32_i16, low and high half: 2 instructions
//     X    = P_neighbour[n-1]                                v_mov_b32_dpp row_ror:1 = (x[n-1], x[n])
//     acc += dot2(X, (b1, b0));  acc += dot2(X_prev, (b2, 0))                                   4 instructions
//     w    = acc_h + (acc_l >> 14)                           v_ashrrev_i32, v_add_u32
//     P_own[n] = (sat16(w[n-1]), sat16(w[n]))                v_cvt_pk_i16_i32: saturation and packing in ONE instruction
// = 10 vector instructions per step against 9 of the Q7 form (filter_q7_kernel<false>) and about 40 of the round-1 form
// (five 64-bit multiply-adds, a 64-bit shift, two compares and selects, three cross-lane moves).  Everything else is
// the Q7 kernel's structure: four waves per workgroup and one workgroup per CU at B = 4096 (one wave per SIMD in every
// placement scenario, profiles/r2_q15_placement.txt), lanes 0 and 9..15 of the row an input shift register refilled by
// one 16-bit LDS read per eight steps (identity sections: b0 = 16384 gives w = x exactly), lanes 7..8 delay stages so
// that lane 8 emits sample T - 8 at step T, the tile loop ONE pinned asm statement.  The outputs leave as packed int16
// (the pairs of the odd steps, v[52:55]: one 16-byte LDS store per eight steps), so the output ring is half the Q7 kernel's.
struct W14Taps {
    unsigned c01l, c01h, c2l, c2h, cfbl, cfbh;      // packed (lo, hi) int16 pairs: (b1, b0), (b2, 0), (-a2, -a1); low / high split
};
__device__ __forceinline__ void w14_split(int c, int &cl, int &ch)
{
    cl = ((c + 8192) & 16383) - 8192;
    ch = (c - cl) >> 14;
}
__device__ __forceinline__ W14Taps w14_taps(int b0, int b1, int b2, int a1, int a2)
{
    int b0l, b0h, b1l, b1h, b2l, b2h, n1l, n1h, n2l, n2h;
    w14_split(b0, b0l, b0h); w14_split(b1, b1l, b1h); w14_split(b2, b2l, b2h);
    w14_split(-a1, n1l, n1h); w14_split(-a2, n2l, n2h);
    W14Taps t;
    t.c01l = pack2(b1l, b0l); t.c01h = pack2(b1h, b0h);
    t.c2l = pack2(b2l, 0);    t.c2h = pack2(b2h, 0);
    t.cfbl = pack2(n2l, n1l); t.cfbh = pack2(n2h, n1h);
    return t;
}

// what one tile hands to the next: the eight pair registers of the group, the two unsaturated outputs and the two
// neighbour pairs the next block reads
struct W14Carry {
    unsigned p[8];
    int w0, w1;
    unsigned x0, x1;
};


__device__ __forceinline__ void w14_tile(W14Carry &c, const W14Taps &t, unsigned xa, unsigned ra, int iters)
{
    int xin, al, ah;
    unsigned long long saved;
    asm volatile(SA_W14_TILE
                 : [p0] "+v"(c.p[0]), [p1] "+v"(c.p[1]), [p2] "+v"(c.p[2]), [p3] "+v"(c.p[3]), [p4] "+v"(c.p[4]), [p5] "+v"(c.p[5]),
                   [p6] "+v"(c.p[6]), [p7] "+v"(c.p[7]), [w0] "+v"(c.w0), [w1] "+v"(c.w1), [x0] "+v"(c.x0), [x1] "+v"(c.x1),
                   [xa] "+v"(xa), [ra] "+v"(ra), [xin] "=&v"(xin), [al] "=&v"(al), [ah] "=&v"(ah), [cnt] "+s"(iters), [sv] "=&s"(saved)
                 : [c01l] "v"(t.c01l), [c01h] "v"(t.c01h), [c2l] "v"(t.c2l), [c2h] "v"(t.c2h), [cfbl] "v"(t.cfbl), [cfbh] "v"(t.cfbh),
                   [k] "s"(8192), SA_TILE_MASKS
                 : SA_TILE_CLOBBERS);
}

// one pass of four groups as the drain: the first delivers the frame's last eight samples, the other three filter whatever
// the input ring holds into slots that were flushed long ago
template <typename InT, typename... Hop>
__global__ __launch_bounds__(64 * kWgWaves) void filter_w14_kernel(const InT *__restrict__ in, int16_t *__restrict__ out, int batch,
                                                                   SaQ15Params prm, const int16_t *__restrict__ rom, Hop... hop)
{
    q15_cascade<int16_t, W14Carry, sizeof...(Hop) != 0>(in, hop_or_zero(hop...), out, batch, prm.win_mode, rom, [&](int sec) {
        // identity: (16384 x + 8192) >> 14 = x exactly
        if (sec < 0 || sec >= prm.nsec_wide) return w14_taps(16384, 0, 0, 0, 0);
        // scipy row order [b0, b1, b2, a0, a1, a2], a0 ignored (= 1.0)
        const int16_t *c = &prm.sos_q14[sec * 6];
        return w14_taps(c[0], c[1], c[2], c[4], c[5]);
    }, [](W14Carry &c, const W14Taps &t, unsigned xa, unsigned ra) { w14_tile(c, t, xa, ra, kTileIters); },
    [](W14Carry &c, const W14Taps &t, unsigned xa, unsigned ra) { w14_tile(c, t, xa, ra, 1); });
}

// the cascade launch of one input form: the wide cascade, or the Q7 cascade with its seven- or nine-instruction step.
// `hop`: nothing for frames back to back, the hop in samples for frames cut from one stream (the kernels' trailing argument).
template <typename InT, typename... Hop>
void launch_cascade(const InT *in, int16_t *out_time, int batch, const SaQ15Params &p, const SaQ15Tables &t, hipStream_t stream,
                    SaLaunchEv ev, Hop... hop)
{
    const int per_wg = kFramesPerWave * kV2Waves;
    const dim3 grid_wg((batch + per_wg - 1) / per_wg), block_wg(64 * kWgWaves);
    if (p.filter == SA_FILTER_WIDE) {
        hipExtLaunchKernelGGL((filter_w14_kernel<InT, Hop...>), grid_wg, block_wg, 0, stream, ev.start, ev.stop, 0, in, out_time, batch,
                              p, t.rom, hop...);
    } else {
        // B1 = 0 in both coefficient sets (wire order b0,b1,b2,a0,a1,a2 per set): the seven-instruction step
        const bool nob1 = p.c12[1] == 0 && p.c12[7] == 0;
        hipExtLaunchKernelGGL(nob1 ? filter_q7_kernel<InT, true, Hop...> : filter_q7_kernel<InT, false, Hop...>, grid_wg, block_wg, 0,
                              stream, ev.start, ev.stop, 0, in, out_time, batch, p, t.rom, hop...);
    }
}

// every launch of one input form: window only (frames alone), or its cascade on frames (hop = 0) or on one stream
template <typename InT>
void launch_filter(const InT *in, int hop, int16_t *out_time, int batch, const SaQ15Params &p, const SaQ15Tables &t,
                   hipStream_t stream, SaLaunchEv ev)
{
    if (p.filter == SA_FILTER_NONE) {
        const size_t chunks = (size_t)batch * (SA_NPTS / 8);
        hipExtLaunchKernelGGL(window_q15_kernel<InT>, dim3((unsigned)((chunks + kWinThreads - 1) / kWinThreads)), dim3(kWinThreads), 0,
                              stream, ev.start, ev.stop, 0, in, out_time, batch, p, t.rom);
    } else if (hop != 0) {
        launch_cascade(in, out_time, batch, p, t, stream, ev, hop);
    } else {
        launch_cascade(in, out_time, batch, p, t, stream, ev);
    }
}

}  // namespace

// A stream is read by a cascade only: window-only output of a stream is not offered (sa_filter_q15 has no kind word), and in
// filter mode 0xB1 the FFT's stage 0 reads the stream itself.
hipError_t sa_launch_filter_q15(const void *in, SaInKind in_kind, int hop, int16_t *out_time, int batch, const SaQ15Params &p,
                                const SaQ15Tables &t, hipStream_t stream, SaLaunchEv ev)
{
    if (in_kind != SaInKind::I16 && in_kind != SaInKind::P12) return hipErrorInvalidValue;
    if (hop != 0 && (hop < 0 || hop > SA_NPTS || hop % 8 != 0 || p.filter == SA_FILTER_NONE)) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    if (in_kind == SaInKind::P12) launch_filter(static_cast<const SaP12 *>(in), hop, out_time, batch, p, t, stream, ev);
    else launch_filter(static_cast<const int16_t *>(in), hop, out_time, batch, p, t, stream, ev);
    return hipGetLastError();
}
