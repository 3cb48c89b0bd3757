// fft_q15.hip -- SA-FXFFT-1 for gfx950 (MI355X): the fixed-point FFT that stands where ip/xfft_0 stands
// (radix-4 DIF, >>2 per stage, Q15 twiddles, truncation).  One 1024-thread workgroup per frame, data in LDS as packed
// (re,im) int16 pairs, Stockham (autosort) addressing so the result is in natural order, stages paired in registers; the
// arithmetic per butterfly is exactly oracle/specan_oracle.c:or_fxfft16k.
#include "q15_dev.hpp"
#include "../../include/specan.h"

namespace {

// The four outputs of a butterfly leave the adder tree as 32-bit sums X (re), Y (im) that still want the >> 2 of
// the spec.  Shift and pack are one instruction per half: v_ashrrev_i32 in its SDWA form writes the low word of
// its result into the chosen half of the destination (the first write zeroes the other half, the second preserves
// it); (sum of four int16) >> 2 lies in [-32768, 32767], so taking the low word is exact.  gfx950 wants one
// instruction between a sub-dword write and a read of the same register (the preserving write reads it): the four
// first-half writes come first, then the four second-half writes, then one s_nop before the compiler's code.
//   LO* / HI*: which sum goes to the low / high word of output 0..3.
#define SA_FX_PACK4(P0, P1, P2, P3, LO0, LO1, LO2, LO3, HI0, HI1, HI2, HI3)                                            \
    asm("v_ashrrev_i32_sdwa %0, %12, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"        \
        "v_ashrrev_i32_sdwa %1, %12, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"        \
        "v_ashrrev_i32_sdwa %2, %12, %6 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"        \
        "v_ashrrev_i32_sdwa %3, %12, %7 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"        \
        "v_ashrrev_i32_sdwa %0, %12, %8 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"   \
        "v_ashrrev_i32_sdwa %1, %12, %9 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"   \
        "v_ashrrev_i32_sdwa %2, %12, %10 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"  \
        "v_ashrrev_i32_sdwa %3, %12, %11 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"  \
        "s_nop 0"                                                                                                      \
        : "=&v"(P0), "=&v"(P1), "=&v"(P2), "=&v"(P3)                                                                   \
        : "v"(LO0), "v"(LO1), "v"(LO2), "v"(LO3), "v"(HI0), "v"(HI1), "v"(HI2), "v"(HI3), "s"(2))

// lo(a) lo(b) + hi(a) hi(b), exact in 32 bits.  Written out: the builtin is selected as the accumulating two-operand
// form v_dot2c_i32_i16, which costs a v_mov of zero into the accumulator per product.
__device__ __forceinline__ int fx_dot2(unsigned a, unsigned b)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// the same with a wave-uniform second operand taken straight from its scalar register (no v_mov per product)
__device__ __forceinline__ int fx_dot2_s(unsigned a, unsigned b)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "s"(b));
    return r;
}

// y = sat16((u * w) >> 15), truncation (SA-FXFFT-1), for u packed as p = (lo = u.im, hi = u.re):
//   y.im = u.im wr + u.re wi = p . (wr, wi);   y.re = u.re wr - u.im wi = p . (-wi, wr)
// wi = -32768 has no int16 negation; the table holds it for the exponents 4082..4110 (-32768 sin rounds to -32768
// that far around pi/2).  Which butterflies of a thread can meet them is known at compile time (the u loops are
// unrolled): output 1 in stages 0 and 1 at u = 3 (e1 = 4082..4095), output 3 there at u = 1 (3 e1 = 4083..4110),
// output 2 at u = 1 or 2 in stages 0 and 1 and at u = 2 from stage 2 on (2 e1 = 4082..4110).  Those form the real
// part from the halves with two 24-bit multiplies (`wide1..3`); everything else takes both words of the table.
template <bool UNIFORM>
__device__ __forceinline__ unsigned fx_twiddle13(unsigned p, uint2 w)
{
    if constexpr (UNIFORM) return sat_pack2(fx_dot2_s(p, w.y) >> 15, fx_dot2_s(p, w.x) >> 15);
    else return sat_pack2(fx_dot2(p, w.y) >> 15, fx_dot2(p, w.x) >> 15);
}
template <bool UNIFORM>
__device__ __forceinline__ unsigned fx_twiddle2(unsigned p, unsigned w)
{
    const int pr = (hi16(p) * lo16(w) - lo16(p) * hi16(w)) >> 15;
    return sat_pack2(pr, (UNIFORM ? fx_dot2_s(p, w) : fx_dot2(p, w)) >> 15);
}

// the three twiddles of one butterfly of a per-lane stage: one 32-byte record (SaQ15Tables::twrec), read as 16 + 8 bytes
struct SaTw3 {
    uint2 w1, w2, w3;
};
__device__ __forceinline__ SaTw3 fx_twrec(const uint4 *__restrict__ twrec, int r)
{
    const uint4 a = twrec[2 * r];
    const uint2 b = *reinterpret_cast<const uint2 *>(&twrec[2 * r + 1]);
    return {make_uint2(a.x, a.y), make_uint2(a.z, a.w), b};
}

// one radix-4 DIF butterfly of SA-FXFFT-1 on packed (re, im) int16 pairs: 32-bit sums, >> 2 (truncation),
// Q15 twiddles on outputs 1..3 (exact pass-through when the exponent is 0), saturation to int16
// UNIFORM: the twiddles are the same for the whole wave (scalar loads, or compile-time exponents)
template <bool UNIFORM = false>
__device__ __forceinline__ void fx_butterfly(unsigned a, unsigned b, unsigned c, unsigned d, uint2 w1, uint2 w2,
                                             uint2 w3, bool unity, unsigned (&o)[4], bool wide1, bool wide2, bool wide3)
{
    const int ar = lo16(a), ai = hi16(a), br = lo16(b), bi = hi16(b);
    const int cr = lo16(c), ci = hi16(c), dr = lo16(d), di = hi16(d);
    const int sr = ar + cr, si = ai + ci, tr = ar - cr, ti = ai - ci;      // a +/- c
    const int ur = br + dr, ui = bi + di, vr = br - dr, vi = bi - di;      // b +/- d
    const int x0 = sr + ur, y0 = si + ui;
    const int x1 = tr + vi, y1 = ti - vr;                                  // a - i b - c + i d
    const int x2 = sr - ur, y2 = si - ui;
    const int x3 = tr - vi, y3 = ti + vr;                                  // a + i b - c - i d
    unsigned p0, p1, p2, p3;
    if (unity) {
        // pass-through: the results are in range by construction, the pack is all that is left
        SA_FX_PACK4(p0, p1, p2, p3, x0, x1, x2, x3, y0, y1, y2, y3);
        o[0] = p0; o[1] = p1; o[2] = p2; o[3] = p3;
    } else {
        SA_FX_PACK4(p0, p1, p2, p3, x0, y1, y2, y3, y0, x1, x2, x3);       // outputs 1..3 as (im, re) for the products
        o[0] = p0;
        o[1] = wide1 ? fx_twiddle2<UNIFORM>(p1, w1.x) : fx_twiddle13<UNIFORM>(p1, w1);
        o[2] = wide2 ? fx_twiddle2<UNIFORM>(p2, w2.x) : fx_twiddle13<UNIFORM>(p2, w2);
        o[3] = wide3 ? fx_twiddle2<UNIFORM>(p3, w3.x) : fx_twiddle13<UNIFORM>(p3, w3);
    }
}

// The first stage's butterfly: the inputs are real (imag = 0, new/command_control.vhd:123), which leaves 7 of the 16
// additions and 6 of the 8 shift-and-insert instructions: with s = a + c, t = a - c, u = b + d, v = b - d
//   out0 = (s + u, 0)    out1 = (t, -v)    out2 = (s - u, 0)    out3 = (t, v)        (each >> 2)
// and output 2's twiddle product is two multiplies (its imaginary input is 0).  Same results as fx_butterfly on
// (a, 0) .. (d, 0) by construction; a, b, c, d are sign-extended 16-bit samples.
__device__ __forceinline__ void fx_butterfly_real(int a, int b, int c, int d, uint2 w1, unsigned w2, uint2 w3, bool unity,
                                                  unsigned (&o)[4], bool wide1, bool wide3)
{
    const int sr = a + c, tr = a - c, ur = b + d, vr = b - d, nv = d - b;
    const int x0 = sr + ur, x2 = sr - ur;
    unsigned p0, p1, p2, p3;
    if (unity) {
        // (re, im) pairs as stored: out0 = (x0, 0), out1 = (t, -v), out2 = (x2, 0), out3 = (t, v)
        asm("v_ashrrev_i32_sdwa %0, %9, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %1, %9, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %2, %9, %6 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %3, %9, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %1, %9, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %3, %9, %8 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
            "s_nop 0"
            : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
            : "v"(x0), "v"(tr), "v"(x2), "v"(nv), "v"(vr), "s"(2));
        o[0] = p0; o[1] = p1; o[2] = p2; o[3] = p3;
    } else {
        // outputs 1 and 3 as (im, re) for the products, output 2's real input as a plain number
        asm("v_ashrrev_i32_sdwa %0, %7, %3 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %1, %7, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %2, %7, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %1, %7, %6 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
            "v_ashrrev_i32_sdwa %2, %7, %6 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
            "s_nop 0"
            : "=&v"(p0), "=&v"(p1), "=&v"(p3)
            : "v"(x0), "v"(nv), "v"(vr), "v"(tr), "s"(2));
        const int u2 = x2 >> 2;
        o[0] = p0;
        o[1] = wide1 ? fx_twiddle2<false>(p1, w1.x) : fx_twiddle13<false>(p1, w1);
        o[2] = sat_pack2((u2 * lo16(w2)) >> 15, (u2 * hi16(w2)) >> 15);
        o[3] = wide3 ? fx_twiddle2<false>(p3, w3.x) : fx_twiddle13<false>(p3, w3);
    }
}

constexpr int kFftWide = 1024;                            // threads per frame (fft_q15_kernel below)

// ---- SA_Q15_OUT_MAG / SA_Q15_OUT_MARKER: the host's decode of the wire frame, made in the epilogue -------------------
// decode_mag_16iq_le (gui.py:250-260) is np.sqrt(re.astype(float32)**2 + im.astype(float32)**2): four float32 operations,
// each rounded on its own.  The two squares and their sum must therefore not be contracted into an FMA (hipcc's default
// is -ffp-contract=fast; squares are exact only up to |v| = 4096), and the root must be the correctly rounded one.
__device__ __forceinline__ float fx_mag_sum(unsigned p)
{
#pragma clang fp contract(off)
    const float r = (float)lo16(p), i = (float)hi16(p);
    const float rr = r * r, ii = i * i;
    return rr + ii;
}

// Correctly rounded square root of s = 0 or an integer-valued float in [1, 2^31]: v_sqrt_f32 is within 1 ulp, so the
// result is y or one of its two neighbours, told apart by the signs of the exact residuals s - y_down y and s - y_up y
// (one FMA each).  This is the compiler's own sequence for sqrtf without its input scaling for denormals and its class
// test for 0 and infinity, neither of which can occur: for s = 0 the lower neighbour is a NaN whose comparison fails
// and the upper one gives a residual of 0, so the result is +0.
__device__ __forceinline__ float fx_sqrt_rn(float s)
{
    const float y = __builtin_amdgcn_sqrtf(s);
    const float dn = __builtin_bit_cast(float, __builtin_bit_cast(int, y) - 1);
    const float up = __builtin_bit_cast(float, __builtin_bit_cast(int, y) + 1);
    const float rd = __builtin_fmaf(-dn, y, s), ru = __builtin_fmaf(-up, y, s);
    float z = rd <= 0.f ? dn : y;
    z = ru > 0.f ? up : z;
    return z;
}

__device__ __forceinline__ float fx_mag(unsigned p) { return fx_sqrt_rn(fx_mag_sum(p)); }

// SA_Q15_OUT_MARKER: a part of the record -- the largest magnitude seen (-1: none yet), the lowest bin attaining it, and
// the exact integer power sum (at most 16384 x 2^31 = 2^45).
struct FxMark {
    float mag;
    int bin;
    unsigned long long pow;
};

// Per bin the thread forms only s = fl(fl(re re) + fl(im im)) (-1 outside [lo, hi)) and the integer power; the root is
// deferred to fx_mark_thread.  re^2 + im^2 reaches 2^31 (re = im = -32768): the dot product's 32-bit result is read as
// unsigned.  MASK: k may lie outside the range.
template <bool MASK>
__device__ __forceinline__ float fx_mark_sum(unsigned long long &pow, unsigned p, int k, int lo, int hi)
{
    float s = fx_mag_sum(p);
    unsigned pw = (unsigned)fx_dot2(p, p);
    if constexpr (MASK) {
        const bool in = (unsigned)(k - lo) < (unsigned)(hi - lo);
        s = in ? s : -1.f;
        pw = in ? pw : 0u;
    }
    pow += pw;
    return s;
}

// The wave's 64 bins of one m' are [kw, kw + 64) (kw wave-uniform): one scalar decision for all of them -- skip, take
// whole, or test bin by bin where an edge of the range cuts through.
__device__ __forceinline__ float fx_mark_sum_any(unsigned long long &pow, unsigned p, int k, int kw, int lo, int hi)
{
    if (kw + 64 <= lo || kw >= hi) return -1.f;
    if (kw >= lo && kw + 64 <= hi) return fx_mark_sum<false>(pow, p, k, lo, hi);
    return fx_mark_sum<true>(pow, p, k, lo, hi);
}

// The thread's part from its 16 sums s[m'] (bin t + 1024 m'), with ONE root instead of sixteen.  The correctly rounded
// root is monotone, so the thread's largest magnitude is M = rt(S), S = max s, and its bins attaining M are those with
// s > L, L = ((M + M_prev) / 2)^2 the square of the rounding boundary below M (s <= S keeps them below the upper one).
// L is exact in double (a 25-bit number squared).  s = L cannot happen: the boundary is an odd multiple of half an ulp,
// its square has some 49 significant bits and s has 24 -- so there is no tie case, and the test per bin is s >= T with
// T the float next above L.  M = 0: every bin of the range attains it (T = 0; bins outside hold -1).  No bin of the
// thread in the range (S = -1): magnitude -1, T = +inf.
__device__ __forceinline__ FxMark fx_mark_thread(const float (&s)[16], int t, unsigned long long pow)
{
    float top = -1.f;
#pragma unroll
    for (int m = 0; m < 16; ++m) top = __builtin_fmaxf(top, s[m]);
    const float mag = fx_sqrt_rn(__builtin_fmaxf(top, 0.f));
    const float prev = __builtin_bit_cast(float, __builtin_bit_cast(int, mag) - 1);
    const double mid = 0.5 * ((double)mag + (double)prev);
    const double edge = mid * mid;
    float thr = (float)edge;
    thr = (double)thr > edge ? thr : __builtin_bit_cast(float, __builtin_bit_cast(int, thr) + 1);
    thr = mag > 0.f ? thr : 0.f;
    thr = top < 0.f ? __builtin_inff() : thr;
    int bin = SA_NPTS;
#pragma unroll
    for (int m = 15; m >= 0; --m) bin = s[m] >= thr ? t + kFftWide * m : bin;      // descending: the lowest bin stays
    return {top < 0.f ? -1.f : mag, bin, pow};
}

// a <- combine(a, b): the exact sum and the (larger magnitude, then lower bin) pair.  Symmetric and associative, integer
// sum: the record's bits depend on the data alone, whatever the order of the merges.
__device__ __forceinline__ void fx_mark_merge(FxMark &a, const FxMark &b)
{
    a.pow += b.pow;
    if (b.mag > a.mag || (b.mag == a.mag && b.bin < a.bin)) {
        a.mag = b.mag;
        a.bin = b.bin;
    }
}

template <int XOR>
__device__ __forceinline__ FxMark fx_mark_swizzle(const FxMark &a)
{
    constexpr int pat = (XOR << 10) | 0x1F;                  // ds_swizzle bitmask mode: lane ^ XOR inside 32 lanes
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)a.pow, pat);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(a.pow >> 32), pat);
    return {__builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, a.mag), pat)),
            __builtin_amdgcn_ds_swizzle(a.bin, pat), (unsigned long long)hi << 32 | lo};
}

// every lane of a half-wave ends with the half-wave's part
__device__ __forceinline__ void fx_mark_reduce32(FxMark &a)
{
    fx_mark_merge(a, fx_mark_swizzle<1>(a));
    fx_mark_merge(a, fx_mark_swizzle<2>(a));
    fx_mark_merge(a, fx_mark_swizzle<4>(a));
    fx_mark_merge(a, fx_mark_swizzle<8>(a));
    fx_mark_merge(a, fx_mark_swizzle<16>(a));
}

// The frame's record from the threads' parts: a swizzle butterfly inside each half-wave, the 32 half-wave parts through
// `scr` (512 bytes of LDS behind the frame image, so no barrier is needed to free the image first), a second butterfly
// over them in wave 0, and one 16-byte vector store by thread 0.  No atomics.
constexpr int kFxMarkParts = kFftWide / 32;
__device__ __forceinline__ void fx_mark_finish(FxMark a, uint4 *scr, void *__restrict__ out, int f, int t, int wave)
{
    fx_mark_reduce32(a);
    if ((t & 31) == 0)
        scr[t >> 5] = make_uint4(__builtin_bit_cast(unsigned, a.mag), (unsigned)a.bin, (unsigned)a.pow, (unsigned)(a.pow >> 32));
    __syncthreads();
    if (wave != 0) return;
    const uint4 v = scr[t & 31];
    a = {__builtin_bit_cast(float, v.x), (int)v.y, (unsigned long long)v.w << 32 | v.z};
    fx_mark_reduce32(a);
    if (t == 0)
        reinterpret_cast<uint4 *>(out)[f] =
            make_uint4(__builtin_bit_cast(unsigned, a.mag), (unsigned)a.bin, (unsigned)a.pow, (unsigned)(a.pow >> 32));
}

// SA-FXFFT-1 with 1024 threads per frame: 16 positions per thread (t + 1024 m); the seven radix-4 stages run as four
// register passes -- stage 0 from global memory, then (1,2), (3,4), (5,6) -- with one LDS exchange between passes.
// (Round 1 and most of round 2 ran 256 threads x 64 positions, stages 4..6 in registers: 120 registers per thread, 2 waves
// per SIMD, a quarter of a wave's life in s_waitcnt behind a barrier with one other wave to cover: 192 us.  Rounds 2-3 ran
// 1024 threads with ONE stage per LDS exchange for stages 0..4: 155-158 us.  Pairing the stages (three exchanges instead
// of five, the second stage of a pair shares one twiddle triple among a thread's four butterflies) and reading a lane's
// three twiddles as one 32-byte record instead of three strided gathers: 126-137 us by box, profiles/r4_fft_q15_passes.txt.)
//   7 radix-4 DIF stages, Stockham addressing:
//   storage after s stages: pos = j * 4^s + kappa   (j: remaining time index, kappa: bins so far)
//   butterfly bf in [0,4096): j' = bf >> 2s, kappa = bf & (4^s - 1); inputs at bf + i*4096;
//   output i' at (j' << (2s+2)) | (i' << 2s) | kappa; twiddle exponent i' * j' * 4^s.
// 8 waves per SIMD (two frames per CU, 64 KiB of LDS each) need <= 64 registers: the second launch bound asks for that.
// OUT (SA_Q15_OUT_*): what the epilogue makes of the natural-order bins -- the wire frame itself, its magnitudes, or the
// marker record over the bins [mrange & 0xFFFF, mrange >> 16) (read by the MARKER instantiations only; last in the
// arguments, so the other kinds' argument loads are where they were).
constexpr int kFftLds = SA_NPTS * 4;                      // the frame image; MARKER: + kFxMarkParts x 16 bytes behind it

template <bool WINDOW, int OUT>
__global__ __launch_bounds__(kFftWide, 8) void fft_q15_kernel(const int16_t *__restrict__ in,
                                                               void *__restrict__ out, int batch,
                                                               SaQ15Params prm, const int16_t *__restrict__ rom,
                                                               const uint2 *__restrict__ tw, const uint4 *__restrict__ twrec,
                                                               unsigned mrange)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_q[];
    unsigned *buf = reinterpret_cast<unsigned *>(smem_q);     // [16384] packed (re, im)
    const int t = threadIdx.x;
    const int f = blockIdx.x;
    if (f >= batch) return;
    // ---- stage 0 straight from global memory: the thread's 16 positions t + 1024 m as 2-byte loads (128 contiguous
    // bytes per wave instruction), optional window, imag = 0 (new/command_control.vhd:123).  No staging pass
    // through LDS, no barrier in front of the first butterflies; outputs 4 bf + i' are one 16-byte LDS write.
    // Exponents with wi = -32768 (see fx_butterfly): stages 0 and 1, u = 3 for output 1, u = 1 for output 3.
    {
        const int16_t *xf = in + (size_t)f * SA_NPTS + t;
        int x[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) x[m] = xf[kFftWide * m];
        if constexpr (WINDOW) {
            int c[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) c[m] = rom[t + kFftWide * m];
#pragma unroll
            for (int m = 0; m < 16; ++m)
                x[m] = (prm.win_mode == SA_WIN_RTL_SIGNED) ? win_rtl(x[m], c[m]) : win_u16(x[m], c[m]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bf = t + kFftWide * u;                   // j' = bf, kappa = 0, e1 = bf
            unsigned o[4];
            const SaTw3 w = fx_twrec(twrec, bf);
            fx_butterfly_real(x[u], x[u + 4], x[u + 8], x[u + 12], w.w1, w.w2.x, w.w3, bf == 0, o, u == 3, u == 1);
            *reinterpret_cast<uint4 *>(buf + 4 * bf) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }

    // ---- stages 1..4 as two register passes of two stages each.  A thread that runs the stage-s butterflies
    // bf = t + 1024 u (u = 0..3) holds, in output i' of butterfly u, input u of the stage-(s+1) butterfly
    // ((j' mod 4^(5-s)) << (2s+2)) | (i' << 2s) | kappa -- its own four next butterflies, which all share ONE twiddle
    // exponent (j'' = (t >> 2s) mod 4^(5-s) does not depend on i').  One LDS exchange per two stages instead of one per
    // stage, a quarter of the twiddle loads in the second stage of a pass.
    //   outputs of the pass: pos = (j'' << (2s+4)) | (i'' << (2s+2)) | (i' << 2s) | kappa
    // Pass (1,2) writes with kappa = t & 3 in the bank bits: the words are stored at pos ^ ((j'' & 15) << 2), which spreads
    // the 16 values of j'' in a wave over the banks (conflict-free), and pass (3,4) reads t + 1024 m through the same
    // exchange of bits (there it permutes the lanes of a wave: conflict-free as well).
    unsigned v[16];
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    {
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = buf[t + kFftWide * m];
        __syncthreads();
        unsigned x[16];                                        // x[4 i' + u]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e1 = ((t + kFftWide * u) >> 2) << 2;
            unsigned o[4];
            // exponents with wi = -32768 (see fx_butterfly): output 1 at u = 3, output 3 at u = 1, output 2 at u = 1 or 2
            const SaTw3 w = fx_twrec(twrec, 4096 + (e1 >> 2));
            fx_butterfly(v[u], v[u + 4], v[u + 8], v[u + 12], w.w1, w.w2, w.w3, e1 == 0, o, u == 3, u == 1 || u == 2, u == 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * i + u] = o[i];
        }
        // stage 2: j'' = (t >> 2) & 255, exponent 16 j'' (never in 4082..4095; 3 e never in 4083..4110; 2 e = 4096 for
        // j'' = 128, i.e. threads 512..515: wave 8 takes the two-multiply form for output 2)
        const int j2 = (t >> 2) & 255, e2 = j2 << 4;
        const SaTw3 w2 = fx_twrec(twrec, 5120 + j2);
        const uint2 a1 = w2.w1, a2 = w2.w2, a3 = w2.w3;
        const int ob = ((j2 << 6) | (t & 3)) ^ ((j2 & 15) << 2);
#pragma unroll
        for (int ip = 0; ip < 4; ++ip) {
            unsigned o[4];
            if (wave == 8) fx_butterfly(x[4 * ip], x[4 * ip + 1], x[4 * ip + 2], x[4 * ip + 3], a1, a2, a3, false, o, false, true, false);
            else fx_butterfly(x[4 * ip], x[4 * ip + 1], x[4 * ip + 2], x[4 * ip + 3], a1, a2, a3, e2 == 0, o, false, false, false);
#pragma unroll
            for (int i = 0; i < 4; ++i) buf[ob ^ ((4 * i + ip) << 2)] = o[i];
        }
        __syncthreads();
    }
    {
        // pass (3,4): scalar twiddles in both stages (j' = wave + 16 u, then j'' = wave)
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = buf[(t + kFftWide * m) ^ (wave << 2)];
        __syncthreads();
        unsigned x[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e1 = (wave + 16 * u) << 6;
            unsigned o[4];
            fx_butterfly<true>(v[u], v[u + 4], v[u + 8], v[u + 12], tw[e1], tw[2 * e1], tw[3 * e1], e1 == 0, o, false, u == 2, false);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * i + u] = o[i];
        }
        const int e2 = wave << 8;                              // 2 e = 4096 for wave 8
        const uint2 a1 = tw[e2], a2 = tw[2 * e2], a3 = tw[3 * e2];
        const int ob = (wave << 10) | (t & 63);
#pragma unroll
        for (int ip = 0; ip < 4; ++ip) {
            unsigned o[4];
            if (wave == 8) fx_butterfly<true>(x[4 * ip], x[4 * ip + 1], x[4 * ip + 2], x[4 * ip + 3], a1, a2, a3, false, o, false, true, false);
            else fx_butterfly<true>(x[4 * ip], x[4 * ip + 1], x[4 * ip + 2], x[4 * ip + 3], a1, a2, a3, e2 == 0, o, false, false, false);
#pragma unroll
            for (int i = 0; i < 4; ++i) buf[ob | ((4 * i + ip) << 6)] = o[i];
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = buf[t + kFftWide * m];
    unsigned w[16];
    // stage 5 (4^s = 1024): j' = u, kappa = t; outputs land at m' = 4u + i'; exponents are compile-time
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        unsigned o[4];
        fx_butterfly<true>(v[u], v[u + 4], v[u + 8], v[u + 12], tw[u * 1024], tw[2 * u * 1024], tw[3 * u * 1024], u == 0, o, false,
                           u == 2, false);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[4 * u + i] = o[i];
    }
    // stage 6 (4^s = 4096): no twiddles; outputs at m' = u + 4 i' = natural-order bin t + 1024 m'
    // frame layout: [16384] x (re, im) int16 = 65536 bytes (imp/sequ2.vhd:153); one dword per lane
    // SA_Q15_OUT_MAG: the same dwords at the same offsets of a float row, each the magnitude of its bin.
    // SA_Q15_OUT_MARKER: no spectrum store; the thread keeps the 16 sums re^2 + im^2 of its bins and roots their largest.
    unsigned *o32 = reinterpret_cast<unsigned *>(reinterpret_cast<int16_t *>(out) + (size_t)f * SA_NPTS * 2);
    const int mlo = (int)(mrange & 0xFFFFu), mhi = (int)(mrange >> 16);
    float ms[16];
    unsigned long long mpow = 0ull;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        unsigned o[4];
        fx_butterfly(w[u], w[u + 4], w[u + 8], w[u + 12], make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), true, o, false,
                     false, false);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mp = u + 4 * i;
            if constexpr (OUT == SA_Q15_OUT_IQ)
                __builtin_nontemporal_store(o[i], o32 + t + kFftWide * mp);   // streaming: written once
            else if constexpr (OUT == SA_Q15_OUT_MAG)
                __builtin_nontemporal_store(fx_mag(o[i]), reinterpret_cast<float *>(o32) + t + kFftWide * mp);
            else
                ms[mp] = fx_mark_sum_any(mpow, o[i], t + kFftWide * mp, (wave << 6) + kFftWide * mp, mlo, mhi);
        }
    }
    if constexpr (OUT == SA_Q15_OUT_MARKER) {
        fx_mark_finish(fx_mark_thread(ms, t, mpow), reinterpret_cast<uint4 *>(smem_q + kFftLds), out, f, t, wave);
    }
}

template <int OUT>
hipError_t launch_fft_q15(const int16_t *in_time, void *out, int batch, bool apply_window, const SaQ15Params &p,
                          const SaQ15Tables &t, hipStream_t stream, SaLaunchEv ev)
{
    const dim3 grid(batch), block(kFftWide);
    const int lds = kFftLds + (OUT == SA_Q15_OUT_MARKER ? kFxMarkParts * (int)sizeof(uint4) : 0);
    auto k = apply_window ? fft_q15_kernel<true, OUT> : fft_q15_kernel<false, OUT>;
    const hipError_t e = sa_set_dyn_lds_once(reinterpret_cast<const void *>(k), lds);
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(k, grid, block, lds, stream, ev.start, ev.stop, 0, in_time, out, batch, p, t.rom, t.tw, t.twrec,
                          (unsigned)t.marker_lo | (unsigned)t.marker_hi << 16);
    return hipGetLastError();
}

}  // namespace

hipError_t sa_launch_fft_q15(const int16_t *in_time, void *out, int batch, int out_kind, bool apply_window,
                             const SaQ15Params &p, const SaQ15Tables &t, hipStream_t stream, SaLaunchEv ev)
{
    if (batch <= 0) return hipSuccess;
    switch (out_kind) {
        case SA_Q15_OUT_IQ: return launch_fft_q15<SA_Q15_OUT_IQ>(in_time, out, batch, apply_window, p, t, stream, ev);
        case SA_Q15_OUT_MAG: return launch_fft_q15<SA_Q15_OUT_MAG>(in_time, out, batch, apply_window, p, t, stream, ev);
        case SA_Q15_OUT_MARKER: return launch_fft_q15<SA_Q15_OUT_MARKER>(in_time, out, batch, apply_window, p, t, stream, ev);
        default: return hipErrorInvalidValue;
    }
}
