// fft_q15.hip -- SA-FXFFT-1 for gfx950 (MI355X): the fixed-point FFT that stands where ip/xfft_0 stands
// (radix-4 DIF, >>2 per stage, Q15 twiddles, truncation).  One 1024-thread workgroup per frame, data in LDS as packed
// (re,im) int16 pairs, Stockham (autosort) addressing so the result is in natural order, stages paired in registers; the
// arithmetic per butterfly is exactly oracle/specan_oracle.c:or_fxfft16k.  One kernel template, fft_q15_kernel, instantiated
// for int16 samples and for packed 12-bit samples (include/specan.h, "p12"; unpacked in stage 0), in frames or in one stream.
#include "q15_dev.hpp"
#include "p12_dev.hpp"
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

// fx_dot2, lo(a) lo(b) + hi(a) hi(b) exact in 32 bits: q15_dev.hpp (shared with spectra_fold_q15.hip)
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
// fx_mag_sum, the three uncontracted float operations under the root, and fx_sqrt_rn, the correctly rounded root: q15_dev.hpp
// (shared with trace_fold_q15.hip and spectra_fold_q15.hip)
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

// ---- SA_Q15_TRACE_KIND(k): one record {peak_mag, power} per bucket of W = 2^k consecutive bins (k = 1..6) -------------
// After stage 6 thread t holds bin t + 1024 m': a bucket is W adjacent lanes of one wave at one m', aligned to W, so the
// reduction is a xor butterfly over the lane bits 0..k-1 and never leaves the wave.  No LDS image, no barrier.
//   peak:  the float sums s = fl(fl(re re) + fl(im im)) are non-negative, so their order is the order of their bit
//          patterns: an unsigned maximum, then ONE root per bucket (the correctly rounded root is monotone).
//   power: the integer power re^2 + im^2 <= 2^31 goes as its two 16-bit halves; a bucket's sums of halves are at most
//          64 x 65535 < 2^22 and 64 x 32768 = 2^21, exact in 32 bits whatever the frame holds.  Both sums are exact as
//          floats (below 2^24), and so is hi 2^16; fma(hi, 2^16, lo) rounds the exact value hi 2^16 + lo ONCE, to
//          nearest even: the float32 nearest to the exact integer sum.
// The template value of the epilogue arm; the bucket width itself is a run-time word (the kernel's trailing argument).
constexpr int kFxOutTrace = SA_Q15_TRACE_KIND(0);
// SA_Q15_TRACE_AVG_KIND(k, a): the same reduction, stopped before the root and the two conversions -- the first lane of each
// bucket stores the bucket's FxTrace as one 16-byte partial record {s, hi, lo, 0} (hi 65536 + lo is the exact bucket power)
// into a [B, 16384 >> k] workspace, and trace_fold_q15.hip folds A = 2^a frames of such records into one trace point.
// The arm knows nothing of a: k alone rides in the trailing word.
constexpr int kFxOutTraceRaw = SA_Q15_TRACE_AVG_KIND(0, 0);

struct FxTrace {
    unsigned s, lo, hi;                                      // bits of max s; sums of the low / high halves of the power
};

// The store of a partial record: plain, so that the fold launch right behind finds the records in the cache hierarchy
// (-DSA_FX_RAW_NT: the nontemporal form, for the A/B of tools/q15_trace_avg_cost.py)
#ifdef SA_FX_RAW_NT
#define SA_FX_RAW_STORE(v, ptr) fx_store_nt4((v), (ptr))
__device__ __forceinline__ void fx_store_nt4(uint4 v, uint4 *p)
{
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    u4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u4 *>(p));
}
#else
#define SA_FX_RAW_STORE(v, ptr) (*(ptr) = (v))
#endif

// a <- a (+) the part of the lane that DPP control CTRL names (a lane inside the same row of 16)
template <int CTRL>
__device__ __forceinline__ void fx_trace_dpp(FxTrace &a)
{
    const unsigned s = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a.s, CTRL, 0xF, 0xF, true);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a.lo, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a.hi, CTRL, 0xF, 0xF, true);
    a.s = a.s > s ? a.s : s;
    a.lo += lo;
    a.hi += hi;
}

// One m' of a wave, K = log2 W.  The steps for lane bits 0..3 stay in the VALU: quad_perm [1,0,3,2] and [2,3,0,1] are
// lane ^ 1 and lane ^ 2; after them the four lanes of a quad agree, so row_half_mirror (lane 7 - i of the eight) reads the
// other quad's part, and after that the eight agree and row_mirror (lane 15 - i) reads the other eight's.  Bit 4 is one
// ds_swizzle (lane ^ 16, as in fx_mark_swizzle).  Bit 5 (W = 64: lane 0 alone stores) takes the upper half-wave's part from
// lane 32 through scalar registers.  All 64 lanes run every step; the first lane of each bucket stores its record.
// RAW (kFxOutTraceRaw): `row` is the frame's row of partial records, no root and no conversion.
template <int K, bool RAW = false>
__device__ __forceinline__ void fx_trace_point(unsigned p, int t, void *__restrict__ row, int bin)
{
    const unsigned pw = (unsigned)fx_dot2(p, p);
    FxTrace a = {__builtin_bit_cast(unsigned, fx_mag_sum(p)), pw & 0xFFFFu, pw >> 16};
    fx_trace_dpp<0xB1>(a);
    if constexpr (K >= 2) fx_trace_dpp<0x4E>(a);
    if constexpr (K >= 3) fx_trace_dpp<0x141>(a);
    if constexpr (K >= 4) fx_trace_dpp<0x140>(a);
    if constexpr (K >= 5) {
        constexpr int pat = (16 << 10) | 0x1F;
        const unsigned s = (unsigned)__builtin_amdgcn_ds_swizzle((int)a.s, pat);
        a.lo += (unsigned)__builtin_amdgcn_ds_swizzle((int)a.lo, pat);
        a.hi += (unsigned)__builtin_amdgcn_ds_swizzle((int)a.hi, pat);
        a.s = a.s > s ? a.s : s;
    }
    if constexpr (K >= 6) {
        const unsigned s = (unsigned)__builtin_amdgcn_readlane((int)a.s, 32);
        a.lo += (unsigned)__builtin_amdgcn_readlane((int)a.lo, 32);
        a.hi += (unsigned)__builtin_amdgcn_readlane((int)a.hi, 32);
        a.s = a.s > s ? a.s : s;
    }
    if constexpr (RAW) {
        if ((t & ((1 << K) - 1)) == 0) SA_FX_RAW_STORE(make_uint4(a.s, a.hi, a.lo, 0u), reinterpret_cast<uint4 *>(row) + (bin >> K));
        return;
    }
    const float peak = fx_sqrt_rn(__builtin_bit_cast(float, a.s));
    const float power = __builtin_fmaf((float)a.hi, 65536.f, (float)a.lo);
    if ((t & ((1 << K) - 1)) == 0)
        reinterpret_cast<uint2 *>(row)[bin >> K] = make_uint2(__builtin_bit_cast(unsigned, peak), __builtin_bit_cast(unsigned, power));
}

// The thread's 16 bins q[m'] = bin t + 1024 m' into the frame's row of 16384 >> K records: one straight-line block per
// width, so the sixteen reductions interleave and no step waits on the one before it.
template <int K, bool RAW>
__device__ __forceinline__ void fx_trace_rows(const unsigned (&q)[16], int t, void *__restrict__ out, int f)
{
    void *row = reinterpret_cast<unsigned char *>(out) + (size_t)f * (SA_NPTS >> K) * (RAW ? sizeof(uint4) : sizeof(uint2));
#pragma unroll
    for (int m = 0; m < 16; ++m) fx_trace_point<K, RAW>(q[m], t, row, t + kFftWide * m);
}

// k is wave-uniform (a kernel argument): one scalar branch per frame
template <bool RAW>
__device__ __forceinline__ void fx_trace_frame(const unsigned (&q)[16], int k, int t, void *__restrict__ out, int f)
{
    switch (k) {
        case 1: fx_trace_rows<1, RAW>(q, t, out, f); break;
        case 2: fx_trace_rows<2, RAW>(q, t, out, f); break;
        case 3: fx_trace_rows<3, RAW>(q, t, out, f); break;
        case 4: fx_trace_rows<4, RAW>(q, t, out, f); break;
        case 5: fx_trace_rows<5, RAW>(q, t, out, f); break;
        case 6: fx_trace_rows<6, RAW>(q, t, out, f); break;
        default: break;                                      // the host admits 1..6 only
    }
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
// arguments, so the other kinds' argument loads are where they were) -- or, OUT = kFxOutTrace, the bucket records of
// SA_Q15_TRACE_KIND(k), for which the same trailing word carries k.
constexpr int kFftLds = SA_NPTS * 4;                      // the frame image; MARKER: + kFxMarkParts x 16 bytes behind it

// Stage 0's samples of thread t, x[m] = sample t + 1024 m of frame f.  int16 samples: 2-byte loads, 128 contiguous bytes
// per wave instruction.  Frame f begins `stride` samples after frame f - 1 (fx_stride): SA_NPTS, a constant, where the
// frames lie back to back, the hop where they are cut from one stream (the kernel's trailing `int hop`).
__device__ __forceinline__ void fx_load16(const int16_t *in, int f, size_t stride, int t, int (&x)[16])
{
    const int16_t *xf = in + (size_t)f * stride + t;
#pragma unroll
    for (int m = 0; m < 16; ++m) x[m] = xf[kFftWide * m];
}
__device__ __forceinline__ size_t fx_stride(const int16_t *) { return (size_t)SA_NPTS; }
__device__ __forceinline__ size_t fx_stride(const int16_t *, int hop) { return (size_t)hop; }
// Packed 12-bit samples (include/specan.h; a frame is 6144 dwords, every frame 16-byte aligned): sample n sits at bit 12 n,
// so sample t + 1024 m begins in dword (12 t >> 5) + 384 m at bit sh = 12 t & 31, the same for all 16 m.  It reaches into
// the next dword only where sh > 20, i.e. sh = 24 or 28, t mod 8 = 2 or 5.  Two aligned dword loads (a wave instruction
// covers 96 contiguous bytes), a funnel shift by sh and a sign-extending extract of the low 12 bits.  The second load
// takes the next dword ONLY in the straddling lanes and the first dword again in all others (where the funnel shift's
// upper input does not reach the 12 bits kept): the frame's last dword, 6143, is the first dword of t = 1022 (sh = 8) and
// t = 1023 (sh = 20) at m = 15, neither of which straddles, so no index exceeds 6143 and no byte outside
// [in, in + B * 24576) is read -- by the address map, not by slack behind the tensor.  `stride` is in dwords: 6144 for
// frames back to back; 3 hop / 8 for frames cut from one stream (hop a multiple of 8: every frame begins on a dword, and
// dwords are all this map reads).  The argument above is per frame, so the last frame of a stream ends with the stream.
constexpr int kP12FrameDwords = SA_P12_FRAME_BYTES / 4;
__device__ __forceinline__ void fx_load16(const SaP12 *in, int f, size_t stride, int t, int (&x)[16])
{
    const int bit = 12 * t, sh = bit & 31;
    const unsigned *lo = reinterpret_cast<const unsigned *>(in) + (size_t)f * stride + (bit >> 5);
    const unsigned *hi = lo + (sh > 20 ? 1 : 0);
    constexpr int step = 12 * kFftWide / 32;                  // dwords from sample n to sample n + 1024
#pragma unroll
    for (int m = 0; m < 16; ++m)
        x[m] = p12_bfe(__builtin_amdgcn_alignbit(hi[step * m], lo[step * m], (unsigned)sh), 0);
}
__device__ __forceinline__ size_t fx_stride(const SaP12 *) { return (size_t)kP12FrameDwords; }
__device__ __forceinline__ size_t fx_stride(const SaP12 *, int hop) { return (size_t)(3 * hop / 8); }

// The integer FFT's kernel, one template for every input form: InT is int16_t or SaP12 (packed 12-bit samples, p12_dev.hpp),
// and Hop is empty for frames back to back -- no further kernel argument, a constant stride -- or `int` for frames cut from
// one stream: the hop in samples, one more kernel argument behind `mrange`.  The forms share every line below and differ in
// fx_load16 and its stride (fx_stride) alone.  A template on the input form, not a shared inlined body: the body inlined into
// one kernel per form changed the int16 kernels' instruction streams, the template leaves every instantiation the code
// it had as a kernel of its own name.  Instantiated: WINDOW = false for <int16_t, ...> without a
// hop alone (the FFT behind a cascade); packed samples and streams come from the caller only, unwindowed (filter mode 0xB1).
template <typename InT, bool WINDOW, int OUT, typename... Hop>
__global__ __launch_bounds__(kFftWide, 8) void fft_q15_kernel(const InT *__restrict__ in, void *__restrict__ out, int batch,
                                                               SaQ15Params prm, const int16_t *__restrict__ rom,
                                                               const uint2 *__restrict__ tw, const uint4 *__restrict__ twrec,
                                                               unsigned mrange, Hop... hop)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_q[];
    unsigned *buf = reinterpret_cast<unsigned *>(smem_q);     // [16384] packed (re, im)
    const int t = threadIdx.x;
    const int f = blockIdx.x;
    if (f >= batch) return;
    // ---- stage 0 straight from global memory: the thread's 16 positions t + 1024 m (fx_load16: 2-byte loads of int16
    // samples, or dword loads and an unpack of packed ones), optional window, imag = 0 (new/command_control.vhd:123).
    // No staging pass through LDS, no barrier in front of the first butterflies; outputs 4 bf + i' are one 16-byte LDS
    // write.
    // Exponents with wi = -32768 (see fx_butterfly): stages 0 and 1, u = 3 for output 1, u = 1 for output 3.
    {
        int x[16];
        fx_load16(in, f, fx_stride(in, hop...), t, x);
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
    // kFxOutTrace: no spectrum store either; the thread keeps its 16 bins, then per m' the wave reduces its 64 bins to
    // 64 / W records (W = 1 << mrange) and the first lane of each bucket stores one: row [16384 / W] of the frame
    // (fx_trace_frame).  kFxOutTraceRaw: the same reduction, the bucket's partial record {s, hi, lo, 0} stored instead
    // (row [16384 / W] of 16-byte records in the workspace `out`).
    unsigned *o32 = reinterpret_cast<unsigned *>(reinterpret_cast<int16_t *>(out) + (size_t)f * SA_NPTS * 2);
    const int mlo = (int)(mrange & 0xFFFFu), mhi = (int)(mrange >> 16);
    float ms[16];
    unsigned long long mpow = 0ull;
    unsigned tq[16];
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
            else if constexpr (OUT == SA_Q15_OUT_MARKER)
                ms[mp] = fx_mark_sum_any(mpow, o[i], t + kFftWide * mp, (wave << 6) + kFftWide * mp, mlo, mhi);
            else
                tq[mp] = o[i];
        }
    }
    if constexpr (OUT == SA_Q15_OUT_MARKER) {
        fx_mark_finish(fx_mark_thread(ms, t, mpow), reinterpret_cast<uint4 *>(smem_q + kFftLds), out, f, t, wave);
    }
    if constexpr (OUT == kFxOutTrace) fx_trace_frame<false>(tq, (int)mrange, t, out, f);
    if constexpr (OUT == kFxOutTraceRaw) fx_trace_frame<true>(tq, (int)mrange, t, out, f);
}

// `log2w`: the k of SA_Q15_TRACE_KIND(k), which rides in the kernel's trailing word in place of the marker range;
// `hop`: nothing for frames back to back, the hop in samples for frames cut from one stream (the kernel's trailing argument)
template <int OUT, bool WINDOW, typename InT, typename... Hop>
hipError_t launch_fft_q15(const InT *in_time, void *out, int batch, const SaQ15Params &p, const SaQ15Tables &t, int log2w,
                          hipStream_t stream, SaLaunchEv ev, Hop... hop)
{
    const auto k = fft_q15_kernel<InT, WINDOW, OUT, Hop...>;
    const dim3 grid(batch), block(kFftWide);
    const int lds = kFftLds + (OUT == SA_Q15_OUT_MARKER ? kFxMarkParts * (int)sizeof(uint4) : 0);
    const hipError_t e = sa_set_dyn_lds_once(reinterpret_cast<const void *>(k), lds);
    if (e != hipSuccess) return e;
    const unsigned word = OUT == kFxOutTrace || OUT == kFxOutTraceRaw ? (unsigned)log2w : (unsigned)t.marker_lo | (unsigned)t.marker_hi << 16;
    hipExtLaunchKernelGGL(k, grid, block, lds, stream, ev.start, ev.stop, 0, in_time, out, batch, p, t.rom, t.tw, t.twrec, word,
                          hop...);
    return hipGetLastError();
}

// hop = 0: frames back to back; otherwise `in_time` is one stream and frame f begins at sample f hop.  The caller has
// refused unwindowed input in any form but int16 frames.
template <int OUT>
hipError_t launch_fft_q15(const void *in_time, SaInKind in_kind, int hop, void *out, int batch, bool apply_window,
                          const SaQ15Params &p, const SaQ15Tables &t, int log2w, hipStream_t stream, SaLaunchEv ev)
{
    const int16_t *i16 = static_cast<const int16_t *>(in_time);
    const SaP12 *p12 = static_cast<const SaP12 *>(in_time);
    if (hop != 0 && in_kind == SaInKind::P12) return launch_fft_q15<OUT, true>(p12, out, batch, p, t, log2w, stream, ev, hop);
    if (hop != 0) return launch_fft_q15<OUT, true>(i16, out, batch, p, t, log2w, stream, ev, hop);
    if (in_kind == SaInKind::P12) return launch_fft_q15<OUT, true>(p12, out, batch, p, t, log2w, stream, ev);
    return apply_window ? launch_fft_q15<OUT, true>(i16, out, batch, p, t, log2w, stream, ev)
                        : launch_fft_q15<OUT, false>(i16, out, batch, p, t, log2w, stream, ev);
}

}  // namespace

hipError_t sa_launch_fft_q15(const void *in_time, SaInKind in_kind, int hop, void *out, int batch, int out_kind, bool apply_window,
                             const SaQ15Params &p, const SaQ15Tables &t, hipStream_t stream, SaLaunchEv ev)
{
    if (hop != 0 && (hop < 0 || hop > SA_NPTS || hop % 8 != 0)) return hipErrorInvalidValue;
    if (in_kind != SaInKind::I16 && in_kind != SaInKind::P12) return hipErrorInvalidValue;
    // unwindowed input is a cascade's output alone: int16 frames
    if (!apply_window && (in_kind != SaInKind::I16 || hop != 0)) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    if (out_kind >= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MIN) && out_kind <= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MAX))
        return launch_fft_q15<kFxOutTrace>(in_time, in_kind, hop, out, batch, apply_window, p, t, out_kind - kFxOutTrace, stream, ev);
    // the grouped kind: `out` is the workspace of partial records [B, 16384 >> k]; the group size is the fold launch's alone
    if (SA_Q15_IS_TRACE_AVG_KIND(out_kind))
        return launch_fft_q15<kFxOutTraceRaw>(in_time, in_kind, hop, out, batch, apply_window, p, t, SA_Q15_TRACE_AVG_LOG2W(out_kind), stream, ev);
    switch (out_kind) {
        case SA_Q15_OUT_IQ: return launch_fft_q15<SA_Q15_OUT_IQ>(in_time, in_kind, hop, out, batch, apply_window, p, t, 0, stream, ev);
        case SA_Q15_OUT_MAG: return launch_fft_q15<SA_Q15_OUT_MAG>(in_time, in_kind, hop, out, batch, apply_window, p, t, 0, stream, ev);
        case SA_Q15_OUT_MARKER:
            return launch_fft_q15<SA_Q15_OUT_MARKER>(in_time, in_kind, hop, out, batch, apply_window, p, t, 0, stream, ev);
        default: return hipErrorInvalidValue;
    }
}
