// q15_dev.hpp -- device helpers shared by the integer cascades (cascade_q15.hip) and the fixed-point FFT (fft_q15.hip):
// the Q15 window of one sample and the packed int16 pair -- and, shared by the FFT's epilogues and the fold kernels
// (trace_fold_q15.hip, spectra_fold_q15.hip), the packed dot product, the float sum under the magnitude's root and the
// correctly rounded square root.
#pragma once
#include "sa_common.hpp"

namespace {

// new/hann8192.vhd:36-39: out = resize16(product(31..15) + product(14)).
// product(31..15) + product(14) = floor((p + 2^14) / 2^15); resize16 of the 17-bit sum keeps its sign bit (16) and its
// low 15 bits, which differs from plain truncation only for +32768 (x = c = -32768), mapped to 0.
__device__ __forceinline__ int win_rtl(int x, int c)
{
    const int r = (x * c + 16384) >> 15;
    return (int)(short)((r & 0x7FFF) | ((r >> 1) & 0x8000));
}

// SURVEY quirk Q2 alternative: ROM + 32768 as unsigned Q16 Hann, round half up.  |x (c + 32768) + 32768| < 2^31 for
// 16-bit x and c (largest 32767 * 65535 + 32768): 32-bit arithmetic is exact.
__device__ __forceinline__ int win_u16(int x, int c)
{
    return (int)(short)((x * (c + 32768) + 32768) >> 16);
}

__device__ __forceinline__ unsigned pack2(int lo, int hi) { return ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16); }
// (sat16(lo), sat16(hi)) as one packed dword: v_cvt_pk_i16_i32 saturates and packs in ONE instruction
// (two v_med3_i32, an and and a shift-or otherwise -- a seventh of the kernel's vector instructions)
__device__ __forceinline__ unsigned sat_pack2(int lo, int hi)
{
    typedef short s2 __attribute__((ext_vector_type(2)));
    const s2 r = __builtin_amdgcn_cvt_pk_i16(lo, hi);
    return __builtin_bit_cast(unsigned, r);
}

__device__ __forceinline__ int lo16(unsigned v) { return (int)(short)(v & 0xFFFFu); }
__device__ __forceinline__ int hi16(unsigned v) { return (int)v >> 16; }

// lo(a) lo(b) + hi(a) hi(b), exact in 32 bits.  Written out: the builtin is selected as the accumulating two-operand
// form v_dot2c_i32_i16, which costs a v_mov of zero into the accumulator per product.
__device__ __forceinline__ int fx_dot2(unsigned a, unsigned b)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// decode_mag_16iq_le (gui.py:250-260) is np.sqrt(re.astype(float32)**2 + im.astype(float32)**2): four float32 operations,
// each rounded on its own.  The two squares and their sum must therefore not be contracted into an FMA (hipcc's default
// is -ffp-contract=fast; squares are exact only up to |v| = 4096), and the root must be the correctly rounded one
// (fx_sqrt_rn below).  This is the sum under the root, s = fl(fl(re re) + fl(im im)), of one packed (re, im) word.
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

}  // namespace
