// p12_dev.hpp -- device side of the packed 12-bit sample format ("p12", include/specan.h: sample n in bits [12n, 12n+12)
// of the frame read as a little-endian bit stream, 24576 bytes per frame), shared by the float chain (chain_f32_dev.hpp)
// and the integer chain (cascade_q15.hip, fft_q15.hip).
#pragma once
#include <stdint.h>

namespace {

// A tag type over the bytes, so that no overload collides with a plain byte pointer.
struct SaP12 {
    uint8_t b;
};

// Eight samples from three dwords (96 bits): sign-extending bit-field extracts; samples 2 and 5 straddle a dword and
// come out of a funnel shift (v_alignbit_b32) first.
__device__ __forceinline__ int p12_bfe(unsigned w, int pos) { return (int)(w << (20 - pos)) >> 20; }
__device__ __forceinline__ void p12_unpack8(unsigned w0, unsigned w1, unsigned w2, int (&s)[8])
{
    s[0] = p12_bfe(w0, 0);
    s[1] = p12_bfe(w0, 12);
    s[2] = p12_bfe(__builtin_amdgcn_alignbit(w1, w0, 24), 0);
    s[3] = p12_bfe(w1, 4);
    s[4] = p12_bfe(w1, 16);
    s[5] = p12_bfe(__builtin_amdgcn_alignbit(w2, w1, 28), 0);
    s[6] = p12_bfe(w2, 8);
    s[7] = (int)w2 >> 20;
}

}  // namespace
