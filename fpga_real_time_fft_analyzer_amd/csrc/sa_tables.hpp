// sa_tables.hpp -- the formats of the constant tables (sa_tables.cpp): the windows in their device layouts, the float
// twiddles and the SA-FXFFT-1 twiddles with their per-butterfly records.  Each table is a contract with the kernel that
// indexes it (SaF32Tables, SaQ15Tables in sa_common.hpp) and this is the single place that fills them.  Pure arithmetic:
// no handle, no stream and no HIP runtime call, so tests/cpp/test_sa_tables.cpp checks every table without a GPU.
// Not exported by the library.
#pragma once
#include "sa_common.hpp"

#include <vector>

#pragma GCC visibility push(hidden)

// The default window, Hann in double (scripts/hann_coeff.py:3-4), and the Q15 window ROM made from it
void default_window_f64(std::vector<double> &w);
void default_rom(std::vector<int16_t> &rom);

// half = 0.5 * window (exact scaling, undone by the split step).  Two device copies, each arranged so
// that the kernel's loads are coalesced 16-byte accesses in the layout it computes in:
//   tr (IIR kernels, chunk layout):   tr[g][t] = w[64t + E g .. + E-1], E = 16 bytes / sizeof(T) (float: the half
//                                     window, [16][256] quads; double: the window of iir_f64.hip, [32][256] pairs)
//   pa (no-IIR kernel, pass-A layout): pa[p][t] = half[512(2p)+2t], [..+1], half[512(2p+1)+2t], [..+1]
void half_window(const std::vector<double> &w, std::vector<float> &half);
template <class T>
void transpose_window(const std::vector<T> &w, std::vector<T> &tr)
{
    constexpr int E = 16 / sizeof(T);
    tr.resize(SA_NPTS);
    for (int t = 0; t < 256; ++t)
        for (int g = 0; g < 64 / E; ++g)
            for (int e = 0; e < E; ++e) tr[(g * 256 + t) * E + e] = w[64 * t + E * g + e];
}
void pass_a_window(const std::vector<float> &half, std::vector<float> &pa);

// Is w[n] = a0 - a1 cos(2 pi n / (N-1)) to within float rounding?  (a0, a1) into out when it is.
bool fit_cosine_window(const float *w, double out[2]);

// SaF32Tables::twT [6][256], twB [8][16] and twC [25]
void float_twiddles(std::vector<float4> &twT, std::vector<float4> &twB, std::vector<float2> &twC);

// SaQ15Tables::tw [16384] and twrec [2 * kSaTwRecs].  False when an entry with wi = -32768 lies outside exponents
// 4082..4110: the kernel's compile-time choice of the butterflies that avoid the second word rests on that range.
bool q15_twiddles(std::vector<uint2> &tw, std::vector<uint4> &twrec);

#pragma GCC visibility pop
