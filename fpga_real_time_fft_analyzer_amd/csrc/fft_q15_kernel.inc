// fft_q15_kernel.inc -- the text of the integer FFT's kernel, included by fft_q15.hip once per input form with
//   SA_FX_KERNEL  the kernel's name        SA_FX_IN  the element type of `in`
//   SA_FX_HOP_ARG  nothing, or `, int hop`: one more kernel argument        SA_FX_STRIDE  the frame stride fx_load16 takes
// defined: fft_q15_kernel on int16 samples and fft_q15_p12_kernel on packed 12-bit samples (p12_dev.hpp), frames back to
// back (a constant stride), and fft_q15_hop_kernel / fft_q15_hop_p12_kernel on frames cut from one stream (the stride from
// `hop`).  The forms differ in fx_load16 and its stride alone.  Text inclusion rather than a shared inlined body or one more template parameter: the
// int16 kernels keep their symbols and, instruction for instruction, the code they had before the packed form existed.
template <bool WINDOW, int OUT>
__global__ __launch_bounds__(kFftWide, 8) void SA_FX_KERNEL(const SA_FX_IN *__restrict__ in,
                                                             void *__restrict__ out, int batch,
                                                             SaQ15Params prm, const int16_t *__restrict__ rom,
                                                             const uint2 *__restrict__ tw, const uint4 *__restrict__ twrec,
                                                             unsigned mrange SA_FX_HOP_ARG)
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
        fx_load16(in, f, SA_FX_STRIDE, t, x);
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
