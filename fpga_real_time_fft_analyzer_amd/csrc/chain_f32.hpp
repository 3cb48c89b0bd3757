// chain_f32.hpp -- fused float signal path for gfx950 (MI355X):
//     Hann window -> 6-section biquad cascade -> 16384-point real FFT -> magnitude
// replacing new/hann8192.vhd -> new/filter_iir12_cust.vhd -> ip/xfft_0 of the reference with one
// pass over HBM (read 64 KiB, write 64 KiB per frame).  One 256-thread workgroup per frame.
//
// Shape of the computation (DESIGN.md sections 3-5):
//   * LDS holds HALF a frame at a time (34 KiB of image, 38.3 KiB per workgroup with the scan scratch, the per-lane scan
//     matrices and the pass-B twiddles) so that four workgroups share a CU
//     (16 waves): every exchange is done in two index-split rounds.  The kernel is latency bound
//     at lower occupancy (profiles/r1_phase_stamps_iir.txt).
//   * thread t owns samples [64t, 64t+64) for the IIR as two chunks of 32 held as float pairs
//     (chunk A in .x, chunk B in .y) so the serial recursion runs on packed-fp32 instructions.
//   * per section: the end state of every chunk from zero state is a dot product ("predict", fused
//     into the previous section's recursion loop); an affine scan over the 512 chunks of the frame
//     (in-row DPP shifts, one LDS hop for the 16 row totals) turns those into true start states;
//     then the exact DF2T recursion of scipy.signal.sosfilt runs from them.
//   * the real FFT is an 8192-point complex FFT of z[m] = x[2m] + i x[2m+1] factored 32 x 16 x 16,
//     each factor in registers (fft_regs.hpp), then the split step X[k] = Xe[k] + W_N^k Xo[k].
//     Taps and scan matrices live in the section's pole coordinates (sa_common.hpp): float32 accuracy
//     then matches a sequential evaluation also for poles next to the real axis.
//   * all 16384 magnitudes are written (upper half mirrored) as aligned 16-byte nontemporal stores, or, for
//     SA_OUT_MARKER, reduced in place to one 16-byte record per frame (peak, its bin, band power).
// The factor 1/2 of the split step is folded into the window table (exact in binary fp).
//
// The kernels are templates on the input type InT: float32 frames (chain_f32.hip: sa_process_f32), int16 samples
// (chain_f32_i16.hip: sa_process_f32_i16 -- what the board's ADC path delivers, imp/dsp_system_top.vhd:435 -- converted
// and scaled in the stage-in) or the same samples packed to 12 bits (chain_f32_p12.hip: sa_process_f32_p12, unpacked in
// the stage-in).  Everything behind the stage-in is the same code.  The entry points live in one translation unit each
// so that the parts of the build compile side by side.
#pragma once
#include <type_traits>
#include "chain_f32_dev.hpp"

namespace {

// The input of a kernel: `const InT *in`, and for int16 samples the scale right behind it, x = float(sample) * scale.
// The float32 kernels take no scale (their argument layout has no slot for one): the kernels' parameter pack Scale... is
// empty for float32 and one float for int16 and packed samples, and in_scale_of turns it into the scale.
__device__ __forceinline__ float in_scale_of() { return 1.f; }          // float32 frames: not scaled, never read
__device__ __forceinline__ float in_scale_of(float s) { return s; }

constexpr int kThreads = 256;
constexpr int kLdsComplex = 16 * 272;                 // half-frame exchange image (4352 complex)
constexpr int kScrOff = kLdsComplex * 8;              // scan scratch: 6 sections x 16 rows x float2
constexpr int kSideOff = kScrOff + 6 * 16 * 8;        // one complex side slot (Z[6144])
constexpr int kLaneOff = kSideOff + 16;               // (two complex side slots) then the per-lane matrices P2^i: 6 x 16 x float4
constexpr int kTwbOff = kLaneOff + 6 * 16 * 16;       // the pass-B twiddles (SaF32Tables::twB): 8 x 16 x float4, 2 KiB
constexpr int kTwbBytes = 8 * 16 * 16;
constexpr int kLdsBytes = kTwbOff + kTwbBytes;        // 39 184 bytes: four workgroups per CU take 156 736 of 163 840
constexpr int kOneRoundImage = 65536;                 // the bypassed chain at small batches: a whole float32 frame at once,
constexpr int kLdsOneRound = kOneRoundImage + kTwbBytes;   // with the pass-B twiddles behind the image
constexpr int kOneRoundMax = 512;                     // ... up to this batch size (launch_spectrum)
static_assert(kTwbOff <= kOneRoundImage, "the exchange images and side slots live inside the one-round image");
static_assert(4 * kLdsBytes <= 160 * 1024, "four workgroups share a CU's LDS");

// The two-component scan state travels as ONE register pair and every 2x2 matrix is stored column-major (a column is
// an aligned register pair): a matrix-vector product is two packed FMAs, column x broadcast component -- for wave-uniform
// matrices straight from their scalar registers.  (Round 3, tools/ubench/valu_throughput.hip: on gfx950 a plain fp32
// instruction with a scalar or DPP operand costs what a packed one costs, so four scalar FMAs per product were four
// packed-instruction slots.)
//   mv_s / mv_v: r = add + c0 * v.x + c1 * v.y with wave-uniform (SGPR) / per-lane (VGPR) columns;  mv_acc_s: in place
__device__ __forceinline__ v2f mv_s(const v2f c0, const v2f c1, const v2f v, const v2f add)
{
    v2f r;
    asm("v_pk_fma_f32 %0, %1, %3, %4 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "=&v"(r) : "s"(c0), "s"(c1), "v"(v), "v"(add));
    return r;
}
__device__ __forceinline__ v2f mv_v(const v2f c0, const v2f c1, const v2f v, const v2f add)
{
    v2f r;
    asm("v_pk_fma_f32 %0, %1, %3, %4 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "=&v"(r) : "v"(c0), "v"(c1), "v"(v), "v"(add));
    return r;
}
__device__ __forceinline__ v2f mv0_s(const v2f c0, const v2f c1, const v2f v)          // c0 * v.x + c1 * v.y
{
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %3 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "=&v"(r) : "s"(c0), "s"(c1), "v"(v));
    return r;
}
__device__ __forceinline__ void mv_acc_s(v2f &z, const v2f c0, const v2f c1, const v2f v)
{
    asm("v_pk_fma_f32 %0, %1, %3, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "+v"(z) : "s"(c0), "s"(c1), "v"(v));
}

// z <- z + P * shifted(z): one Kogge-Stone level of the affine scan inside a row (two DPP moves, two packed FMAs)
template <int N, typename MatT>
__device__ __forceinline__ void scan_level(v2f &z, const MatT &p)
{
    const v2f u = {row_shr<N>(z.x), row_shr<N>(z.y)};
    mv_acc_s(z, v2f{p[0], p[1]}, v2f{p[2], p[3]}, u);
}

__device__ __forceinline__ float mul_to(float a, float b)
{
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---------------------------------------------------------------------------------------------
// Stage-in for the IIR through the row image (chain_f32_dev.hpp, dma_rows): each thread reads its own row and multiplies
// by the window, which the host stored transposed (wint[g][t] = window[64t + 4g .. +3]) so that its loads are coalesced
// in this layout.  Thread t ends with d[j] = (x[64t + j], x[64t + 32 + j]) * window.
//
// Integer samples in (InT = int16_t or SaP12): ONE round of the LDS-DMA brings the whole frame (int16: 128 bytes per thread,
// 32 KiB; packed 12-bit: 96 bytes per thread, 24 KiB), and the forms differ only in the reader that gets samples 8g .. 8g+7
// of chunk A and of chunk B out of the row (chain_f32_dev.hpp: row_open, row_step).  x = float(sample) * scale is rounded
// once and then takes the window exactly as a float32 input sample does, so the results are those of sa_process_f32 on the
// converted frame, bit for bit, and the packed form's are those of the int16 form on the sign-extended samples.
template <bool WINGEN, typename InT>
__device__ __forceinline__ void stage_in_chunks(const InT *__restrict__ xin, const float in_scale,
                                                const float4 *__restrict__ wint, const SaIirLaneTab *__restrict__ lt,
                                                unsigned char *smem, int t, v2f (&d)[32])
{
    const int lane = t & 63, wave = t >> 6;
    float4 pq = make_float4(0.f, 0.f, 0.f, 0.f);               // the window generator: see the float32 form below
    float g0 = 0.f;
    if constexpr (WINGEN) {
        pq = *reinterpret_cast<const float4 *>(&lt->wgen[t][0]);
        g0 = lt->wg0;
    }
    // the rows are wave-private: the wave waits for its own DMA, and nothing of the window arithmetic is scheduled
    // above the wait (float32 form below)
    dma_rows(xin, smem, lane, wave);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const v2f Pw = {pq.x, pq.z}, Qw = {pq.y, pq.w}, G0 = {g0, g0}, sc = {in_scale, in_scale};
    unsigned row[2][12];                                       // packed form: the 12 dwords of chunk A and of chunk B
    row_open(xin, smem, t, row);
#pragma unroll
    for (int g = 0; g < 4; ++g) {                              // samples 8g .. 8g+7 of chunk A and of chunk B
        int sa[8], sb[8];
        row_step(xin, smem, t, row, 0, g, sa);
        row_step(xin, smem, t, row, 1, g, sb);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                          // four samples of either chunk at a time
            float4 wa = make_float4(0.f, 0.f, 0.f, 0.f), wb = wa;
            if constexpr (!WINGEN) {                           // table window: win_t[g'][t] = window at 64 t + 4 g' .. + 3
                wa = *at_bytes(wint + (2 * g + u) * 256, 16u * (unsigned)t);
                wb = *at_bytes(wint + (8 + 2 * g + u) * 256, 16u * (unsigned)t);
            }
            const float fa[4] = {wa.x, wa.y, wa.z, wa.w}, fb[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                const int e = 4 * u + e4, j = 8 * g + e;
                const v2f x = v2f{(float)sa[e], (float)sb[e]} * sc;   // rounded once: the float32 sample
                v2f w;
                if constexpr (WINGEN) {
                    const v2f cs = {lt->wcs[j][0], lt->wcs[j][1]};
                    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
                        "v_pk_fma_f32 %0, %4, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
                        : "=&v"(w) : "v"(Pw), "s"(cs), "v"(G0), "v"(Qw));
                } else {
                    w = v2f{fa[e4], fb[e4]};
                }
                d[j] = x * w;
            }
        }
    }
}

// float32 frames in: two rounds, round h brings chunk h (32 samples = 128 bytes) of every thread.
template <bool WINGEN>
__device__ __forceinline__ void stage_in_chunks(const float *__restrict__ xin, float, const float4 *__restrict__ wint,
                                                const SaIirLaneTab *__restrict__ lt, unsigned char *smem, int t,
                                                v2f (&d)[32])
{
    const float4 *lds4 = reinterpret_cast<const float4 *>(smem);
    const int lane = t & 63, wave = t >> 6;
    // WINGEN: the window is a0 - a1 cos(2 pi n / (N-1)) (Hann, Hamming; what scripts/hann_coeff.py:3-4 generates) and is
    // evaluated in place by the angle-addition formula: with n = 64 t + 32 h + j,
    //   W[n] = G0 + P_h c_j + Q_h s_j,   c_j = cos(theta j), s_j = sin(theta j) wave-uniform (scalar loads),
    //   (P_h, Q_h) = S a1 (-cos, sin)(theta (64 t + 32 h)) per thread and chunk, G0 = S a0, S = 0.5 * cascade gain.
    // The 64 KiB per-frame read of the window table (L2 -> L1, 16 more loads per thread) is gone.  !WINGEN (any other
    // window): the transposed table.
    float4 pq = make_float4(0.f, 0.f, 0.f, 0.f);
    float g0 = 0.f;
    if constexpr (WINGEN) {
        pq = *reinterpret_cast<const float4 *>(&lt->wgen[t][0]);
        g0 = lt->wg0;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // The image is WAVE-PRIVATE, so no workgroup barrier: a wave waits for its own DMA (vmcnt) and, before
        // overwriting the rows with round 1, for its own reads of round 0 (lgkmcnt).  Three barriers fewer per
        // frame; a wave delayed on its SIMD no longer holds the other three here.
        if (h == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dma_rows(xin, h, smem, lane, wave);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // nothing of the window arithmetic below may be scheduled above the wait (register-only instructions do
        // cross an asm statement): computed early, the 32 window values of the round sit in registers and spill
        __builtin_amdgcn_sched_barrier(0);
        const int sw = row_swizzle(t);
        // WINGEN: round 0 evaluates the window of BOTH chunks as pairs (chunk A, chunk B) -- two packed FMAs per pair with
        // the wave-uniform (c_j, s_j) in a scalar pair -- multiplies chunk A and parks chunk B's factor in the pair's
        // other half, where round 1 multiplies it in place.  (Per sample it used to be two scalar-operand FMAs, each of
        // which costs a packed-instruction slot on gfx950: tools/ubench/valu_throughput.hip.)
        const v2f Pw = {pq.x, pq.z}, Qw = {pq.y, pq.w}, G0 = {g0, g0};
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            // two batches of four units: all eight in flight at once push the kernel over 128 VGPRs
            if (g == 4) __builtin_amdgcn_sched_barrier(0);
            const float4 q = lds4[t * 8 + (g ^ sw)];
            const float qv[4] = {q.x, q.y, q.z, q.w};
            if constexpr (WINGEN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * g + e;
                    if (h == 0) {
                        const v2f cs = {lt->wcs[j][0], lt->wcs[j][1]};
                        v2f w;
                        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
                            "v_pk_fma_f32 %0, %4, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
                            : "=&v"(w) : "v"(Pw), "s"(cs), "v"(G0), "v"(Qw));
                        d[j].x = mul_to(qv[e], w.x);
                        d[j].y = w.y;
                    } else {
                        d[j].y = mul_to(qv[e], d[j].y);
                    }
                }
            } else {
                const float4 w = *at_bytes(wint + (8 * h + g) * 256, 16u * (unsigned)t);
                // mul_to: one v_mul_f32 straight into its half of the (chunk A, chunk B) pair.  Left to the
                // SLP vectoriser the two rounds become v_pk_mul_f32 on re-paired operands: ~100 v_mov per thread.
                if (h == 0) {
                    d[4 * g + 0].x = mul_to(q.x, w.x);
                    d[4 * g + 1].x = mul_to(q.y, w.y);
                    d[4 * g + 2].x = mul_to(q.z, w.z);
                    d[4 * g + 3].x = mul_to(q.w, w.w);
                } else {
                    d[4 * g + 0].y = mul_to(q.x, w.x);
                    d[4 * g + 1].y = mul_to(q.y, w.y);
                    d[4 * g + 2].y = mul_to(q.z, w.z);
                    d[4 * g + 3].y = mul_to(q.w, w.w);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Predictor taps.  (m1, m2) is one wave-uniform tap pair in an aligned SGPR pair; the chunk-end states of chunk A and
// chunk B (from zero state) accumulate as (z1, z2) pairs: nA += tap * y.x, nB += tap * y.y.  Eight taps in one statement
// (the compiler pads a wait state after every asm statement whose output the next one reads; 32 single-tap statements =
// 32 pads per section).  Two accumulator sets alternate: a dependent FMA every fourth instruction.
// FIRST_A / FIRST_B: the statement holds the first tap of the (nAa, nBa) / (nAb, nBb) chains, which is then a packed
// multiply into a fresh register pair (tap_mul beside tap_fma): no accumulator is zeroed first.  fma(t, y, 0) and t * y
// round alike, so the sums are the same bits but for the sign of an exact zero.
template <bool FIRST_A, bool FIRST_B>
__device__ __forceinline__ void tap_fma8(v2f &nAa, v2f &nBa, v2f &nAb, v2f &nBb, const v2f (&tp)[8], const v2f (&y)[8])
{
#define SA_TAP(ACCA, ACCB, T, Y)                                                               \
    "v_pk_fma_f32 %[" ACCA "], %[" T "], %[" Y "], %[" ACCA "] op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t" \
    "v_pk_fma_f32 %[" ACCB "], %[" T "], %[" Y "], %[" ACCB "] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define SA_TAP_MUL(ACCA, ACCB, T, Y)                                       \
    "v_pk_mul_f32 %[" ACCA "], %[" T "], %[" Y "] op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
    "v_pk_mul_f32 %[" ACCB "], %[" T "], %[" Y "] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
#define SA_TAPS_2_7                                                                                        \
    SA_TAP("a1", "a2", "t2", "y2") SA_TAP("b1", "b2", "t3", "y3") SA_TAP("a1", "a2", "t4", "y4")           \
        SA_TAP("b1", "b2", "t5", "y5") SA_TAP("a1", "a2", "t6", "y6") SA_TAP("b1", "b2", "t7", "y7") ""
#define SA_TAP_INS                                                                                                          \
    [t0] "s"(tp[0]), [t1] "s"(tp[1]), [t2] "s"(tp[2]), [t3] "s"(tp[3]), [t4] "s"(tp[4]), [t5] "s"(tp[5]), [t6] "s"(tp[6]),  \
        [t7] "s"(tp[7]), [y0] "v"(y[0]), [y1] "v"(y[1]), [y2] "v"(y[2]), [y3] "v"(y[3]), [y4] "v"(y[4]), [y5] "v"(y[5]),    \
        [y6] "v"(y[6]), [y7] "v"(y[7])
    if constexpr (FIRST_A && FIRST_B)
        asm(SA_TAP_MUL("a1", "a2", "t0", "y0") SA_TAP_MUL("b1", "b2", "t1", "y1") SA_TAPS_2_7
            : [a1] "=&v"(nAa), [a2] "=&v"(nBa), [b1] "=&v"(nAb), [b2] "=&v"(nBb)
            : SA_TAP_INS);
    else if constexpr (FIRST_B)
        asm(SA_TAP("a1", "a2", "t0", "y0") SA_TAP_MUL("b1", "b2", "t1", "y1") SA_TAPS_2_7
            : [a1] "+v"(nAa), [a2] "+v"(nBa), [b1] "=&v"(nAb), [b2] "=&v"(nBb)
            : SA_TAP_INS);
    else {
        static_assert(!FIRST_A, "the (nAa, nBa) chains never start alone");
        asm(SA_TAP("a1", "a2", "t0", "y0") SA_TAP("b1", "b2", "t1", "y1") SA_TAPS_2_7
            : [a1] "+v"(nAa), [a2] "+v"(nBa), [b1] "+v"(nAb), [b2] "+v"(nBb)
            : SA_TAP_INS);
    }
#undef SA_TAP_INS
#undef SA_TAPS_2_7
#undef SA_TAP_MUL
#undef SA_TAP
}

// The predictor of one section over the thread's 32 fresh pairs y = (chunk A, chunk B): chunk end states from zero state,
//   z = A^16 (sum_{j<16} m[j] y[j]) + sum_{j<16} m[j] y[16 + j]     (SaIirSecK::mnext; block Horner over two half chunks:
// the same sixteen tap pairs serve both halves and stay in their scalar registers).
__device__ __forceinline__ void predict_chunk_ends(const v2f (&tp)[16], const v2f q0, const v2f q1, const v2f (&d)[32],
                                                   v2f &zA, v2f &zB)
{
    // four accumulators: each chain sees a dependent FMA every fourth instruction.  None is zeroed: the first tap of a
    // chain is a multiply (tap_fma8<FIRST_A, FIRST_B>)
    v2f nAa, nBa, nAb, nBb;
    const auto y8_at = [&](int o, v2f (&y8)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) y8[i] = d[o + i];
    };
    const v2f tlo[8] = {tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], tp[6], tp[7]};
    const v2f thi[8] = {tp[8], tp[9], tp[10], tp[11], tp[12], tp[13], tp[14], tp[15]};
    v2f y8[8];
    y8_at(0, y8);
    tap_fma8<true, true>(nAa, nBa, nAb, nBb, tlo, y8);
    y8_at(8, y8);
    tap_fma8<false, false>(nAa, nBa, nAb, nBb, thi, y8);
    nAa = mv0_s(q0, q1, nAa + nAb);
    nBa = mv0_s(q0, q1, nBa + nBb);
    y8_at(16, y8);
    tap_fma8<false, true>(nAa, nBa, nAb, nBb, tlo, y8);
    y8_at(24, y8);
    tap_fma8<false, false>(nAa, nBa, nAb, nBb, thi, y8);
    zA = nAa + nAb;
    zB = nBa + nBb;
}

// The wave-uniform constants of one section, read one section ahead (while the previous section's loops run)
// so that their scalar-load latency is not on the path between two sections.
struct SecConsts {
    v2f pc0, pc1, mb0, mb1;            // columns of Pc and of T^-1
    float b0, b1, b2, a1, a2, flags_bits;     // flags travel as raw bits
};
template <typename SecT>
__device__ __forceinline__ SecConsts load_consts(const SecT &k)
{
    return {v2f{k.pc[0], k.pc[1]}, v2f{k.pc[2], k.pc[3]}, v2f{k.mback[0], k.mback[1]}, v2f{k.mback[2], k.mback[3]},
            k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], __builtin_bit_cast(float, k.flags)};
}
__device__ __forceinline__ void pin_consts(const SecConsts &c)
{
    asm volatile("" ::"s"(c.pc0), "s"(c.pc1), "s"(c.mb0), "s"(c.mb1), "s"(c.b1), "s"(c.a1), "s"(c.a2), "s"(c.flags_bits));
}

// One cascade section, in place on the thread's two chunks.
//   zA, zB (in) : predicted end states (z1, z2) of chunk A and chunk B from zero state, pole coordinates
//   zA, zB (out): the same for the NEXT section
//   c  (in)    : this section's constants;   cn (out): the next section's, requested here
// Two loops: the recursion (3 scalar constants), then the next section's predictor over the fresh outputs (its
// 16 tap pairs and half-chunk matrix, requested before the recursion so that they arrive under it and resident in
// 36 scalar registers until the predictor is done: predict_chunk_ends).
// (-DSA_STAMP_IIR, diagnostic builds: stamps 3..8 mark the inside of section 2 instead of the FFT passes)
#ifdef SA_STAMP_IIR
#define SA_STAMP_SEC(i) do { if constexpr (SIDX == 2) SA_STAMP(i); } while (0)
#define SA_STAMP_FFT(i) do {} while (0)
#else
#define SA_STAMP_SEC(i) do {} while (0)
#define SA_STAMP_FFT(i) SA_STAMP(i)
#endif
// ScanLane: what a lane's scan reads need and every section would compute again, formed once in iir_cascade --
struct ScanLane {
    unsigned own;         // LDS address of this lane's row total in section 0's scratch (section S: + 128 S, the offset field)
    unsigned prev;        // ... of row (row - 1) & 15's total
    unsigned mine;        // ... of row (lane & 15)'s total
    unsigned lanep;       // ... of the lane's matrix P2^(lane & 15) of section 0 (section S: + 256 S)
    unsigned src;         // ds_bpermute byte index of lane (lane & 48) | ((row - 1) & 15)
    int t;                // the thread index, for the two lane predicates
};
template <bool PREDICT_NEXT, bool UNIT, int SIDX, typename SecT>
__device__ __forceinline__ void iir_section(v2f (&d)[32], const SecT &k, const SecT &knext, const SecConsts c,
                                            SecConsts &cn, const ScanLane sl, v2f &zA, v2f &zB)
{
    SA_STAMP_SEC(3);
    // state after both chunks of this thread, from zero state: T = Pc zA + zB
    v2f T = mv_s(c.pc0, c.pc1, zA, zB);
    // inclusive affine scan inside the 16-lane row; levels whose transition power has decayed below
    // float resolution are skipped (wave-uniform flags from the host)
    const int flags = __builtin_bit_cast(int, c.flags_bits);
    if (!(flags & 1)) scan_level<1>(T, k.plev[0]);
    if (!(flags & 2)) scan_level<2>(T, k.plev[1]);
    if (!(flags & 4)) scan_level<4>(T, k.plev[2]);
    if (!(flags & 8)) scan_level<8>(T, k.plev[3]);
    if ((sl.t & 15) == 15) *(__attribute__((address_space(3))) v2f *)(size_t)(sl.own + 128u * SIDX) = T;
    const v2f e = {row_shr<1>(T.x), row_shr<1>(T.y)};            // exclusive: state before this thread, row-local
    SA_STAMP_SEC(4);
    lds_barrier();
    SA_STAMP_SEC(5);
    v2f cst;
    if (flags & SA_IIR_SKIP_ROWSCAN) {
        // a row (1024 samples) outlasts the section's memory: the row starts from the previous row's total
        cst = lds_at<v2f>(sl.prev + 128u * SIDX);
    } else {
        // scan over the 16 row totals (every row of every wave repeats it: 16 lanes, 4 DPP levels)
        v2f r = lds_at<v2f>(sl.mine + 128u * SIDX);
        scan_level<1>(r, k.prow[0]);
        scan_level<2>(r, k.prow[1]);
        scan_level<4>(r, k.prow[2]);
        scan_level<8>(r, k.prow[3]);
        // state at the start of this lane's row = inclusive result of the previous row
        cst = v2f{lane_get_at(r.x, sl.src), lane_get_at(r.y, sl.src)};
    }
    if (sl.t < 16) cst = v2f{0.f, 0.f};                   // row 0
    // start state of chunk A: row-local part + P2^i * (row start state); chunk B: Pc sA + zA
    const f4v lanep = lds_at<f4v>(sl.lanep + 256u * SIDX);   // read behind this section's barrier (the copy of section 0 is then visible)
    const v2f aS = mv_v(v2f{lanep.x, lanep.y}, v2f{lanep.z, lanep.w}, cst, e);
    const v2f bS = mv_s(c.pc0, c.pc1, aS, zA);
    // pole coordinates -> DF2T states of the recursion (sa_common.hpp), re-paired as (chunk A, chunk B)
    const v2f q1 = {aS.x, bS.x}, q2 = {aS.y, bS.y};
    v2f s1 = c.mb0.x * q1 + c.mb1.x * q2, s2 = c.mb0.y * q1 + c.mb1.y * q2;
    // the next section's tap pairs: requested now, consumed after the recursion
    v2f tp[16], h0 = {0.f, 0.f}, h1 = {0.f, 0.f};
    if constexpr (PREDICT_NEXT) {
#pragma unroll
        for (int j = 0; j < 16; ++j) tp[j] = v2f{k.mnext[j][0], k.mnext[j][1]};
        h0 = v2f{k.p16next[0], k.p16next[1]};
        h1 = v2f{k.p16next[2], k.p16next[3]};
    }
    const float b0 = c.b0, b1 = c.b1, b2 = c.b2, na1 = -c.a1, na2 = -c.a2;
    SA_STAMP_SEC(6);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const v2f x = d[j];
        v2f y;
        if constexpr (UNIT) {                 // b = [1, r1, 1]: the cascade gain sits in the window table
            y = x + s1;
            s1 = na1 * y + (b1 * x + s2);
            s2 = na2 * y + x;
        } else {
            y = b0 * x + s1;
            s1 = na1 * y + (b1 * x + s2);
            s2 = na2 * y + b2 * x;
        }
        d[j] = y;
    }
    SA_STAMP_SEC(7);
    if constexpr (PREDICT_NEXT) {
        cn = load_consts(knext);
        predict_chunk_ends(tp, h0, h1, d, zA, zB);
        pin_consts(cn);
    }
    SA_STAMP_SEC(8);
}

// All NSEC sections run unconditionally (the host pads shorter cascades with identity sections,
// which are exact: y = 1*x + 0).  A run-time section count would carry the 64 data registers
// through control-flow merges and cost ~190 register copies.
template <int S, int NSEC, bool UNIT, typename PlanT>
__device__ __forceinline__ void iir_sections(v2f (&d)[32], const PlanT &ka, const SaIirLaneTab *__restrict__ lt,
                                             const ScanLane sl, v2f &zA, v2f &zB, const SecConsts c)
{
    if constexpr (S < NSEC) {
        // the per-lane matrices sit in LDS (iir_cascade copies them once): a 64-bit global address per thread held through
        // the whole cascade was among the values the tightest variants spilled
        SecConsts cn = c;
        iir_section<(S + 1 < NSEC), UNIT, S>(d, ka.sec[S], ka.sec[S + 1 < NSEC ? S + 1 : S], c, cn, sl, zA, zB);
        iir_sections<S + 1, NSEC, UNIT>(d, ka, lt, sl, zA, zB, cn);
    }
}

template <int NSEC, bool UNIT, typename PlanT>
__device__ __forceinline__ void iir_cascade(v2f (&d)[32], const PlanT &ka, const SaIirLaneTab *__restrict__ lt,
                                            float2 *scr, int t)
{
    // the per-lane matrices P2^i of all sections into LDS (96 x 16 bytes; read behind each section's scan barrier)
    if (t < 16 * NSEC)
        reinterpret_cast<float4 *>(reinterpret_cast<unsigned char *>(scr) + (kLaneOff - kScrOff))[t] =
            *at_bytes(reinterpret_cast<const float4 *>(&lt->p[0][0][0]), 16u * (unsigned)t);
    // predictor for the first section (later ones run after the previous section's recursion)
    const SecConsts c0 = load_consts(ka.sec[0]);
    v2f tp[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) tp[j] = v2f{ka.m0[j][0], ka.m0[j][1]};
    v2f zA, zB;
    predict_chunk_ends(tp, v2f{ka.p16_0[0], ka.p16_0[1]}, v2f{ka.p16_0[2], ka.p16_0[3]}, d, zA, zB);
    pin_consts(c0);
    // the scan's lane addresses, once for all sections and opaque: left visible, every section forms them again (about
    // ten integer instructions each) where it cannot spare the three registers
    // (and from an opaque copy of the thread index, or the frame's other uses of lane & 15 and t >> 4 keep theirs beside these)
    unsigned tc = (unsigned)t;
    asm volatile("" : "+v"(tc));
    const unsigned prow = ((tc >> 4) - 1u) & 15u, lo = tc & 15u, sb = lds_addr(scr);
    ScanLane sl = {sb + 8u * (tc >> 4), sb + 8u * prow, sb + 8u * lo, sb + (unsigned)(kLaneOff - kScrOff) + 16u * lo,
                   4u * ((tc & 48u) | prow), (int)tc};
    asm volatile("" : "+v"(sl.own), "+v"(sl.prev), "+v"(sl.mine), "+v"(sl.lanep), "+v"(sl.src));
    iir_sections<0, NSEC, UNIT>(d, ka, lt, sl, zA, zB, c0);
}

// Half-spectrum outputs (SA_OUT_MAG_HALF, SA_OUT_SPEC_HALF: the numpy.fft.rfft layout, rows of 8193 elements).  A row is
// 4- or 8-byte aligned only (every other row of complex values starts 8 bytes off a 16-byte boundary), so 16-byte stores
// straight from the registers are not possible and element-wise stores put two half-written lines into every wave
// instruction: round 2 measured twice the L2 write requests and +46 % HBM write bytes against the full-magnitude output.
// Here the 2048 consecutive bins a round produces per segment go through LDS in natural order and leave as 16-byte stores
// at ABSOLUTE 16-byte boundaries, 1 KiB contiguous per wave instruction; only the (at most n - 1) elements in front of the
// first and behind the last boundary of the segment are stored one by one.
//   seg: the segment's 2048 elements in LDS;  g: where its first element goes in the output row
template <typename Et>
__device__ __forceinline__ void stream_out_segment(const Et *__restrict__ seg, Et *__restrict__ g, int t)
{
    constexpr int n = 16 / (int)sizeof(Et);                         // elements per 16-byte unit
    const int h = (int)(((size_t)g / sizeof(Et)) & (size_t)(n - 1)); // unit u holds elements n u - h .. n u - h + n - 1
    constexpr int per_thread = 2048 / n / kThreads;
#pragma unroll
    for (int i = 0; i <= per_thread; ++i) {
        const int u = t + kThreads * i;
        if (i == per_thread && (h == 0 || t != 0)) break;           // the unit behind the last full one: thread 0, if any
        const int e0 = n * u - h;
        if (e0 >= 0 && e0 + n <= 2048) {
            float v[4];
            if constexpr (n == 2) {
                const float2 a = reinterpret_cast<const float2 *>(seg)[e0], b = reinterpret_cast<const float2 *>(seg)[e0 + 1];
                v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = reinterpret_cast<const float *>(seg)[e0 + j];
            }
            store_nt(reinterpret_cast<float *>(g + e0), v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < n; ++j)
                if (e0 + j >= 0 && e0 + j < 2048) {
                    if constexpr (n == 2) {
                        const float2 a = reinterpret_cast<const float2 *>(seg)[e0 + j];
                        store_nt(reinterpret_cast<float2 *>(g + e0 + j), a.x, a.y);
                    } else {
                        store_nt(reinterpret_cast<float *>(g + e0 + j), reinterpret_cast<const float *>(seg)[e0 + j]);
                    }
                }
        }
    }
}

// Position of Z[k] inside the half image of the natural-order exchange.  Round r holds the rows
// d = k >> 9 of {0..3, 12..15} (r = 0) or {4..11} (r = 1), compacted to d' = (d + 4r) & 7; inside a row
// the 512 entries are padded by one per 32.  With q = k - 2048 r for the low member of a pair and
// w = 2048 - q for its partner 8192 - k, the compacted row is the same expression in both rounds:
//   low  member: row = q >> 9            partner: row = (4 + (w >> 9)) & 7
__device__ __forceinline__ int zrow_pos(int within, int row)
{
    const int rest = within & 511;
    return rest + (rest >> 5) + 528 * row;
}
__device__ __forceinline__ int zpos_low(int q) { return zrow_pos(q, q >> 9); }
__device__ __forceinline__ int zpos_partner(int w) { return zrow_pos(w, (4 + (w >> 9)) & 7); }

// The ten reads of one split-step group and their wait, written out as single 8-byte reads with 16-bit offsets: left to the
// compiler they pair up (ds_read2_b64), whose offsets reach 2040 bytes only, and every pair two rows away from its position
// gets a base of its own.  Low members zk[e] at za + UP + 8 e (e < 4) and zb + ZB_OFF; partners zm[0] at zm0 + ZM0_OFF and
// zm[e] at zm4 + DN + 8 (4 - e).
// (!WRITTEN_OUT: the same reads left to the compiler.)
template <bool WRITTEN_OUT, int UP, int ZB_OFF, int ZM0_OFF, int DN>
__device__ __forceinline__ void split_reads(unsigned za, unsigned zb, unsigned zm0, unsigned zm4, cf (&zk)[5], cf (&zm)[5])
{
    if constexpr (!WRITTEN_OUT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) zk[e] = lds_at<cf>(za + UP + 8 * e);
        zk[4] = lds_at<cf>(zb + ZB_OFF);
        zm[0] = lds_at<cf>(zm0 + ZM0_OFF);
#pragma unroll
        for (int e = 1; e < 5; ++e) zm[e] = lds_at<cf>(zm4 + DN + 8 * (4 - e));
        return;
    }
    asm volatile("ds_read_b64 %0, %10 offset:%14\n\t"
                 "ds_read_b64 %5, %12 offset:%16\n\t"
                 "ds_read_b64 %1, %10 offset:%14+8\n\t"
                 "ds_read_b64 %6, %13 offset:%17+24\n\t"
                 "ds_read_b64 %2, %10 offset:%14+16\n\t"
                 "ds_read_b64 %7, %13 offset:%17+16\n\t"
                 "ds_read_b64 %3, %10 offset:%14+24\n\t"
                 "ds_read_b64 %8, %13 offset:%17+8\n\t"
                 "ds_read_b64 %4, %11 offset:%15\n\t"
                 "ds_read_b64 %9, %13 offset:%17\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(zk[0]), "=&v"(zk[1]), "=&v"(zk[2]), "=&v"(zk[3]), "=&v"(zk[4]), "=&v"(zm[0]), "=&v"(zm[1]), "=&v"(zm[2]),
                   "=&v"(zm[3]), "=&v"(zm[4])
                 : "v"(za), "v"(zb), "v"(zm0), "v"(zm4), "n"(UP), "n"(ZB_OFF), "n"(ZM0_OFF), "n"(DN)
                 : "memory");
}

// ---------------------------------------------------------------------------------------------
// One frame: window -> IIR -> FFT -> split -> store.
// ONE_ROUND (bypassed chain on float32 frames, small batches only: sa_launch_chain_f32): the whole 64 KiB frame is
// requested at once into a 64 KiB LDS image instead of two half-frame rounds -- one HBM round trip and one barrier
// fewer per frame, at two workgroups per CU instead of four, which costs nothing while the batch leaves the CUs
// half empty anyway (B <= 512: at most two workgroups per CU either way).
// mlo, mhi: the marker range [mlo, mhi) of full-spectrum bins; read by the SA_OUT_MARKER instantiations only.
template <int NSEC, bool UNIT, int OUT, bool WINGEN, bool ONE_ROUND, typename InT, typename PlanT>
__device__ __forceinline__ void chain_frame(const InT *__restrict__ in, const float in_scale, void *__restrict__ out,
                                            const int f, unsigned char *smem,
                                            const float4 *__restrict__ winb, const float4 *__restrict__ twT,
                                            const float4 *__restrict__ twB, const float2 *__restrict__ twC,
                                            const SaIirLaneTab *__restrict__ lanetab, const PlanT &ka,
                                            const int mlo = 0, const int mhi = 0)
{
    cf *ldc = reinterpret_cast<cf *>(smem);
    float2 *scr = reinterpret_cast<float2 *>(smem + kScrOff);
    cf *side = reinterpret_cast<cf *>(smem + kSideOff);

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int lo = lane & 15;          // b in pass B, c in pass C
    const int kq = lane >> 4;
    const InT *xin = in + (size_t)f * kFrameElems<InT>;
    constexpr bool IIR = NSEC > 0;
    cf a[32];
#ifdef SA_STAMPS
    if (threadIdx.x == 0 && g_sa_stamps) g_sa_stamps[(size_t)f * 16 + 13] = __builtin_amdgcn_s_memrealtime();
#endif
    SA_STAMP(0);
    // The pass-B twiddles depend on lane & 15 alone: 2 KiB, which every thread used to read as eight 16-byte loads per frame
    // (32 KiB through L1).  Threads 0..127 request one quad each in front of the frame and park it in LDS (park_twb) where
    // the stage-in waits for the frame anyway; pass B reads them as 16-byte LDS reads, behind the barriers of the exchange
    // into pass B.  Every word of the table is written before it is read.
    float4 *twb_lds = reinterpret_cast<float4 *>(smem + (ONE_ROUND ? kOneRoundImage : kTwbOff));
    float4 twb_mine = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < kTwbBytes / 16) twb_mine = twB[t];
    const auto park_twb = [&] {
        if (t < kTwbBytes / 16) twb_lds[t] = twb_mine;
    };

    if constexpr (IIR) {
        v2f d[32];
        stage_in_chunks<WINGEN>(xin, in_scale, reinterpret_cast<const float4 *>(lanetab->win_t), lanetab, smem, t, d);
        park_twb();
        SA_STAMP(1);
        iir_cascade<NSEC, UNIT>(d, ka, lanetab, scr, t);
        SA_STAMP(2);
        // exchange to the pass-A layout in two rounds (m1 < 16, m1 >= 16): the owners of the half
        // write z[32 t' + j] = (x[2j], x[2j+1]) at 33 t' + j; everybody reads z[256 m1 + t].  Real and
        // imaginary part (even / odd sample) sit in different register pairs of d[], so each complex value is
        // stored as two dwords at adjacent addresses (one ds_write2_b32, no register copies); the reader then
        // gets an aligned (re, im) pair per 8-byte read: half the LDS read instructions of two float planes.
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            lds_barrier();
            if ((t >> 7) == h) {
                // written out: left to itself the compiler merges the two dword stores into one 64-bit store and
                // copies the two halves into a register pair first (128 v_mov per thread)
                const unsigned zw = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)(smem) +
                                    8u * 33u * (unsigned)(t & 127);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(zw), "v"(d[2 * j].x), "v"(d[2 * j + 1].x),
                                 "i"(2 * j), "i"(2 * j + 1) : "memory");
                    asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(zw), "v"(d[2 * j].y), "v"(d[2 * j + 1].y),
                                 "i"(2 * (16 + j)), "i"(2 * (16 + j) + 1) : "memory");
                }
            }
            lds_barrier();
#pragma unroll
            for (int m = 0; m < 16; ++m) a[safft::brev(16 * h + m, 5)] = ldc[264 * m + 33 * (t >> 5) + (t & 31)];
        }
    } else if constexpr (!std::is_same_v<InT, float>) {
        // No IIR, integer samples (int16 or packed 12-bit): as float32 frames do (below), but the whole frame (32 KiB or
        // 24 KiB) comes in one round of 1 KiB requests, natural order, and the form's reader (chain_f32_dev.hpp:
        // image_dword, point_of) gives z[256 m1 + t] = (x[2 i], x[2 i + 1])
        static_assert(!ONE_ROUND, "the one-round form is float32 only");
        constexpr int kUnit = 16 / (int)sizeof(InT);                            // elements of InT per 16-byte lane request
        constexpr int kSlabs = kFrameElems<InT> / (64 * kUnit) / (kThreads / 64);   // per wave: 8 (int16) or 6 (packed)
        static_assert(kSlabs * (kThreads / 64) * 1024 == kFrameElems<InT> * (int)sizeof(InT), "the requests cover the frame exactly");
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int i = 0; i < kSlabs; ++i) {
            const int n = wave * kSlabs + i;
            const InT *src = at_bytes(xin + (uniform_wave(wave) * kSlabs + i) * (64 * kUnit), 16u * (unsigned)lane);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(smem + n * 1024), 16, 0, SA_DMA_AUX);
        }
        __builtin_amdgcn_s_setprio(0);
        park_twb();               // requested ahead of the frame: arrives first, and the barrier orders the write too
        __syncthreads();
#pragma unroll
        for (int pp = 0; pp < 16; ++pp) {
            const float4 w = winb[pp * 256 + t];
            const unsigned u0 = image_dword(xin, smem, t, 2 * pp), u1 = image_dword(xin, smem, t, 2 * pp + 1);
            const cf z0 = point_of(xin, u0) * cf{in_scale, in_scale}, z1 = point_of(xin, u1) * cf{in_scale, in_scale};
            a[safft::brev(2 * pp, 5)] = {z0.x * w.x, z0.y * w.y};
            a[safft::brev(2 * pp + 1, 5)] = {z1.x * w.z, z1.y * w.w};
        }
    } else {
        // No IIR: the frame goes HBM -> LDS in natural order (two rounds of 32 KiB, LDS-DMA), and the
        // thread picks z[256 m1 + t] straight out of the image; the window comes as 16-byte loads of
        // the pass-A layout (winb[p][t] = window at samples 512(2p)+2t, +1, 512(2p+1)+2t, +1).
        // 8 + 8 vector-memory instructions per wave and round instead of 32 8-byte loads.
        constexpr int kRounds = ONE_ROUND ? 1 : 2;
        constexpr int kSlabs = 32 / kRounds / 2;           // 1 KiB DMA requests per wave and round: 8 (two rounds) or 16
        constexpr int kPairs = 16 / kRounds;               // window quads (two complex points each) per thread and round
#pragma unroll
        for (int h = 0; h < kRounds; ++h) {
            if (h == 1) __syncthreads();
            __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int i = 0; i < kSlabs; ++i) {
                const int n = wave * kSlabs + i;
                const float *src = at_bytes(xin + h * 8192 + (uniform_wave(wave) * kSlabs + i) * 256, 16u * (unsigned)lane);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(smem + n * 1024), 16, 0, SA_DMA_AUX);
            }
            __builtin_amdgcn_s_setprio(0);
            if (h == 0) park_twb();   // requested ahead of the frame: arrives first, and the barrier orders the write too
            __syncthreads();          // (the round's window values requested in front of this barrier: 2 % slower, round 4)
#pragma unroll
            for (int pp = 0; pp < kPairs; ++pp) {
                const float4 w = winb[(kPairs * h + pp) * 256 + t];
                const cf z0 = ldc[256 * (2 * pp) + t];
                const cf z1 = ldc[256 * (2 * pp + 1) + t];
                a[safft::brev(2 * kPairs * h + 2 * pp, 5)] = {z0.x * w.x, z0.y * w.y};
                a[safft::brev(2 * kPairs * h + 2 * pp + 1, 5)] = {z1.x * w.z, z1.y * w.w};
            }
        }
    }

    // ---- pass A: 32-point FFT over m1 (stride 256), then twiddle W_8192^(k1*m2), m2 = t
    SA_STAMP_FFT(3);
    // the thread's twiddle anchors (requested before the butterflies, consumed after them): W^(b t) for
    // b = 1..7 and W^(8 a t) for a = 1..3 with W = W_8192, plus W_16384^(4 t) for the split step.  The 31
    // factors W^(k1 t), k1 = 8a + b, are applied as two complex products per point; the 64 KiB table of all
    // of them (one 16-byte load per two points, every frame, through L2 -> L1) is what this replaces:
    // 24 KiB of anchors per frame, and the loads no longer sit between the butterflies and the exchange.
    float4 an[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) an[i] = *at_bytes(twT + i * 256, 16u * (unsigned)t);
    // The split-step anchors W_16384^(4 t), W_16384^(4 (t + 1)) ride along for the full-spectrum output (round 4: requested
    // right before the split step their L2 round trip was exposed once per frame -- 103.8 -> 97.0 us on the bypassed chain
    // at B = 4096, 11.5 -> 10.8 us at B = 256, -1 % with the cascade, gpurun_out/ab_an5.txt).  The half-spectrum variants
    // keep the late request: four more registers through three FFT passes make them spill.  The marker, whose epilogue
    // holds no staging registers either, takes the early one.
    constexpr bool AN5_EARLY = OUT == SA_OUT_MAG_FULL || OUT == SA_OUT_MARKER;
    float4 an5_early = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (AN5_EARLY) an5_early = *at_bytes(twT + 5 * 256, 16u * (unsigned)t);
    safft::fft_dit<32>(a);
    {
        const cf wb[8] = {{1.f, 0.f}, {an[0].x, an[0].y}, {an[0].z, an[0].w}, {an[1].x, an[1].y},
                          {an[1].z, an[1].w}, {an[2].x, an[2].y}, {an[2].z, an[2].w}, {an[3].x, an[3].y}};
        const cf wa[4] = {{1.f, 0.f}, {an[3].z, an[3].w}, {an[4].x, an[4].y}, {an[4].z, an[4].w}};
#pragma unroll
        for (int k1 = 1; k1 < 32; ++k1) {
            if ((k1 & 7) != 0) a[k1] = safft::cmul(a[k1], wb[k1 & 7]);
            if ((k1 >> 3) != 0) a[k1] = safft::cmul(a[k1], wa[k1 >> 3]);
        }
    }
    SA_STAMP_FFT(4);
    // ---- exchange A -> B in two rounds of 16 rows; FFT q of a thread lives in round q:
    //      k1 = 16q + 4 wave + kq, b = lo; inputs ldc[row][16 a + b] with row pitch 272
    cf p[2][16];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        lds_barrier();                                   // previous image fully consumed
#pragma unroll
        for (int r = 0; r < 16; ++r) ldc[r * 272 + t] = a[16 * q + r];
        lds_barrier();
        const int row = 4 * wave + kq;
#pragma unroll
        for (int aa = 0; aa < 16; ++aa) p[q][safft::brev(aa, 4)] = ldc[row * 272 + 16 * aa + lo];
    }
    SA_STAMP_FFT(5);
    // ---- pass B: 16-point FFT over a, twiddle W_256^(b*c)
    safft::fft_dit<16>(p[0]);
    safft::fft_dit<16>(p[1]);
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {                       // twB4[pp][b] = (W_256^(2pp * b), W_256^((2pp+1) * b))
        const float4 w = twb_lds[pp * 16 + lo];
        if (pp > 0) {
            p[0][2 * pp] = safft::cmul(p[0][2 * pp], {w.x, w.y});
            p[1][2 * pp] = safft::cmul(p[1][2 * pp], {w.x, w.y});
        }
        p[0][2 * pp + 1] = safft::cmul(p[0][2 * pp + 1], {w.z, w.w});
        p[1][2 * pp + 1] = safft::cmul(p[1][2 * pp + 1], {w.z, w.w});
    }
    SA_STAMP_FFT(6);
    // ---- exchange B -> C: a 16x16 transpose inside each 16-lane group, through the row this group
    //      just read (pitch 17).  Only these 16 lanes touch the row: no workgroup barrier; the LDS
    //      executes a wave's accesses in order.
    {
        const int base = (4 * wave + kq) * 272;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int c = 0; c < 16; ++c) ldc[base + c * 17 + lo] = p[q][c];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int b = 0; b < 16; ++b) p[q][safft::brev(b, 4)] = ldc[base + lo * 17 + b];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    SA_STAMP_FFT(7);
    // ---- pass C: 16-point FFT over b -> d;  Z[k1 + 32c + 512d], k1 = 16q + 4 wave + kq, c = lo
    safft::fft_dit<16>(p[0]);
    safft::fft_dit<16>(p[1]);
    SA_STAMP_FFT(8);
    // split-step anchors: W_16384^(4 t) and the right-hand neighbour's W_16384^(4 (t + 1)), (1, 0) for t = 255 (its
    // neighbour is thread 0 of the next block of 1024 bins, whose anchor is W^0).  Half-spectrum outputs request them
    // here, through an opaque copy of the thread index (see an5_early above).
    int ts = t;
    asm volatile("" : "+v"(ts));
    float4 an5 = an5_early;
    if constexpr (!AN5_EARLY) an5 = *at_bytes(twT + 5 * 256, 16u * (unsigned)ts);
    const cf wP = {an5.x, an5.y}, wPn = {an5.z, an5.w};
    MarkerAcc mk = {-1.f, SA_NPTS, 0.f};                   // SA_OUT_MARKER: this thread's part of the record
    // The split step's read positions, as LDS byte addresses, the same in both rounds.  A group of four bins never straddles
    // a padding or row boundary, so four positions serve the ten reads of a group: low members q0 + e at za + 8 e (e < 4)
    // and zb; partners at zm0, zm4 + 24, zm4 + 16, zm4 + 8, zm4.  Group jj = 1 (q0 = 4 t + 1024) lies two image rows
    // (kTwoRows bytes) above group jj = 0 for the low members and two rows below it for the partners, so each position is
    // evaluated for the lower of the two groups and the other group's is its reads' offset field.
    // Three reads leave that pattern, and each takes its address by a select here instead of its value by two selects in
    // every round (and the side slots are read by the lanes that need them only):
    //   t = 0, jj = 0: the partner of bin 2048 r is Z[8192] = Z[0], the image's first entry, in round 0 and Z[6144], not
    //                  in round 1's image, in round 1 (side slot 0); the pattern's address is one row past the image
    //   t = 255, jj = 1, round 0: bin 2048 is not in round 0's image (side slot 1).  Its partner Z[6144] is: the image
    //                  holds the value that side slot 0 holds, at the pattern's address
    constexpr int kTwoRows = 8 * 2 * 528;
    // The 8-byte accesses of the natural-order image are written out one by one (below, split_reads) except in the one-round
    // kernels: those sit at 127-128 registers, and with all ten reads of a group behind one wait the marker form spills one.
    constexpr bool kWrittenOut = !ONE_ROUND;
    const unsigned img = lds_addr(smem);
    const unsigned za = img + 8u * (unsigned)zpos_low(4 * t), zb = img + 8u * (unsigned)zpos_low(4 * t + 4);
    const unsigned zm0 = img + 8u * (unsigned)zpos_partner(1024 - 4 * t), zm4 = img + 8u * (unsigned)zpos_partner(1020 - 4 * t);
    const unsigned zm0_r0 = t == 0 ? img : zm0 + kTwoRows, zm0_r1 = t == 0 ? img + (unsigned)kSideOff : zm0 + kTwoRows;
    const unsigned zb_r0 = t == 255 ? img + (unsigned)kSideOff + 8u : zb + kTwoRows;
    // ---- natural-order image + split step, two rounds: round 0 = d in {0..3,12..15} (bins k < 2048
    //      and their partners), round 1 = d in {4..11}.  Z[2048] and Z[6144] sit on the seam and
    //      travel through two side slots.
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        lds_barrier();
        // Z[k1 + 32 c + 512 d] at k1 + 33 c + 528 d', k1 = 16 q + 4 wave + kq: one address per thread, q and the row in the
        // offset field.  Written out: the compiler pairs the 8-byte stores (ds_write2_b64), whose offsets reach 2040 bytes,
        // and adds a base per row.  (kWrittenOut: not in the one-round kernels, see there)
        {
            const unsigned zw = img + 8u * (unsigned)(4 * wave + kq + 33 * lo);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int dd = 0; dd < 8; ++dd) {
                    const int dsel = (r == 0) ? (dd < 4 ? dd : dd + 8) : dd + 4;
                    if constexpr (kWrittenOut)
                        asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(zw), "v"(p[q][dsel]), "n"(8 * (16 * q + 528 * dd)) : "memory");
                    else
                        ldc[16 * q + 4 * wave + kq + 33 * lo + 528 * dd] = p[q][dsel];
                }
            }
        }
        if (r == 0 && t == 0) {                               // k1 = 0, c = 0: d = 12 and d = 4
            side[0] = p[0][12];
            side[1] = p[0][4];
        }
        lds_barrier();
        SA_STAMP(9 + r);
        constexpr bool HALF = OUT == SA_OUT_MAG_HALF || OUT == SA_OUT_SPEC_HALF;
        cf Rs[2][5], Is[2][5];                                 // half-spectrum outputs: both groups wait for the staging pass
        float mps[2][5], mqs[2][5];                            // (magnitudes only for SA_OUT_MAG_HALF: half the registers)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            // (half-spectrum outputs keep both groups' results until the staging pass: the groups must not be interleaved)
            if (HALF && jj == 1) __builtin_amdgcn_sched_barrier(0);
            const int q0 = 4 * (t + 256 * jj);                 // k0 - 2048 r: bins q0 .. q0+4 of this round
            const int k0 = q0 + 2048 * r;
            // W_16384^(k0 + e) = W^(4 t) * W^(2048 r + 1024 jj + e): the second factor is the same for every
            // thread (twC, scalar loads), the first is the thread's anchor -- no per-bin table
            cf w[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = cmul_s(wP, twC[(2 * r + jj) * 5 + e]);
            // bin k0 + 4 is bin 0 of the neighbouring group, which also stores it: the mirrored halves of the
            // spectrum stay bit-identical only if both evaluate the same product, so this is the NEIGHBOUR's
            // twiddle for its e = 0, anchor(t + 1) * C[block][0], with the block advancing at t = 255
            {
                const float2 c0 = twC[(2 * r + jj) * 5], c1 = twC[(2 * r + jj + 1) * 5];
                const cf csel = (t == 255) ? cf{c1.x, c1.y} : cf{c0.x, c0.y};
                w[4] = safft::cmul(wPn, csel);
            }
            // the ten reads (positions and the seam pair (2048, 6144): above the rounds)
            cf zk[5], zm[5];
            if (jj == 1 && r == 0)
                split_reads<kWrittenOut, kTwoRows, 0, 0, 0>(za, zb_r0, zm0, zm4, zk, zm);
            else if (jj == 1)
                split_reads<kWrittenOut, kTwoRows, kTwoRows, 0, 0>(za, zb, zm0, zm4, zk, zm);
            else
                split_reads<kWrittenOut, 0, 0, 0, kTwoRows>(za, zb, r == 0 ? zm0_r0 : zm0_r1, zm4, zk, zm);
            cf R[5], I[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) split_eval(zk[e], zm[e], w[e], R[e], I[e]);
            if constexpr (OUT == SA_OUT_MARKER) {
                marker_group(R, I, k0, __builtin_amdgcn_readfirstlane(k0), mlo, mhi, mk);     // lane 0: the wave's first group
            } else if constexpr (!HALF) {
                split_store<OUT>(R, I, out, f, k0, t);
            } else if constexpr (OUT == SA_OUT_SPEC_HALF) {
#pragma unroll
                for (int e = 0; e < 5; ++e) {
                    Rs[jj][e] = R[e];
                    Is[jj][e] = I[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 5; ++e) {
                    const cf m2 = safft::pk_fma(I[e], I[e], R[e] * R[e]);          // (|P|^2, |Q|^2)
                    mps[jj][e] = fast_sqrt(m2.x);
                    mqs[jj][e] = fast_sqrt(m2.y);
                }
            }
        }
        if constexpr (HALF) {
            // stage the round's two runs of 2048 bins in natural order (stream_out_segment):
            //   segment 0 = bins 2048 r .. 2048 r + 2047           P_e = X[k0 + e], e < 4, at q0 + e
            //   segment 1 = bins 6144 - 2048 r .. 8191 - 2048 r    conj Q_e = X[8192 - k0 - e], e = 1..4, at 2048 - q0 - e
            lds_barrier();                                     // every thread is done with the Z image
            if constexpr (OUT == SA_OUT_SPEC_HALF) {
                float4 *s0 = reinterpret_cast<float4 *>(smem), *s1 = reinterpret_cast<float4 *>(smem + 2048 * 8);
                float2 *orow = reinterpret_cast<float2 *>(out) + (size_t)f * (SA_MC + 1);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int q0 = 4 * (t + 256 * jj);
                    const cf(&R)[5] = Rs[jj];
                    const cf(&I)[5] = Is[jj];
                    s0[q0 / 2] = make_float4(R[0].x, I[0].x, R[1].x, I[1].x);
                    s0[q0 / 2 + 1] = make_float4(R[2].x, I[2].x, R[3].x, I[3].x);
                    s1[(2044 - q0) / 2] = make_float4(R[4].y, -I[4].y, R[3].y, -I[3].y);
                    s1[(2044 - q0) / 2 + 1] = make_float4(R[2].y, -I[2].y, R[1].y, -I[1].y);
                    if (r == 0 && q0 == 0) store_nt(orow + SA_MC, R[0].y, -I[0].y);          // X[8192]
                }
                lds_barrier();
                stream_out_segment(reinterpret_cast<const float2 *>(smem), orow + 2048 * r, t);
                stream_out_segment(reinterpret_cast<const float2 *>(smem + 2048 * 8), orow + 6144 - 2048 * r, t);
            } else {
                float4 *s0 = reinterpret_cast<float4 *>(smem), *s1 = reinterpret_cast<float4 *>(smem + 2048 * 4);
                float *orow = reinterpret_cast<float *>(out) + (size_t)f * (SA_MC + 1);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int q0 = 4 * (t + 256 * jj);
                    const float(&mp)[5] = mps[jj];
                    const float(&mq)[5] = mqs[jj];
                    s0[q0 / 4] = make_float4(mp[0], mp[1], mp[2], mp[3]);
                    s1[(2044 - q0) / 4] = make_float4(mq[4], mq[3], mq[2], mq[1]);
                    if (r == 0 && q0 == 0) store_nt(orow + SA_MC, mq[0]);
                }
                lds_barrier();
                stream_out_segment(reinterpret_cast<const float *>(smem), orow + 2048 * r, t);
                stream_out_segment(reinterpret_cast<const float *>(smem + 2048 * 4), orow + 6144 - 2048 * r, t);
            }
        }
    }
    // the scan scratch has been idle since the cascade; the barrier inside orders the half-wave parts before thread 0
    if constexpr (OUT == SA_OUT_MARKER) marker_finish(mk, reinterpret_cast<float4 *>(scr), out, f, t);
    SA_STAMP(11);
#ifdef SA_STAMPS
    __builtin_amdgcn_s_waitcnt(0);      // drain the stores so the last stamp sees them retire
#endif
    SA_STAMP(12);
#ifdef SA_STAMPS
    if (threadIdx.x == 0 && g_sa_stamps) {             // placement and wall-clock end (100 MHz counter, the same on every XCD)
        g_sa_stamps[(size_t)f * 16 + 14] = __builtin_amdgcn_s_memrealtime();
        g_sa_stamps[(size_t)f * 16 + 15] =
            (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |
            ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);
    }
#endif
}

template <typename InT, int NSEC, bool UNIT, int OUT, bool WINGEN, bool ONE_ROUND, typename... Scale>
__global__ __launch_bounds__(kThreads, 4) void chain_f32_kernel(const InT *__restrict__ in, const Scale... in_scale,
                                                                 void *__restrict__ out, int batch,
                                                                 const float4 *__restrict__ winb,
                                                                 const float4 *__restrict__ twT,
                                                                 const float4 *__restrict__ twB,
                                                                 const float2 *__restrict__ twC,
                                                                 const SaIirLaneTab *__restrict__ lanetab,
                                                                 const SaIirK ka)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int f = blockIdx.x;
    if (f >= batch) return;
    chain_frame<NSEC, UNIT, OUT, WINGEN, ONE_ROUND>(in, in_scale_of(in_scale...), out, f, smem, winb, twT, twB, twC,
                                                     lanetab, ka);
}

// SA_OUT_MARKER: the same chain with the marker range [lo, hi) in its arguments (chain_f32_kernel keeps its own), packed
// as lo | hi << 16 into one word: one scalar register held through the kernel, not two (the six-section variants run
// out of scalar registers)
template <typename InT, int NSEC, bool UNIT, bool WINGEN, bool ONE_ROUND, typename... Scale>
__global__ __launch_bounds__(kThreads, 4) void chain_marker_kernel(const InT *__restrict__ in, const Scale... in_scale,
                                                                    void *__restrict__ out, int batch, int range,
                                                                    const float4 *__restrict__ winb,
                                                                    const float4 *__restrict__ twT,
                                                                    const float4 *__restrict__ twB,
                                                                    const float2 *__restrict__ twC,
                                                                    const SaIirLaneTab *__restrict__ lanetab,
                                                                    const SaIirK ka)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int f = blockIdx.x;
    if (f >= batch) return;
    chain_frame<NSEC, UNIT, SA_OUT_MARKER, WINGEN, ONE_ROUND>(in, in_scale_of(in_scale...), out, f, smem, winb, twT, twB,
                                                               twC, lanetab, ka, range & 0xFFFF, range >> 16);
}

// Window (+ IIR) only: the FFT input time series (debug / parity output, not a hot path: two workgroups per CU are
// asked for, so the register allocator has 256 registers and spills nothing in any instantiation).
template <typename InT, int NSEC, bool UNIT, typename... Scale>
__global__ __launch_bounds__(kThreads, 2) void time_f32_kernel(const InT *__restrict__ in, const Scale... in_scale,
                                                                float *__restrict__ out, int batch,
                                                                const float4 *__restrict__ wint_plain,
                                                                const SaIirLaneTab *__restrict__ lanetab,
                                                                const SaIirK ka)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *scr = reinterpret_cast<float2 *>(smem + kScrOff);
    const int t = threadIdx.x;
    const int f = blockIdx.x;
    if (f >= batch) return;
    v2f d[32];
    const float4 *wint = NSEC > 0 ? reinterpret_cast<const float4 *>(lanetab->win_t) : wint_plain;
    stage_in_chunks<false>(in + (size_t)f * kFrameElems<InT>, in_scale_of(in_scale...), wint, lanetab, smem, t, d);
    if constexpr (NSEC > 0) iir_cascade<NSEC, UNIT>(d, ka, lanetab, scr, t);
    // Stage-out through the row image (chain_f32_dev.hpp): round h writes the thread's chunk h into its row, then
    // store_rows.  Stored straight from the registers it measured 5x slower than the whole spectrum chain.
    float4 *lds4 = reinterpret_cast<float4 *>(smem);
    float *o = out + (size_t)f * SA_NPTS;
    const int sw = row_swizzle(t);
    int ts = t;                              // opaque copy for store_rows
    asm volatile("" : "+v"(ts));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lds_barrier();                       // scan scratch / previous round consumed
#pragma unroll
        for (int g = 0; g < 8; ++g) {        // undo the folded 1/2 (exact)
            const float4 v = h == 0 ? make_float4(2.f * d[4 * g].x, 2.f * d[4 * g + 1].x, 2.f * d[4 * g + 2].x, 2.f * d[4 * g + 3].x)
                                    : make_float4(2.f * d[4 * g].y, 2.f * d[4 * g + 1].y, 2.f * d[4 * g + 2].y, 2.f * d[4 * g + 3].y);
            lds4[t * 8 + (g ^ sw)] = v;
        }
        lds_barrier();
        store_rows(o, h, smem, ts);
    }
}

// Raise the kernel's dynamic-LDS limit (once) and launch one workgroup per frame.
template <typename K, typename... Args>
hipError_t launch(K kern, int lds_bytes, int batch, hipStream_t stream, SaLaunchEv ev, const Args &...args)
{
    const hipError_t e = sa_set_dyn_lds_once(reinterpret_cast<const void *>(kern), lds_bytes);
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(kern, dim3(batch), dim3(kThreads), lds_bytes, stream, ev.start, ev.stop, 0, args...);
    return hipGetLastError();
}

// The launchers below take the input last: `in` and, for int16 samples, its scale (in_scale: the kernels' Scale...).
//
// One spectrum output kind (SA_OUT_MARKER included).  The window generator exists only with the cascade: for NSEC = 0
// both arms of the WINGEN choice are the same kernel.
// Small batches of the bypassed chain on float32 frames (the board's power-on mode, new/command_control.vhd:31;
// BASELINE config 2 is B = 256): at most two workgroups per CU are resident whatever the kernel asks for, so the frame
// comes in as ONE 64 KiB round (chain_frame<ONE_ROUND>).  Same arithmetic, same results.
// A/B in one process (gpurun_out/ab_oneround.txt): 11.0 -> 10.8 us at B = 256, 15.5 -> 15.3 us at B = 512.
template <int NSEC, bool UNIT, int OUT, typename InT, typename... Scale>
hipError_t launch_spectrum(void *out, int batch, const SaF32Tables &tb, const SaIirK &ka, hipStream_t stream,
                           SaLaunchEv ev, const InT *in, const Scale... in_scale)
{
    constexpr bool WG = NSEC > 0, ONE_ROUND_FORM = NSEC == 0 && std::is_same_v<InT, float>;
    const bool one_round = ONE_ROUND_FORM && batch <= kOneRoundMax;
    const int lds = one_round ? kLdsOneRound : kLdsBytes;
    if constexpr (OUT == SA_OUT_MARKER) {
        auto kern = ka.wingen ? chain_marker_kernel<InT, NSEC, UNIT, WG, false, Scale...>
                              : chain_marker_kernel<InT, NSEC, UNIT, false, false, Scale...>;
        if constexpr (ONE_ROUND_FORM)
            if (one_round) kern = chain_marker_kernel<InT, 0, false, false, true>;
        return launch(kern, lds, batch, stream, ev, in, in_scale..., out, batch, tb.marker_lo | tb.marker_hi << 16,
                      tb.win_b, tb.twT, tb.twB, tb.twC, tb.lanetab, ka);
    } else {
        auto kern = ka.wingen ? chain_f32_kernel<InT, NSEC, UNIT, OUT, WG, false, Scale...>
                              : chain_f32_kernel<InT, NSEC, UNIT, OUT, false, false, Scale...>;
        if constexpr (ONE_ROUND_FORM)
            if (one_round) kern = chain_f32_kernel<InT, 0, false, OUT, false, true>;
        return launch(kern, lds, batch, stream, ev, in, in_scale..., out, batch, tb.win_b, tb.twT, tb.twB, tb.twC,
                      tb.lanetab, ka);
    }
}

template <int NSEC, bool UNIT, typename InT, typename... Scale>
hipError_t launch_nsec(void *out, int batch, int out_kind, const SaF32Tables &tb, const SaIirK &ka, hipStream_t stream,
                       SaLaunchEv ev, const InT *in, const Scale... in_scale)
{
    switch (out_kind) {
        case SA_OUT_MAG_FULL: return launch_spectrum<NSEC, UNIT, SA_OUT_MAG_FULL>(out, batch, tb, ka, stream, ev, in, in_scale...);
        case SA_OUT_MAG_HALF: return launch_spectrum<NSEC, UNIT, SA_OUT_MAG_HALF>(out, batch, tb, ka, stream, ev, in, in_scale...);
        case SA_OUT_SPEC_HALF: return launch_spectrum<NSEC, UNIT, SA_OUT_SPEC_HALF>(out, batch, tb, ka, stream, ev, in, in_scale...);
        case SA_OUT_MARKER: return launch_spectrum<NSEC, UNIT, SA_OUT_MARKER>(out, batch, tb, ka, stream, ev, in, in_scale...);
        case SA_OUT_TIME:
            return launch(time_f32_kernel<InT, NSEC, UNIT, Scale...>, kLdsBytes, batch, stream, ev, in, in_scale...,
                          static_cast<float *>(out), batch, tb.win_t, tb.lanetab, ka);
        default: return hipErrorInvalidValue;
    }
}

// The launcher behind sa_launch_chain_f32 (chain_f32.hip), sa_launch_chain_f32_i16 (chain_f32_i16.hip) and
// sa_launch_chain_f32_p12 (chain_f32_p12.hip).
// tb.iir->nsec is the PADDED section count (0, 2, 4 or 6; see build_plan in iir_plan.cpp).
template <typename InT, typename... Scale>
hipError_t launch_chain(void *out, int batch, int out_kind, const SaF32Tables &tb, hipStream_t stream, SaLaunchEv ev,
                        const InT *in, const Scale... in_scale)
{
    if (batch <= 0) return hipSuccess;
    static const SaIirK kNoIir = {};
    const int nsec = tb.iir ? tb.iir->nsec : 0;
    const SaIirK &ka = nsec > 0 ? *tb.iir : kNoIir;
    const bool unit = nsec > 0 && ka.unit != 0;
    switch (nsec) {
        case 0: return launch_nsec<0, false>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...);
        case 2: return unit ? launch_nsec<2, true>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...)
                            : launch_nsec<2, false>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...);
        case 4: return unit ? launch_nsec<4, true>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...)
                            : launch_nsec<4, false>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...);
        case 6: return unit ? launch_nsec<6, true>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...)
                            : launch_nsec<6, false>(out, batch, out_kind, tb, ka, stream, ev, in, in_scale...);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace
