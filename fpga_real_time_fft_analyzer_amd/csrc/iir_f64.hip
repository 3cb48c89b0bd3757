// iir_f64.hip -- window and IIR cascade of the float path with float64 state (SA_PRECISION_F64_STATE):
//     x * window  ->  up to 6 biquads (DF2T of scipy.signal.sosfilt)  ->  y rounded once to float32
// The first of the two launches of a call in that mode; the second is the bypassed float chain (chain_f32.hpp, NSEC = 0)
// on y with a constant window of 1/2 (the split step's factor, exact), so the FFT half is the proven float32 kernel.
//
// Shape (the float32 cascade's, chain_f32.hpp, in double):
//   * one 256-thread workgroup per frame; thread t owns samples [64t, 64t+64) as two independent chunks of 32 (chunk A,
//     chunk B): the recursion then has two dependency chains per thread instead of one.
//   * per section: chunk end states from zero state (predictor taps, block Horner over two half chunks), an affine scan
//     over the 512 chunks (in-row DPP shifts, one LDS hop for the 16 row totals), then the exact DF2T recursion from
//     the true start states.  The signal between sections stays in double; only the cascade output is rounded.
//   * 64 doubles of data per thread = 128 VGPRs: two workgroups per CU.
#include "chain_f32_dev.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kImgBytes = 32768;                         // stage-in / stage-out image: 256 rows of 128 bytes
constexpr int kScrOff = kImgBytes;                       // scan scratch: 6 sections x 16 rows x 2 doubles
constexpr int kLdsBytes = kScrOff + SA_MAXSEC * 16 * 16;

struct d2 {
    double x, y;
};

__device__ __forceinline__ d2 mv_add(const double (&m)[4], const d2 v, const d2 a)
{
    return {m[0] * v.x + m[1] * v.y + a.x, m[2] * v.x + m[3] * v.y + a.y};
}

// a double from the lane N to the left inside the 16-lane row (0 when there is none): two 32-bit DPP moves
template <int N>
__device__ __forceinline__ double row_shr_d(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x110 + N, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x110 + N, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double lane_get_d(double v, int src_lane)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)b);
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// z <- z + P * shifted(z): one Kogge-Stone level of the affine scan inside a row
template <int N>
__device__ __forceinline__ void scan_level(d2 &z, const double (&p)[4])
{
    const d2 u = {row_shr_d<N>(z.x), row_shr_d<N>(z.y)};
    z = mv_add(p, u, z);
}

// ---------------------------------------------------------------------------------------------
// Stage-in through the row image of the float32 cascade (chain_f32_dev.hpp): wave-private rows, no workgroup barrier.
// The window is read as 16-byte pairs of a transposed double table.
// float32 frames: two rounds, round h brings chunk h (32 samples = 128 bytes) of every thread.
__device__ __forceinline__ void stage_in(const float *__restrict__ xin, float, const double2 *__restrict__ wt,
                                         unsigned char *smem, int t, double (&d)[2][32])
{
    const float4 *lds4 = reinterpret_cast<const float4 *>(smem);
    const int lane = t & 63, wave = t >> 6, sw = row_swizzle(t);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's reads of round 0 are done
        // opaque copies per round: otherwise the row addresses of both rounds are computed and held from the start
        int l = lane, w = wave;
        asm volatile("" : "+v"(l), "+v"(w));
        dma_rows(xin, h, smem, l, w);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const float4 q = lds4[t * 8 + (g ^ sw)];
            const double2 w0 = wt[(16 * h + 2 * g) * 256 + t], w1 = wt[(16 * h + 2 * g + 1) * 256 + t];
            d[h][4 * g + 0] = (double)q.x * w0.x;
            d[h][4 * g + 1] = (double)q.y * w0.y;
            d[h][4 * g + 2] = (double)q.z * w1.x;
            d[h][4 * g + 3] = (double)q.w * w1.y;
        }
    }
}

// Integer samples (InT = int16_t or SaP12): one round brings the whole frame, and the reader of the form (chain_f32_dev.hpp:
// row_open, row_step) gives samples 8g .. 8g+7 of either chunk.  x = float(sample) * scale is rounded to float32 exactly as
// on the float32 path -- one v_mul_f32, written out so that it is never fused into the double multiply behind it -- so the
// int16 entry point and the float32 one on the converted frames agree bit for bit, and the packed one with the int16 one
// on the sign-extended samples.
template <typename InT>
__device__ __forceinline__ void stage_in(const InT *__restrict__ xin, const float in_scale, const double2 *__restrict__ wt,
                                         unsigned char *smem, int t, double (&d)[2][32])
{
    const int lane = t & 63, wave = t >> 6;
    dma_rows(xin, smem, lane, wave);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    unsigned row[2][12];                                       // packed form: the 12 dwords of either chunk
    row_open(xin, smem, t, row);
    // chunk by chunk: with both chunks of a step converted together the int16 kernels take up to 20 more VGPRs
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {                          // samples 8g .. 8g+7 of chunk h
            int s[8];
            row_step(xin, smem, t, row, h, g, s);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = 8 * g + e;                       // index inside the chunk
                float x;
                asm("v_mul_f32 %0, %1, %2" : "=v"(x) : "v"((float)s[e]), "v"(in_scale));     // one float32 rounding, never fused
                const double2 w = wt[(16 * h + (j >> 1)) * 256 + t];
                d[h][j] = (double)x * ((j & 1) ? w.y : w.x);
            }
        }
    }
}

// Chunk end state from zero state: z = A^16 (sum_{j<16} m[j] v[j]) + sum_{j<16} m[j] v[16 + j]
__device__ __forceinline__ d2 predict(const SaIirSecF64 &k, const double (&v)[32])
{
    d2 a0 = {0.0, 0.0}, a1 = {0.0, 0.0}, b0 = {0.0, 0.0}, b1 = {0.0, 0.0};     // two accumulators per half
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        a0.x += k.m[j][0] * v[j];           a0.y += k.m[j][1] * v[j];
        a1.x += k.m[j + 1][0] * v[j + 1];   a1.y += k.m[j + 1][1] * v[j + 1];
        b0.x += k.m[j][0] * v[16 + j];      b0.y += k.m[j][1] * v[16 + j];
        b1.x += k.m[j + 1][0] * v[17 + j];  b1.y += k.m[j + 1][1] * v[17 + j];
    }
    return mv_add(k.p16, d2{a0.x + a1.x, a0.y + a1.y}, d2{b0.x + b1.x, b0.y + b1.y});
}

__device__ __forceinline__ void section(double (&d)[2][32], const SaIirSecF64 &k, double2 *scr, int lane, int wave)
{
    const d2 zA = predict(k, d[0]), zB = predict(k, d[1]);
    // state after both chunks of this thread from zero state, then the inclusive scan inside the 16-lane row
    d2 T = mv_add(k.pc, zA, zB);
    scan_level<1>(T, k.plev[0]);
    scan_level<2>(T, k.plev[1]);
    scan_level<4>(T, k.plev[2]);
    scan_level<8>(T, k.plev[3]);
    const int row = 4 * wave + (lane >> 4);
    if ((lane & 15) == 15) scr[row] = make_double2(T.x, T.y);
    const d2 e = {row_shr_d<1>(T.x), row_shr_d<1>(T.y)};          // exclusive: state before this thread, row-local
    lds_barrier();
    // scan over the 16 row totals (every row of every wave repeats it), start of this lane's row = previous row's result
    const double2 tt = scr[lane & 15];
    d2 r = {tt.x, tt.y};
    scan_level<1>(r, k.prow[0]);
    scan_level<2>(r, k.prow[1]);
    scan_level<4>(r, k.prow[2]);
    scan_level<8>(r, k.prow[3]);
    const int src = (lane & 48) | ((row - 1) & 15);
    d2 cst = {lane_get_d(r.x, src), lane_get_d(r.y, src)};
    if (row == 0) cst = d2{0.0, 0.0};
    // true start states of chunk A (row-local part + A^(64 i) * row start) and chunk B
    const double *lp = k.lane[lane & 15];
    const d2 sA = {lp[0] * cst.x + lp[1] * cst.y + e.x, lp[2] * cst.x + lp[3] * cst.y + e.y};
    const d2 sB = mv_add(k.pc, sA, zA);
    // the DF2T recursion of sosfilt on both chunks, interleaved: two independent dependency chains
    const double b0 = k.c[0], b1 = k.c[1], b2 = k.c[2], a1 = k.c[3], a2 = k.c[4];
    double s1a = sA.x, s2a = sA.y, s1b = sB.x, s2b = sB.y;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const double xa = d[0][j], xb = d[1][j];
        const double ya = b0 * xa + s1a, yb = b0 * xb + s1b;
        s1a = b1 * xa + s2a - a1 * ya;
        s1b = b1 * xb + s2b - a1 * yb;
        s2a = b2 * xa - a2 * ya;
        s2b = b2 * xb - a2 * yb;
        d[0][j] = ya;
        d[1][j] = yb;
    }
}

// All NSEC sections unconditionally (the host pads with identity sections): no run-time loop over sections.
template <int NSEC, typename InT>
__global__ __launch_bounds__(kThreads, 2) void iir_f64_kernel(const InT *__restrict__ in, const float in_scale,
                                                               float *__restrict__ out, int batch,
                                                               const SaIirF64 *__restrict__ plan,
                                                               const double2 *__restrict__ wt)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[kLdsBytes];
    const int t = threadIdx.x, f = blockIdx.x;
    if (f >= batch) return;
    const int lane = t & 63, wave = t >> 6;
    double d[2][32];
    stage_in(in + (size_t)f * kFrameElems<InT>, in_scale, wt, smem, t, d);
    double2 *scr = reinterpret_cast<double2 *>(smem + kScrOff);
#pragma unroll
    for (int s = 0; s < NSEC; ++s) {
        // the sections' scan slots are separate: no barrier between the last read of one and the first write of the next
        section(d, plan->sec[s], scr + 16 * s, lane, wave);
    }
    // Stage-out through the row image, as time_f32_kernel (chain_f32.hpp) does: round h writes chunk h, rounded once to
    // float32, into the thread's row, then store_rows.  The barriers keep the rounds apart.
    float4 *lds4 = reinterpret_cast<float4 *>(smem);
    float *o = out + (size_t)f * SA_NPTS;
    const int sw = row_swizzle(t);
    int ts = t;                              // opaque copy for store_rows
    asm volatile("" : "+v"(ts));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lds_barrier();
#pragma unroll
        for (int g = 0; g < 8; ++g)
            lds4[t * 8 + (g ^ sw)] = make_float4((float)d[h][4 * g], (float)d[h][4 * g + 1], (float)d[h][4 * g + 2],
                                                 (float)d[h][4 * g + 3]);
        lds_barrier();
        store_rows(o, h, smem, ts);
    }
}

template <int NSEC, typename InT>
hipError_t launch(const InT *in, float in_scale, float *out, int batch, const SaIirF64 *plan, const double *win_tr,
                  hipStream_t stream, SaLaunchEv ev)
{
    hipExtLaunchKernelGGL(iir_f64_kernel<NSEC, InT>, dim3(batch), dim3(kThreads), 0, stream, ev.start, ev.stop, 0, in, in_scale,
                          out, batch, plan, reinterpret_cast<const double2 *>(win_tr));
    return hipGetLastError();
}

template <typename InT>
hipError_t launch_in(const InT *in, float in_scale, float *out, int batch, int nsec, const SaIirF64 *plan,
                     const double *win_tr, hipStream_t stream, SaLaunchEv ev)
{
    switch (nsec) {
        case 0: return launch<0>(in, in_scale, out, batch, plan, win_tr, stream, ev);
        case 2: return launch<2>(in, in_scale, out, batch, plan, win_tr, stream, ev);
        case 4: return launch<4>(in, in_scale, out, batch, plan, win_tr, stream, ev);
        case 6: return launch<6>(in, in_scale, out, batch, plan, win_tr, stream, ev);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t sa_launch_iir_f64(const void *in, SaInKind in_kind, float in_scale, float *out, int batch, int nsec,
                             const SaIirF64 *plan, const double *win_tr, hipStream_t stream, SaLaunchEv ev)
{
    if (batch <= 0) return hipSuccess;
    switch (in_kind) {
        case SaInKind::I16: return launch_in(static_cast<const int16_t *>(in), in_scale, out, batch, nsec, plan, win_tr, stream, ev);
        case SaInKind::P12: return launch_in(static_cast<const SaP12 *>(in), in_scale, out, batch, nsec, plan, win_tr, stream, ev);
        case SaInKind::F32: return launch_in(static_cast<const float *>(in), 1.f, out, batch, nsec, plan, win_tr, stream, ev);
    }
    return hipErrorInvalidValue;
}
