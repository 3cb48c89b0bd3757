// chain_f32_dev.hpp -- device helpers of the float-path kernels (chain_f32.hpp, iir_f64.hip): LDS-only barrier, DPP row
// shifts, nontemporal stores, the row image that stages frames in and out of the IIR kernels, the split step of the
// packed real FFT, its output layouts and the marker reduction.
#pragma once
#include <type_traits>
#include "sa_common.hpp"
#include "fft_regs.hpp"
#include "p12_dev.hpp"
#include "../../include/specan.h"

using safft::cf;
typedef float v2f __attribute__((ext_vector_type(2)));

namespace {

#ifndef SA_DMA_AUX
#define SA_DMA_AUX 2          // cache policy bits of the input LDS-DMA: 2 = nontemporal (a frame is read once); 0 in A/B
                              // builds: 132.2 -> 130.3 us stream-ordered, no difference with two launches in flight
#endif

__device__ __forceinline__ float fast_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }

// Phase stamps: diagnostic build only (make stamps -> libspecan_hip_stamps.so, tools/phase_stamps.py).
// In the product build SA_STAMP expands to nothing.
#ifdef SA_STAMPS
__device__ unsigned long long *g_sa_stamps = nullptr;
#define SA_STAMP(i)                                                                        \
    do {                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        if (threadIdx.x == 0 && g_sa_stamps) {   /* never a store through a null table */  \
            unsigned long long c_;                                                         \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_)::"memory");     \
            g_sa_stamps[(size_t)blockIdx.x * 16 + (i)] = c_;                               \
        }                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    } while (0)
#else
#define SA_STAMP(i) do {} while (0)
#endif

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// counter (s_waitcnt vmcnt(0)), i.e. it waits for every outstanding global load AND store of the wave;
// the exchanges below hand data over through LDS alone, so in-flight twiddle loads and output stores
// may stay in flight across them.  (The stage-in barrier keeps __syncthreads(): the LDS-DMA completes
// on vmcnt.)
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---------------------------------------------------------------------------------------------
// Global addresses with a wave-uniform base (a frame, an output row, a table): the base stays in a scalar register pair
// and a lane contributes one unsigned 32-bit byte offset, so that the access takes the scalar-base form of global_load /
// global_store / LDS-DMA with the compile-time part as its immediate offset.  Formed as pointer + signed index the same
// address costs a 64-bit vector add (v_lshl_add_u64 or a carry pair) per access and a register pair per address held.
// `base` MUST be the same in every lane of the wave: the scalar constraint below takes one lane's value for all.
template <typename T>
__device__ __forceinline__ T *at_bytes(T *base, unsigned lane_bytes)
{
    using Byte = std::conditional_t<std::is_const_v<T>, const unsigned char, unsigned char>;
    // the base as it stands, in a scalar pair: left transparent, the compiler adds the lane's offset to the common part of
    // several bases first and every access is a 64-bit vector add again.  Two scalar adds per base instead.
    // The offset likewise as the 32-bit register it is: widened where it is computed (the compiler knows 16 t fits) it
    // reaches the access as a 64-bit pair, which the scalar-base form does not take.
    // Behind the opaque copy the pointer is global memory by this cast alone (else: flat accesses).
    asm("" : "+s"(base));
    asm("" : "+v"(lane_bytes));
    using GlobalByte = __attribute__((address_space(1))) Byte;
    return reinterpret_cast<T *>((Byte *)((GlobalByte *)reinterpret_cast<Byte *>(base) + lane_bytes));
}
// the wave index as the scalar it is (the compiler takes threadIdx.x >> 6 for a per-lane value)
__device__ __forceinline__ int uniform_wave(int wave) { return __builtin_amdgcn_readfirstlane(wave); }

// LDS positions as the 32-bit byte addresses they are.  An address computed once (lds_addr + the lane's part) and kept
// serves every access that differs from it by a compile-time constant through the access's 16-bit offset field; formed as
// pointer + index each access adds the image's base to a fresh index again.
__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)(p);
}
template <typename T>                                          // T: float or a vector of floats (cf, v2f, f4v)
__device__ __forceinline__ T lds_at(unsigned addr)
{
    return *(const __attribute__((address_space(3))) T *)(size_t)(addr);
}
typedef float f4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// DPP helpers: value of the lane `n` to the left inside the 16-lane row, 0 when there is none.
template <int N>
__device__ __forceinline__ float row_shr(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x110 + N, 0xF, 0xF, true));
}

// the value of another lane of the wave; src_bytes = 4 * that lane, as ds_bpermute takes it
__device__ __forceinline__ float lane_get_at(float v, unsigned src_bytes)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)src_bytes, __builtin_bit_cast(int, v)));
}

// Output stores are streaming: every byte is written once and not read by this launch.  Marked
// nontemporal they do not displace the window / twiddle tables (and the other workgroups' input lines)
// from L2: measured -9 % on the fused kernel and -19 % on the no-IIR kernel at B = 4096.
typedef float f4nt __attribute__((ext_vector_type(4)));
typedef float f2nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_nt(float *p, float a, float b, float c, float d)
{
    __builtin_nontemporal_store(f4nt{a, b, c, d}, reinterpret_cast<f4nt *>(p));
}
__device__ __forceinline__ void store_nt(float2 *p, float a, float b)
{
    __builtin_nontemporal_store(f2nt{a, b}, reinterpret_cast<f2nt *>(p));
}
__device__ __forceinline__ void store_nt(float *p, float a) { __builtin_nontemporal_store(a, p); }

// ---------------------------------------------------------------------------------------------
// The row image that stages a frame in and out of the IIR kernels (float and float64 state).  Thread t owns the 64
// samples [64t, 64t+64) and LDS row t (128 bytes: all 64 int16 samples, or one chunk of 32 float32 samples per round).
// Wave w moves rows 64w .. 64w+63 as eight 1 KiB slabs, one wave instruction each; the 16-byte column c of row r sits
// in slot c ^ row_swizzle(r), i.e. at 16-byte unit 8r + (c ^ row_swizzle(r)) of the image, so that a thread's
// ds_read_b128 / ds_write_b128 of its own row are conflict-free at this pitch.  The rows are wave-private: a wave waits
// for its own traffic only, no workgroup barrier.
__device__ __forceinline__ int row_swizzle(int r) { return (r >> 1) & 7; }

// Stage-in, one round: row r <- 128 bytes of the frame x by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no ds_write).
// The slab lands linearly in LDS, so the swizzle is applied to the per-lane SOURCE address.  Issued at raised priority
// so that the requests leave ahead of the other workgroups' arithmetic.
template <typename T>
__device__ __forceinline__ void dma_rows_impl(const T *x, int h, unsigned char *smem, int lane, int wave)
{
    // Slab n = 8 wave + i holds rows r = 8n + rl, rl = lane >> 3, and row_swizzle(r) = 4 (i & 1) | (rl >> 1): the lane's
    // source is  x + (512 wave + 64 i + 8 rl) row bytes + h * 32 elements + 16 ((lane & 7) ^ row_swizzle(r)), of which only
    //   v0 = rl * row bytes + 16 ((lane & 7) ^ (rl >> 1))     (even i;  odd i: v0 ^ 64)
    // differs from lane to lane (at_bytes): two registers instead of eight 64-bit addresses
    constexpr int kRow = 64 * (int)sizeof(T);
    const int rl = lane >> 3;
    const unsigned v0 = (unsigned)(rl * kRow + (((lane & 7) ^ (rl >> 1)) << 4)), v1 = v0 ^ 64u;
    const int uw = uniform_wave(wave);                         // the slabs' LDS bases are scalar adds on it, as the sources are
    const T *xw = x + uw * (64 * 64) + h * 32;
    __builtin_amdgcn_s_setprio(3);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = uw * 8 + i;                              // slab: rows 8n .. 8n+7
        const T *src = at_bytes(xw + i * (8 * 64), (i & 1) ? v1 : v0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(smem + n * 1024), 16, 0, SA_DMA_AUX);
    }
    __builtin_amdgcn_s_setprio(0);
}
// float32 frames: round h (0 or 1) brings chunk h, samples x[64r + 32h ..], of every row
__device__ __forceinline__ void dma_rows(const float *x, int h, unsigned char *smem, int lane, int wave)
{
    dma_rows_impl(x, h, smem, lane, wave);
}
// int16 samples: one round brings all 64 samples of every row
__device__ __forceinline__ void dma_rows(const int16_t *x, unsigned char *smem, int lane, int wave)
{
    dma_rows_impl(x, 0, smem, lane, wave);
}

// Packed 12-bit samples: the tag type SaP12 over the bytes and the unpack of eight samples are in p12_dev.hpp.
// elements of InT from one frame to the next
template <typename InT> constexpr int kFrameElems = SA_NPTS;
template <> constexpr int kFrameElems<SaP12> = SA_P12_FRAME_BYTES;

// The p12 row image.  A thread's 64 samples are 96 bytes: row r is the six 16-byte units 6r .. 6r+5 of the frame, and
// wave w's 64 rows are exactly six 1 KiB slabs, so ONE round of 6 requests per wave brings the frame and the rows stay
// wave-private.  At the natural place (unit u in slot u) a ds_read_b128 of column g by every thread is 2-way
// conflicted: the 16-byte slot inside the 256-byte bank row is (6r + g) mod 16, which has the parity of g and repeats
// with r + 8, and each of the instruction's four 16-lane groups ({0-3, 12-15, 20-27}, ...) holds every r mod 8 twice,
// once with bit 3 of r clear and once with it set.  So the rows with bit 3 set swap the two units of each 32-byte pair:
// unit u sits in slot u ^ ((r >> 3) & 1), r = u / 6 (6r is even, so a pair never leaves its row).  The rows with the bit
// clear then cover the eight slots of g's parity and the others the eight of the opposite parity: 16 lanes, 16 slots,
// conflict-free.  The swap is applied to the per-lane SOURCE address (the slab lands linearly in LDS); a request still
// reads 1 KiB contiguous.
__device__ __forceinline__ int p12_row_swizzle(int r) { return (r >> 3) & 1; }

__device__ __forceinline__ void dma_rows(const SaP12 *x, unsigned char *smem, int lane, int wave)
{
    const int uw = uniform_wave(wave);
    __builtin_amdgcn_s_setprio(3);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int n = uw * 6 + i;                              // slab: slots 64n .. 64n+63
        const int s = 64 * n + lane;                           // the slot this lane fills, of row s / 6
        // unit u = s ^ swizzle = 64 n + (lane ^ swizzle): the slab's KiB is wave-uniform, the lane's part 16 (lane ^ swizzle)
        const unsigned v = (unsigned)((lane ^ p12_row_swizzle(s / 6)) << 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)at_bytes(x + 1024 * (uw * 6 + i), v),
                                         (__attribute__((address_space(3))) void *)(smem + n * 1024), 16, 0, SA_DMA_AUX);
    }
    __builtin_amdgcn_s_setprio(0);
}

// The six units of row t (chunk A: 12 dwords, chunk B: 12 dwords) as six ds_read_b128 and their wait, written out as one
// statement: left to the compiler the reads of some instantiations come out as ds_read2_b64 / ds_read2_b32 pieces, which
// bank differently (modulo 32 dwords) and are not conflict-free in this image.  Unit c sits in slot 6t + (c ^ swizzle):
// the even units are read from one base address and the odd ones from another, both with immediate offsets.
typedef unsigned u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void p12_read_row(const unsigned char *smem, int t, unsigned (&ua)[12], unsigned (&ub)[12])
{
    const unsigned sw = (unsigned)p12_row_swizzle(t);
    const unsigned row = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)(smem) + 96u * (unsigned)t;
    const unsigned ae = row + 16u * sw, ao = row + 16u * (sw ^ 1u);          // units 0, 2, 4 and 1, 3, 5 at +0, +32, +64
    u4v q[6];
    asm volatile("ds_read_b128 %0, %6\n\t"
                 "ds_read_b128 %1, %7\n\t"
                 "ds_read_b128 %2, %6 offset:32\n\t"
                 "ds_read_b128 %3, %7 offset:32\n\t"
                 "ds_read_b128 %4, %6 offset:64\n\t"
                 "ds_read_b128 %5, %7 offset:64\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3]), "=&v"(q[4]), "=&v"(q[5])
                 : "v"(ae), "v"(ao)
                 : "memory");
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ua[4 * c] = q[c].x; ua[4 * c + 1] = q[c].y; ua[4 * c + 2] = q[c].z; ua[4 * c + 3] = q[c].w;
        ub[4 * c] = q[3 + c].x; ub[4 * c + 1] = q[3 + c].y; ub[4 * c + 2] = q[3 + c].z; ub[4 * c + 3] = q[3 + c].w;
    }
}

// The readers of the integer sample forms.  Behind dma_rows the two forms differ only in how a thread gets samples out of
// its row, so the stage-ins (chain_f32.hpp: stage_in_chunks, iir_f64.hip: stage_in) are written once on two overloads
// that the pointer type selects:
//   row_open: what is read once per row, in front of the steps
//   row_step: samples 8g .. 8g+7 of chunk h (0: chunk A, 1: chunk B) as ints, g = 0 .. 3
// Free functions of (smem, t) on purpose: with t and the swizzle held in a reader object the address arithmetic of the
// int16 kernels comes out differently.
//
// int16: nothing to open; column c of a row holds samples 8c .. 8c+7, c < 4 is chunk A and c >= 4 chunk B, so a step is the
// ds_read_b128 of column g + 4h and the half-word extracts.
__device__ __forceinline__ void row_open(const int16_t *, const unsigned char *, int, unsigned (&)[2][12]) {}
__device__ __forceinline__ void row_step(const int16_t *, const unsigned char *smem, int t, unsigned (&)[2][12], int h, int g,
                                         int (&s)[8])
{
    const uint4 q = reinterpret_cast<const uint4 *>(smem)[t * 8 + ((g + 4 * h) ^ row_swizzle(t))];
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = (e & 1) ? (int)u[e >> 1] >> 16 : (int)(short)(u[e >> 1] & 0xFFFFu);
}
// packed 12-bit: the whole row is read at the start (p12_read_row: units 0..2 are chunk A, 3..5 chunk B); three dwords
// hold eight samples, so step g unpacks dwords 3g .. 3g+2 of the chunk.
__device__ __forceinline__ void row_open(const SaP12 *, const unsigned char *smem, int t, unsigned (&u)[2][12])
{
    p12_read_row(smem, t, u[0], u[1]);
}
__device__ __forceinline__ void row_step(const SaP12 *, const unsigned char *, int, unsigned (&u)[2][12], int h, int g,
                                         int (&s)[8])
{
    p12_unpack8(u[h][3 * g], u[h][3 * g + 1], u[h][3 * g + 2], s);
}

// The readers of the bypassed chain's natural-order image of integer samples (chain_f32.hpp, chain_frame with NSEC = 0):
//   image_dword: the complex point z[m] = (x[2 m], x[2 m + 1]), m = 256 m1 + t, as the form packs it into a dword
//   point_of   : that dword as a pair of floats
// int16: the point is one dword of the image, two half-words
__device__ __forceinline__ unsigned image_dword(const int16_t *, const unsigned char *smem, int t, int m1)
{
    return reinterpret_cast<const unsigned *>(smem)[256 * m1 + t];
}
__device__ __forceinline__ cf point_of(const int16_t *, unsigned u)
{
    return cf{(float)(int)(short)(u & 0xFFFFu), (float)((int)u >> 16)};
}
// packed 12-bit: the point is the three bytes at byte 3 m = 768 m1 + 3 t: the two aligned dwords around them and a funnel
// shift by 8 * (3 t mod 4) bits (the same for every m1), then two sign-extending extracts.  The second dword of the
// frame's last point lies one dword behind the frame (inside the image's allocation); at that point's shift of 8 none of
// its bits reaches the 24 that are used.
__device__ __forceinline__ unsigned image_dword(const SaP12 *, const unsigned char *smem, int t, int m1)
{
    const unsigned *ldu = reinterpret_cast<const unsigned *>(smem) + ((3 * t) >> 2);
    const unsigned sh = 8u * ((3u * (unsigned)t) & 3u);
    return __builtin_amdgcn_alignbit(ldu[192 * m1 + 1], ldu[192 * m1], sh);
}
__device__ __forceinline__ cf point_of(const SaP12 *, unsigned u) { return cf{(float)p12_bfe(u, 0), (float)p12_bfe(u, 12)}; }

// Stage-out, round h, the stage-in run backwards: row r (32 float32 samples) -> o[64r + 32h ..].
// Every wave instruction picks up 1 KiB of LDS in linear order and stores it with 16 bytes per lane: stored straight
// from the registers, every lane of a store instruction would land in another 256-byte block.
// t: the thread index, passed by the kernels as an opaque copy (asm volatile).  Derived from the plain index, the row
// addresses here equal the stage-in's, and the compiler keeps those live through the whole cascade to reuse them: up to
// 40 more VGPRs in the time-series and float64-state kernels.
__device__ __forceinline__ void store_rows(float *o, int h, const unsigned char *smem, int t)
{
    const float4 *lds4 = reinterpret_cast<const float4 *>(smem);
    const int lane = t & 63, wave = t >> 6, rl = lane >> 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = wave * 8 + i;
        const int r = 8 * n + rl;
        const int lc = (lane & 7) ^ row_swizzle(r);
        const float4 v = lds4[n * 64 + lane];
        store_nt(o + r * 64 + h * 32 + lc * 4, v.x, v.y, v.z, v.w);
    }
}

// ---------------------------------------------------------------------------------------------
// a * w with w wave-uniform (an SGPR pair): two packed ops, no copy of w into VGPRs
__device__ __forceinline__ cf cmul_s(const cf a, const float2 wu)
{
    const cf w = {wu.x, wu.y};
    cf t, r;
    asm("v_pk_mul_f32 %0, %2, %3 op_sel:[0,0] op_sel_hi:[0,1]\n\t"                                        // a.x * (w.x, w.y)
        "v_pk_fma_f32 %1, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"                      // + a.y * (-w.y, w.x)
        : "=&v"(t), "=v"(r) : "v"(a), "s"(w));
    return r;
}

// Split step of the packed real FFT for the bin pair (k, 8192-k):
//   Xe = Z[k] + conj Z[M-k],  Xo = -i (Z[k] - conj Z[M-k]),  X[k] = Xe + W_N^k Xo,  X[M-k] = conj(Xe - W_N^k Xo)
// (the 1/2 of the textbook form is already in the window table).  With s = Z[k] + Z[M-k], d = Z[k] - Z[M-k]:
//   Xe = (s.x, d.y), Xo = (s.y, -d.x), T = W Xo = s.y (w.x, w.y) + d.x (w.y, -w.x)
// and the results come out transposed, R = (Re P, Re Q) = s.x + (T.x, -T.x), I = (Im P, Im Q) = d.y + (T.y, -T.y)
// with P = X[k], Q = conj X[M-k]: every operand is a broadcast / swap / negation of a register pair
// (modifiers of the packed instructions), never a pair assembled from two registers, and both squared
// magnitudes are one packed multiply-add.
__device__ __forceinline__ void split_eval(const cf zk, const cf zm, const cf w, cf &R, cf &I)
{
    const cf s = zk + zm;
    const cf d = zk - zm;
    // written out: the compiler assembles (w.y, -w.x) and (T.x, -T.x) with v_xor/v_mov pairs otherwise
    // (one asm statement: no compiler pad between the dependent instructions)
    cf u, tw;
    asm("v_pk_mul_f32 %0, %4, %6 op_sel:[1,0] op_sel_hi:[1,1]\n\t"                                          // u = s.y * w
        "v_pk_fma_f32 %1, %5, %6, %0 op_sel:[0,1,0] op_sel_hi:[0,0,1] neg_hi:[0,1,0]\n\t"                   // T = u + d.x * (w.y, -w.x)
        "v_pk_add_f32 %2, %4, %1 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]\n\t"                             // R = s.x + (T.x, -T.x)
        "v_pk_add_f32 %3, %5, %1 op_sel:[1,1] op_sel_hi:[1,1] neg_hi:[0,1]"                                  // I = d.y + (T.y, -T.y)
        : "=&v"(u), "=&v"(tw), "=&v"(R), "=v"(I) : "v"(s), "v"(d), "v"(w));
}

// Output of one group of bins k0..k0+4 (k0 = 4g).  The group evaluates five pairs so that all four
// output streams (bins k, 8192-k and their mirrors 16384-k, 8192+k) leave as aligned 16-byte stores:
//   [k0 .. k0+3] = |P0..3|        [16384-k0-4 .. ] = |P4..1|
//   [8192+k0 ..] = |Q0..3|        [8192-k0-4 ..  ] = |Q4..1|
// Every bin of the frame is written exactly once over the 1024 groups.
template <int OUT>
__device__ __forceinline__ void split_store(const cf (&R)[5], const cf (&I)[5], void *__restrict__ out, int f, int k0, int t)
{
    if constexpr (OUT == SA_OUT_MAG_FULL || OUT == SA_OUT_MAG_HALF) {
        float mp[5], mq[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const cf m2 = safft::pk_fma(I[e], I[e], R[e] * R[e]);          // (|P|^2, |Q|^2)
            mp[e] = fast_sqrt(m2.x);
            mq[e] = fast_sqrt(m2.y);
        }
        if constexpr (OUT == SA_OUT_MAG_FULL) {
            // k0 = kc + 4 t with kc the same for every thread: the row and kc make four scalar bases, and the thread adds
            // 16 t to the ascending streams and 16 (255 - t) to the descending ones (at_bytes)
            float *o = reinterpret_cast<float *>(out) + (size_t)f * SA_NPTS;
            const unsigned up = 16u * (unsigned)t, dn = 16u * (unsigned)(SA_NTHREADS - 1 - t);
            const int kc = k0 - 4 * t;
            store_nt(at_bytes(o + kc, up), mp[0], mp[1], mp[2], mp[3]);
            store_nt(at_bytes(o + (SA_NPTS - 4 * SA_NTHREADS - kc), dn), mp[4], mp[3], mp[2], mp[1]);
            store_nt(at_bytes(o + (SA_MC + kc), up), mq[0], mq[1], mq[2], mq[3]);
            store_nt(at_bytes(o + (SA_MC - 4 * SA_NTHREADS - kc), dn), mq[4], mq[3], mq[2], mq[1]);
        } else {
            float *o = reinterpret_cast<float *>(out) + (size_t)f * (SA_MC + 1);     // rows are not 16-byte aligned
#pragma unroll
            for (int e = 0; e < 4; ++e) store_nt(o + k0 + e, mp[e]);
#pragma unroll
            for (int e = 1; e < 5; ++e) store_nt(o + SA_MC - k0 - e, mq[e]);
            if (k0 == 0) store_nt(o + SA_MC, mq[0]);
        }
    } else {
        float2 *o = reinterpret_cast<float2 *>(out) + (size_t)f * (SA_MC + 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) store_nt(o + k0 + e, R[e].x, I[e].x);
#pragma unroll
        for (int e = 1; e < 5; ++e) store_nt(o + SA_MC - k0 - e, R[e].y, -I[e].y);
        if (k0 == 0) store_nt(o + SA_MC, R[0].y, -I[0].y);
    }
}

// ---------------------------------------------------------------------------------------------
// SA_OUT_MARKER: peak search and band power over the full-spectrum bins [lo, hi) of a frame, with no spectrum stored.
// A thread owns the positions split_store<SA_OUT_MAG_FULL> writes for its groups, and sees each with the value that
// call stores there: every bin of the range is counted once, with no special case for bin 0, bin 8192 or the
// duplicated e = 4 pairs.  Ties on the magnitude go to the lower bin, so the result is numpy.argmax on the MAG_FULL row.
struct MarkerAcc {
    float mag;      // largest |X[k]| seen (-1: none yet)
    int bin;        // lowest k attaining it
    float pow;      // sum of |X[k]|^2, in the thread's fixed visiting order
};

// One run of four consecutive bins s .. s+3 holding magnitudes m[0..3] and squares p[0..3], visited in ascending order:
// a strict > keeps the lowest bin of the run on a tie, and the run's winner joins the thread's pair with the full rule.
// MASK: the run may straddle [lo, hi) (a bin outside counts as magnitude -1, power 0).
template <bool MASK>
__device__ __forceinline__ void marker_run(MarkerAcc &a, const float (&m)[4], const float (&p)[4], int s, int lo, int hi)
{
    float best = -1.f, pw = 0.f;
    int be = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float mm = m[e], pe = p[e];
        if constexpr (MASK) {
            const bool in = (unsigned)(s + e - lo) < (unsigned)(hi - lo);
            mm = in ? mm : -1.f;
            pe = in ? pe : 0.f;
        }
        pw += pe;
        if (mm > best) {
            best = mm;
            be = e;
        }
    }
    a.pow += pw;
    if (best > a.mag || (best == a.mag && s + be < a.bin)) {
        a.mag = best;
        a.bin = s + be;
    }
}

// The wave's 64 runs of one kind cover the bins [w, w + 256) (w wave-uniform): one scalar decision for all of them --
// skip, take whole, or mask bin by bin where the range edge cuts through.
__device__ __forceinline__ void marker_run_any(MarkerAcc &a, const float (&m)[4], const float (&p)[4], int s, int w, int lo,
                                               int hi)
{
    if (w + 256 <= lo || w >= hi) return;
    if (w >= lo && w + 256 <= hi)
        marker_run<false>(a, m, p, s, lo, hi);
    else
        marker_run<true>(a, m, p, s, lo, hi);
}

// one group of bins k0..k0+4 (the ownership map of split_store): same squares, same square roots.
// kw: the wave-uniform k0 of the wave's lane 0 (the wave's groups of this round are k0 = kw + 4 lane)
__device__ __forceinline__ void marker_group(const cf (&R)[5], const cf (&I)[5], int k0, int kw, int lo, int hi, MarkerAcc &a)
{
    float mp[5], mq[5], pp[5], pq[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        const cf m2 = safft::pk_fma(I[e], I[e], R[e] * R[e]);          // (|P|^2, |Q|^2)
        pp[e] = m2.x;
        pq[e] = m2.y;
        mp[e] = fast_sqrt(m2.x);
        mq[e] = fast_sqrt(m2.y);
    }
    const float m0[4] = {mp[0], mp[1], mp[2], mp[3]}, p0[4] = {pp[0], pp[1], pp[2], pp[3]};
    const float m1[4] = {mp[4], mp[3], mp[2], mp[1]}, p1[4] = {pp[4], pp[3], pp[2], pp[1]};
    const float m2[4] = {mq[0], mq[1], mq[2], mq[3]}, p2[4] = {pq[0], pq[1], pq[2], pq[3]};
    const float m3[4] = {mq[4], mq[3], mq[2], mq[1]}, p3[4] = {pq[4], pq[3], pq[2], pq[1]};
    marker_run_any(a, m0, p0, k0, kw, lo, hi);                                            // [k0 ..]        P0..3
    marker_run_any(a, m1, p1, SA_NPTS - k0 - 4, SA_NPTS - kw - 256, lo, hi);              // [N-k0-4 ..]    P4..1
    marker_run_any(a, m2, p2, SA_MC + k0, SA_MC + kw, lo, hi);                            // [8192+k0 ..]   Q0..3
    marker_run_any(a, m3, p3, SA_MC - k0 - 4, SA_MC - kw - 256, lo, hi);                  // [8192-k0-4 ..] Q4..1
}

// a <- combine(a, b): the sum and the (larger magnitude, then lower bin) pair.  Symmetric in a and b, so both lanes of
// a butterfly pair end with the same bits.
__device__ __forceinline__ void marker_merge(MarkerAcc &a, const MarkerAcc &b)
{
    a.pow += b.pow;
    if (b.mag > a.mag || (b.mag == a.mag && b.bin < a.bin)) {
        a.mag = b.mag;
        a.bin = b.bin;
    }
}

template <int XOR>
__device__ __forceinline__ MarkerAcc marker_swizzle(const MarkerAcc &a)
{
    constexpr int pat = (XOR << 10) | 0x1F;                  // ds_swizzle bitmask mode: lane ^ XOR inside 32 lanes
    return {__builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, a.mag), pat)),
            __builtin_amdgcn_ds_swizzle(a.bin, pat),
            __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, a.pow), pat))};
}

// The workgroup's record: a swizzle butterfly inside each half-wave, the eight half-wave results through `scr`
// (8 x 16 bytes of LDS no other thread uses at this point), merged by thread 0 in a fixed order and stored as one
// 16-byte sa_marker.  No atomics: the bits depend on the data alone.
constexpr int kMarkerParts = SA_NTHREADS / 32;
__device__ __forceinline__ void marker_finish(MarkerAcc a, float4 *scr, void *__restrict__ out, int f, int t)
{
    marker_merge(a, marker_swizzle<1>(a));
    marker_merge(a, marker_swizzle<2>(a));
    marker_merge(a, marker_swizzle<4>(a));
    marker_merge(a, marker_swizzle<8>(a));
    marker_merge(a, marker_swizzle<16>(a));
    if ((t & 31) == 0) scr[t >> 5] = make_float4(a.mag, __builtin_bit_cast(float, a.bin), a.pow, 0.f);
    lds_barrier();
    if (t == 0) {
#pragma unroll
        for (int i = 1; i < kMarkerParts; ++i) {
            const float4 v = scr[i];
            marker_merge(a, MarkerAcc{v.x, __builtin_bit_cast(int, v.y), v.z});
        }
        store_nt(reinterpret_cast<float *>(out) + (size_t)f * 4, a.mag, __builtin_bit_cast(float, a.bin), a.pow, 0.f);
    }
}

}  // namespace
