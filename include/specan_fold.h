/* specan_fold.h -- max hold and summed power of float magnitude spectra over groups of frames and buckets of bins.
 *
 * The float chain of specan.h has two outputs a display or a Welch estimate can use: the full spectrum (SA_OUT_MAG_FULL,
 * 64 KiB per frame) and one peak per frame (SA_OUT_MARKER).  This call is what lies between: it takes the float32 [B,16384]
 * magnitudes that sa_process_f32*(.., SA_OUT_MAG_FULL) or sa_process_q15_out(.., SA_Q15_OUT_MAG) wrote -- all N bins of each
 * frame as gui.py:294-305 plots them, the values gui.py:250-260 decodes -- and reduces them over groups of A = 2^a consecutive
 * frames and buckets of W = 2^k adjacent bins, as SA_Q15_TRACE_KIND, SA_Q15_TRACE_AVG_KIND and sa_spectra_q15 do for the
 * integer chain.  It is a pure function of a device tensor: no handle, no workspace, no state.  The functions are exported
 * by libspecan_fold.so, a library of its own beside libspecan_hip.so that links the HIP runtime and nothing else; no name of
 * specan.h or specan_ext.h is in it, and neither of those surfaces changes.  This header is plain C and includes specan.h
 * for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * `mag` is float32 [B,16384], `out` is sa_fold_point [B / A, 16384 / W].  a = log2a = 0..7 (A = 1..128), k = log2w = 0..6
 * (W = 1..64); (a, k) = (0, 0) would be a copy and is refused.  Record (g, j) covers the W A inputs at the bins
 * [jW, (j+1)W) of the frames gA .. gA + A - 1:
 *   - peak_mag is the input whose bit pattern with the sign bit cleared is the largest as a 32-bit unsigned integer, as that
 *     pattern.  For the non-negative finite values a chain writes it is the float maximum, bit for bit.  +inf beats every
 *     finite value; a NaN beats +inf, so a NaN among the inputs shows in the record; -0.0 reads as +0.0.  The comparison
 *     is an integer one: a denormal input is never flushed.
 *   - power is the float32 nearest (ties to even, IEEE overflow to +inf, denormal results kept) to a float64 sum S of the
 *     exact squares (double)m * (double)m -- the product of two float32 values is exact in float64, so a fused multiply-add
 *     and a multiply followed by an add give the same bits.  S is accumulated in this order and no other:
 *       1. per bin of the bucket, over the frames: c = (((+0.0 + sq(frame gA)) + sq(frame gA + 1)) + ...), ascending, one
 *          after the other;
 *       2. across the W bins, a balanced tree of adjacent pairs on the bin index: t[i] = t[2i] + t[2i+1], k levels.
 *     It is the SUM: A and W are powers of two, so the mean is power / (A W), exact on the host.
 *   - an all-zero record is (+0.0f, +0.0f).  If any input of a record is a NaN, power is some NaN (only isnan is
 *     specified); +inf without a NaN gives +inf.  A record depends on its own W A inputs alone.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_fold_mag_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of 16 workgroups per group of frames, nothing else -- it can be captured into a graph at any
 * time and may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the
 * handle's streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_fold_check() gives the same codes from the same code:
 *   1. a negative batch: SA_ESHAPE
 *   2. log2a outside 0..7, log2w outside 0..6, or both 0: SA_EINVAL, also at batch 0
 *   3. batch 0: SA_OK, whatever the pointers are
 *   4. a batch that is no multiple of A, or one whose launch would pass 2^31 - 1 workgroups (B / A >= 2^27): SA_ESHAPE,
 *      before the pointers
 *   5. a NULL pointer; `mag` or `out` not 16-byte aligned; [mag, mag + B * 65536) meeting
 *      [out, out + (B / A) * (16384 / W) * 8): SA_EINVAL.  Buffers that merely touch are fine; the call is never in place.
 * A launch the runtime refuses is SA_EHIP.  sa_fold_last_error() is the text of the calling thread's last refused call
 * ("" after a good one).
 * Known answers: a = 2, k = 0, B = 8 reads 524288 bytes and writes 262144; a = 0, k = 4, B = 8 writes 65536; a = 4, k = 4,
 * B = 16 writes 8192. */
#ifndef SPECAN_FOLD_H
#define SPECAN_FOLD_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_FOLD_VERSION 1
int sa_fold_version(void);

#define SA_FOLD_LOG2A_MAX 7
#define SA_FOLD_LOG2W_MAX 6

typedef struct sa_fold_point {
    float peak_mag;   /* max hold over the bucket's bins and the group's frames */
    float power;      /* the sum of m^2 over them */
} sa_fold_point;      /* 8 bytes */

int sa_fold_mag_f32(const float *mag, sa_fold_point *out, int batch, int log2a, int log2w, void *stream);

/* The refusals above as a pure function: no GPU, the addresses are compared as integers and never dereferenced. */
int sa_fold_check(int log2a, int log2w, uint64_t in_addr, uint64_t out_addr, int batch);

const char *sa_fold_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
