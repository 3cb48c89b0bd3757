/* specan_cfar.h -- the local noise floor per bin: cell-averaging CFAR normalisation of spectra, made on the device.
 *
 * The other reductions judge a row against one level: a threshold per row (specan_peaks.h, specan_signals.h), one floor per
 * row (specan_rank.h), limits shared by all rows (specan_mask.h).  A spectrum whose noise is shaped -- a filter in front of
 * the FFT -- has a floor that varies across the span, and a row-wide threshold is blind where the floor is low and raises
 * false alarms where it is high.  This call compares every bin with the mean power of T training cells on either side of
 * it, beyond G guard cells: a cell-averaging CFAR, with its greatest-of and smallest-of forms.  It reads the R rows of 16384
 * points a chain or a fold wrote and writes float32 [R,16384]: the ratio of every bin to its local floor, or the floor
 * itself.  That is layout 0 of every other library, so the peak table, the signal list, the mask test and the histogram work
 * on a whitened spectrum as they are.  It is a pure function of device tensors: no handle, no workspace, no state.  The
 * functions are exported by libspecan_cfar.so, a library of its own beside libspecan_hip.so, libspecan_fold.so,
 * libspecan_peaks.so, libspecan_rank.so, libspecan_hist.so, libspecan_bands.so, libspecan_mask.so, libspecan_harm.so and
 * libspecan_signals.so that links the HIP runtime and nothing else; no name of the other headers is in it, and none of those
 * surfaces changes.  This header is plain C and includes specan.h for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts of specan_signals.h):
 *   0  SA_CFAR_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_CFAR_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) of which the FIRST float is the point;
 *   2  SA_CFAR_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Point: a is the point with its sign cleared, widened to float64, denormals kept.  v = a * a for layouts 0 and 1 (a float32
 * squared is exact in float64), v = a for layout 2.
 * Cells: c[j] = v[j] for lo <= j < hi and c[j] = +0.0 for every other integer j, negative j and j beyond 16383 included.
 * Window sums by doubling, T = 2^log2_train: W0 = c, W(l+1)[j] = W(l)[j] + W(l)[j + 2^l] for l = 0..log2_train-1, W the
 * last level: W[j] is the balanced pair tree over the cells j .. j + T - 1 in bin order.
 * Sides of bin i, with G = guard: L = W[i - G - T] and nL the number of those T cells inside [lo, hi); R = W[i + G + 1] and
 * nR likewise.  hi - lo >= 2 G + 2 is required, so nL + nR >= 1 for every bin of the range.
 * Mode:
 *   0  SA_CFAR_MODE_CA   S = L + R and n = nL + nR
 *   1  SA_CFAR_MODE_GO   the side with the larger mean
 *   2  SA_CFAR_MODE_SO   the side with the smaller mean
 * For GO and SO: with nR == 0 the left, with nL == 0 the right; otherwise the left where L * (double)nR >= R * (double)nL
 * (GO) or <= (SO) holds, both rounded float64 products, compared and never subtracted; a tie goes left.  S and n are those of
 * the side taken.
 * Output for lo <= i < hi, `what`:
 *   0  SA_CFAR_OUT_RATIO   (float)((v * (double)n) / S): a correctly rounded float64 product and division, then round to
 *                          nearest even to float32; overflow gives +inf, a float32 denormal result is kept
 *   1  SA_CFAR_OUT_FLOOR   (float)(S / (double)n): the mean training power; its square root is the amplitude
 * Special cases, in this order:
 *   1. L or R a NaN (the side not taken included), or for RATIO the point a NaN: 0x7FC00000
 *   2. S == 0: RATIO is +0.0 where v == 0 and +inf otherwise; FLOOR is +0.0
 *   3. a quotient that is a NaN (infinity over infinity): 0x7FC00000, so that no other NaN pattern is ever written
 * Bins outside [lo, hi) are written +0.0.  Every float of `out` is stored exactly once.
 * A row depends on its own points alone, the order of every addition is fixed above, there are no atomics, and every byte of
 * `out` is bit-reproducible.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_cfar_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, the parameters in its arguments, no atomics, no memset -- it can be
 * captured into a graph at any time and may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode
 * (sa_set_overlap), join the handle's streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_cfar_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field`, `mode` outside 0..2 or `what` outside 0..1; log2_train outside 0..SA_CFAR_LOG2_TRAIN_MAX; guard outside
 *      0..SA_CFAR_GUARD_MAX; not 0 <= lo < hi <= 16384; hi - lo < 2 * guard + 2: SA_EINVAL, also at rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. `in` or `out` NULL; `in` or `out` not 16-byte aligned; [out, out + rows * 65536) meeting
 *      [in, in + rows * 65536 * (field ? 2 : 1)): SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on
 *      differences that cannot wrap, every size in 64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24) is SA_EHIP.
 * sa_cfar_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3 reads 196608 bytes and writes 196608; field 2, rows 1 reads 131072 and writes 65536.  A row
 * of 1.0 with 3.0 at bin 100, log2_train 2 (T = 4), guard 1, the full range, RATIO: CA gives 9.0 at bin 100, 0.5 at bins 97,
 * 98 and 102, and 1.0 at bins 0, 99, 101 and 16383; GO gives 0x3EAAAAAB (1/3) at bins 97, 98 and 102 and 9.0 at bin 100; SO
 * gives 1.0 at all of those and 9.0 at bin 100.  A row of 1.0 gives 1.0 everywhere in every mode. */
#ifndef SPECAN_CFAR_H
#define SPECAN_CFAR_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_CFAR_VERSION 1
int sa_cfar_version(void);

#define SA_CFAR_IN_MAG         0
#define SA_CFAR_IN_POINT_PEAK  1
#define SA_CFAR_IN_POINT_POWER 2

#define SA_CFAR_MODE_CA 0
#define SA_CFAR_MODE_GO 1
#define SA_CFAR_MODE_SO 2

#define SA_CFAR_OUT_RATIO 0
#define SA_CFAR_OUT_FLOOR 1

#define SA_CFAR_LOG2_TRAIN_MAX 6    /* T = 1, 2, ..., 64 training cells a side */
#define SA_CFAR_GUARD_MAX      64   /* guard cells a side */

int sa_cfar_f32(const void *in, int field, float *out, int rows, int log2_train, int guard, int mode, int what, int lo, int hi,
                void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced. */
int sa_cfar_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, int log2_train, int guard, int mode, int what,
                  int lo, int hi);

const char *sa_cfar_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
