/* specan_bands.h -- band power and occupied bandwidth per spectrum: the power of each row summed over given ranges of bins, in
 * float64, and the bins at which the cumulative power of a range crosses given fractions of it, found on the device.
 *
 * Channel power and adjacent-channel power ratio are sums of power over a handful of bin ranges; occupied bandwidth is the
 * pair of bins at which the cumulative power of a span crosses 0.5 % and 99.5 %.  This call reads the R rows of 16384 points a
 * chain or a fold wrote and writes nb doubles and nb * nq bins per row.  It is a pure function of a device tensor: no handle,
 * no workspace, no state.  The functions are exported by libspecan_bands.so, a library of its own beside libspecan_hip.so,
 * libspecan_fold.so, libspecan_peaks.so, libspecan_rank.so and libspecan_hist.so that links the HIP runtime and nothing else;
 * no name of the other headers is in it, and none of those surfaces changes.  This header is plain C and includes specan.h
 * for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts and values of specan_peaks.h and
 * specan_rank.h):
 *   0  SA_BANDS_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_BANDS_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) -- sa_fold_point at W = 1, or the
 *                               sa_trace_point_q15 of sa_spectra_q15 -- of which the FIRST float is the point;
 *   2  SA_BANDS_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Value: a is the point with its sign bit cleared, widened to float64 (exact; a float32 denormal is kept).  For layouts 0 and
 * 1, v[i] = a * a: the product of two float32 values is exact in float64, so a contraction into an fma cannot change a bit.
 * For layout 2, v[i] = a: the record's second float already is a power sum (of sa_fold_mag_f32 over A frames it is the sum
 * over the frames; the mean is / A on the host).
 * Band j: 0 <= lo_j < hi_j <= 16384; bands may overlap, repeat and come in any order.  w[i] = v[i] for lo_j <= i < hi_j and
 * +0.0 outside: bins outside a band do not exist for it.
 * Tree: T0 = w, T(l+1)[k] = T(l)[2k] + T(l)[2k+1] for l = 0..13, S = T14[0]: the balanced tree of adjacent pairs that
 * sa_fold_mag_f32 uses across a bucket, continued to the whole row.  power[r][j] = S, a float64 that is not rounded further.
 * Where the result is a NaN only isnan is specified.
 * Crossing q of band j (only when nq > 0): t = fracs[q] * S, rounded once to float64.  Descend from the root with E = +0.0
 * and k = 0: for l = 13 down to 0, let L = T(l)[2k]; if E + L >= t then k = 2k, otherwise E = E + L and k = 2k + 1.  At the
 * leaf, cross[r][j][q] = min(max(k, lo_j), hi_j - 1) if E + w[k] >= t, else -1.  A NaN in the band gives -1 (every compare
 * is false); an all-zero band gives lo_j; a fraction of 0 gives lo_j.  Fractions are doubles in [0, 1 - 2^-32] and need not
 * be sorted: the descent's partial sums and S associate differently and can differ by a few units of 14 * 2^-53 S, so below
 * that bound the last bin of the band always satisfies the test, and nearer to 1 it might not.  Occupied bandwidth at 99 %
 * is fracs = (0.005, 0.995); the power median of a band is 0.5.
 * The crossing is a descent of the tree and not "the first bin whose running sum reaches t": floating-point prefix sums taken
 * through different nodes are not monotone to the last bit, so the first-bin rule would need every bin of every band; the
 * descent is 14 steps.  Away from fractions aimed at a bin's own prefix the two rules name the same bin.
 * Output: float64 power[R, nb] and, when nq > 0, int32 cross[R, nb, nq].  A row depends on its own points alone; the order
 * of every addition is fixed above, there are no atomics, and the output is bit-reproducible.
 * `bands` and `fracs` are HOST pointers: their values travel by value in the kernel's arguments (128 + 32 bytes), so they are
 * stream-ordered for free, the arrays may be reused as soon as the call returns, and the call can be captured into a graph.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_bands_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, no atomics, no memset -- it can be captured into a graph at any time
 * and may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's
 * streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_bands_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced.  `bands` is read only after nb has passed, `fracs` only after nq has:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; nb outside 1..SA_BANDS_MAX; `bands` NULL; a band that is not 0 <= lo < hi <= 16384; nq outside
 *      0..SA_BANDS_Q_MAX; nq > 0 with `fracs` NULL; a fraction that is a NaN or outside [0, 1 - 2^-32]: SA_EINVAL, also at
 *      rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. `in` or `power` NULL; `cross` NULL with nq > 0 (with nq 0, `cross` is never looked at); `in` not 16-byte aligned,
 *      `power` not 8-byte aligned, `cross` not 4-byte aligned; any two of
 *        [in, in + rows * 65536 * (field ? 2 : 1)),   [power, power + rows * nb * 8),   [cross, cross + rows * nb * nq * 4)
 *      meeting: SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on differences that cannot wrap, every
 *      size in 64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24, a terabyte of input) is SA_EHIP.
 * sa_bands_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3, nb 2, nq 2 reads 196608 bytes and writes 48 + 48; field 2, rows 1, nb 16, nq 0 reads 131072
 * and writes 128 and no `cross` byte. */
#ifndef SPECAN_BANDS_H
#define SPECAN_BANDS_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_BANDS_VERSION 1
int sa_bands_version(void);

#define SA_BANDS_MAX   16          /* bands per call */
#define SA_BANDS_Q_MAX 4           /* crossing fractions per call */

#define SA_BANDS_IN_MAG         0
#define SA_BANDS_IN_POINT_PEAK  1
#define SA_BANDS_IN_POINT_POWER 2

typedef struct { int32_t lo, hi; } sa_band;

int sa_bands_f32(const void *in, int field, double *power, int32_t *cross, int rows, int nb, const sa_band *bands, int nq,
                 const double *fracs, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced, `bands` is a
 * host array of nb entries (read only after nb has passed) and `fracs` one of nq (read only after nq has). */
int sa_bands_check(int field, uint64_t in_addr, uint64_t power_addr, uint64_t cross_addr, int rows, int nb,
                   const sa_band *bands, int nq, const double *fracs);

const char *sa_bands_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
