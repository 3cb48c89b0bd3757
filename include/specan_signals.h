/* specan_signals.h -- the signal list per spectrum: the contiguous runs of bins that stand above a threshold, each with its
 * start and stop, its peak and its float64 power, and how much of the span is occupied, found on the device.
 *
 * A monitoring receiver asks of every spectrum which emissions are there and how wide each is.  The peak table
 * (specan_peaks.h) says where the maxima are, not whether two of them are one signal; the order statistics (specan_rank.h)
 * give the noise floor a threshold rides on, and this call takes that threshold per row from device memory.  It reads the R
 * rows of 16384 points a chain or a fold wrote and writes k records of 24 bytes and three counters per row.  It is a pure
 * function of device tensors: no handle, no workspace, no state.  The functions are exported by libspecan_signals.so, a
 * library of its own beside libspecan_hip.so, libspecan_fold.so, libspecan_peaks.so, libspecan_rank.so, libspecan_hist.so,
 * libspecan_bands.so, libspecan_mask.so and libspecan_harm.so that links the HIP runtime and nothing else; no name of the
 * other headers is in it, and none of those surfaces changes.  This header is plain C and includes specan.h for SA_N and the
 * SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts of specan_peaks.h):
 *   0  SA_SIGNALS_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_SIGNALS_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) of which the FIRST float is the point;
 *   2  SA_SIGNALS_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Key: u[i] is the point's bits with the sign cleared, as a uint32: a NaN is above +inf, -0.0 is +0.0, denormals are kept.
 * Threshold of row r: with `thr` NULL, T_r = key(threshold) for every row; with `thr` given (float32 [R] in device memory),
 * T_r = key(thr[r]), keyed like a point, and `threshold` is not looked at: a negative value counts by its magnitude, a NaN
 * lies above +inf so that only NaN points pass, and a zero lets every non-zero bin pass.
 * On: bin i is on when lo <= i < hi, u[i] > 0 and u[i] >= T_r.  A zero is never on.
 * Closing: an off bin i of [lo, hi) is bridged when an on bin p < i and an on bin n > i exist with no on bin between p and n
 * and n - p - 1 <= gap: the off runs of at most `gap` bins that have an on bin at either end are filled.  gap = 0 bridges
 * nothing; on bins outside [lo, hi) do not exist.  closed = on or bridged.
 * Segments: the maximal runs [start, stop) of closed bins, of which one is kept when stop - start >= min_width.  The records
 * of a row are its first k kept segments in ascending bin order.
 * Record (sa_signal, 24 bytes, every byte written exactly once and nothing beyond the k records of a row):
 *   start, stop      the run [start, stop)
 *   peak, peak_bin   the largest key of the segment as a float (the point with its sign cleared) and its bin, equal keys to
 *                    the lowest bin
 *   power            the float64 sum S of specan_bands.h for the band [start, stop) of that row: v[i] = a * a for layouts 0
 *                    and 1 and v[i] = a for layout 2, a the float of u[i] widened to float64; w[i] = v[i] inside the band and
 *                    +0.0 outside, over the whole row; T0 = w, T(l+1)[k] = T(l)[2k] + T(l)[2k+1] for l = 0..13, S = T14[0].
 *                    Bridged bins are in the band.  Not rounded further; of a NaN only isnan is specified.
 *   unused slots     (-1, -1, +0.0f, -1, +0.0)
 * Row statistics, int32 stats[R][3]:
 *   count      the number of kept segments before the truncation to k
 *   occupied   the number of on bins
 *   covered    the sum of stop - start over all kept segments, those beyond k included
 * A row depends on its own points and its own thr[r] alone -- the call reads nothing else -- the order of every addition is
 * fixed above, there are no atomics, and every byte of `out` and `stats` is bit-reproducible and stored exactly once.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_signals_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, the parameters in its arguments, no atomics, no memset -- it can be
 * captured into a graph at any time and may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode
 * (sa_set_overlap), join the handle's streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_signals_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced and the threshold as its bits:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; k outside 1..SA_SIGNALS_K_MAX; `thr` NULL and `threshold` a NaN or with the sign bit set (-0.0
 *      included); not 0 <= lo < hi <= 16384; gap outside 0..16383; min_width outside 1..16384: SA_EINVAL, also at rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. `in`, `out` or `stats` NULL; `in` not 16-byte aligned; `out` not 8-byte aligned; `stats` or `thr` not 4-byte aligned;
 *        [out, out + rows * k * 24)   or   [stats, stats + rows * 12)
 *      meeting each other, [in, in + rows * 65536 * (field ? 2 : 1)) or [thr, thr + rows * 4): SA_EINVAL.  `in` and `thr` are
 *      only read and may meet each other.  Buffers that merely touch are fine.  The overlap is decided on differences that
 *      cannot wrap, every size in 64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24) is SA_EHIP.
 * sa_signals_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3, k 8 with `thr` reads 196608 + 12 bytes and writes 576 + 36; field 2, rows 1, k 32 without
 * `thr` reads 131072 and writes 768 + 12.  A row that is +0.0 but for 1.0 at bins 10, 11 and 14 gives, with threshold 0.5,
 * gap 0, min_width 1: (10, 12, 1.0, 10, 2.0), (14, 15, 1.0, 14, 1.0) and stats (2, 3, 3); with gap 2: (10, 15, 1.0, 10, 3.0)
 * and stats (1, 3, 5); with gap 0 and min_width 2: (10, 12, 1.0, 10, 2.0) and stats (1, 3, 2). */
#ifndef SPECAN_SIGNALS_H
#define SPECAN_SIGNALS_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_SIGNALS_VERSION 1
int sa_signals_version(void);

#define SA_SIGNALS_K_MAX 32         /* the most records of a row */

#define SA_SIGNALS_IN_MAG         0
#define SA_SIGNALS_IN_POINT_PEAK  1
#define SA_SIGNALS_IN_POINT_POWER 2

typedef struct {
    int32_t start, stop;            /* the bins [start, stop); -1, -1 in an unused slot */
    float   peak;
    int32_t peak_bin;
    double  power;
} sa_signal;

int sa_signals_f32(const void *in, int field, const float *thr, float threshold, sa_signal *out, int32_t *stats, int rows, int k,
                   int lo, int hi, int gap, int min_width, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced;
 * `threshold_bits` is the float's bit pattern and is looked at only where `thr_addr` is 0. */
int sa_signals_check(int field, uint64_t in_addr, uint64_t thr_addr, uint32_t threshold_bits, uint64_t out_addr,
                     uint64_t stats_addr, int rows, int k, int lo, int hi, int gap, int min_width);

const char *sa_signals_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
