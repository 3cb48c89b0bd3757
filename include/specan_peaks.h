/* specan_peaks.h -- the peak table: the K strongest local maxima of each spectrum, found on the device.
 *
 * The reduced outputs of specan.h, specan_ext.h and specan_fold.h give one peak per frame (SA_OUT_MARKER,
 * SA_Q15_OUT_MARKER), bucketed traces and folds over groups of frames.  What an analyser's peak table needs -- the K strongest
 * signals of a spectrum with their bins: a second tone, the mirror line, a spur beside a carrier -- took the full spectrum on
 * the host (np.max / np.argmax of the user's slice, gui.py:415-455, answers K = 1 only).  This call reads the R rows of
 * 16384 points a chain or a fold wrote and writes K records and one count per row.  It is a pure function of a device tensor:
 * no handle, no workspace, no state.  The functions are exported by libspecan_peaks.so, a library of its own beside
 * libspecan_hip.so and libspecan_fold.so that links the HIP runtime and nothing else; no name of specan.h, specan_ext.h or
 * specan_fold.h is in it, and none of those surfaces changes.  This header is plain C and includes specan.h for SA_N and the
 * SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field`:
 *   0  SA_PEAKS_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_PEAKS_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) -- sa_fold_point at W = 1, or the
 *                               sa_trace_point_q15 of sa_spectra_q15 -- of which the FIRST float is the point;
 *   2  SA_PEAKS_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Key: point i has the key u[i], the float's bit pattern with the sign bit cleared, read as a 32-bit unsigned integer -- the
 * rule of specan_fold.h.  It is the float order of non-negative values; +inf ranks above every finite value; a NaN ranks
 * above +inf, so it shows instead of vanishing; -0.0 counts as +0.0; the compare is an integer one, so no denormal is
 * flushed.  key(threshold) is formed the same way.
 * Candidate: bin i is a candidate when all five hold:
 *     lo <= i < hi;   u[i] > 0;   u[i] >= key(threshold);   u[i] > u[i-1];   u[i] >= u[i+1].
 * The neighbours are the row's neighbours whether or not they lie in [lo, hi).  A neighbour that does not exist (i = 0,
 * i = 16383) satisfies its condition.  A plateau therefore yields its lowest bin, two adjacent bins are never both
 * candidates, and a zero is never a peak.  The conditions look one bin to each side and no further: the lowest bin of a plateau
 * is a candidate also where the plateau ends in a rise (5 5 7 gives the first 5 and the 7); what the rise rules out is every
 * later bin of the plateau.
 * Selection: order the candidates by larger key first, then lower bin, and walk that order: a candidate p is accepted when
 * |p - q| >= min_sep for every q accepted before it; stop at K accepted.  min_sep = 1 suppresses nothing, and a candidate
 * that was not accepted suppresses nothing.
 * Output: sa_peak [R,K], the accepted peaks of each row in acceptance order, `mag` the input float with its sign cleared; the
 * remaining slots are (+0.0f, -1).  int32 count[R] is the number of candidates of the row, before suppression and
 * truncation.  A row depends on its own 16384 points alone; there are no atomics and no order that depends on scheduling:
 * the records are bit-reproducible.
 * Consequence: with K = 1, threshold 0 and the range [0, 16384) the record is (peak_mag, peak_bin) of SA_OUT_MARKER /
 * SA_Q15_OUT_MARKER over the full range on the same frame, bit for bit, whenever that peak is not zero.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_peaks_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, nothing else -- it can be captured into a graph at any time and may be
 * called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's streams
 * with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_peaks_check() gives the same codes from the same code, as a pure
 * function of integers (threshold_bits is the bit pattern of `threshold`):
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; k outside 1..SA_PEAKS_K_MAX; a threshold that is a NaN or has its sign bit set (-0.0 included);
 *      a range that is not 0 <= lo < hi <= 16384; min_sep outside 1..16384: SA_EINVAL, also at rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. a NULL pointer; `in` not 16-byte aligned; `out` not 8-byte aligned; `count` not 4-byte aligned; any two of
 *        [in, in + rows * 65536 * (field ? 2 : 1)),   [out, out + rows * k * 8),   [count, count + rows * 4)
 *      meeting: SA_EINVAL.  Buffers that merely touch are fine.  Every size is decided in 64-bit arithmetic that cannot wrap
 *      (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24, a terabyte of input) is SA_EHIP.
 * sa_peaks_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 1, rows 8, k 8 reads 1048576 bytes and writes 512 + 32; field 0, rows 3, k 32 reads 196608 and writes
 * 768 + 12; field 2, rows 1, k 1 reads 131072 and writes 8 + 4. */
#ifndef SPECAN_PEAKS_H
#define SPECAN_PEAKS_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_PEAKS_VERSION 1
int sa_peaks_version(void);

#define SA_PEAKS_K_MAX 32

#define SA_PEAKS_IN_MAG         0
#define SA_PEAKS_IN_POINT_PEAK  1
#define SA_PEAKS_IN_POINT_POWER 2

typedef struct sa_peak {
    float   mag;   /* the point with its sign cleared; +0.0f in an unused slot */
    int32_t bin;   /* 0..16383; -1 in an unused slot */
} sa_peak;         /* 8 bytes */

int sa_peaks_f32(const void *in, int field, sa_peak *out, int32_t *count, int rows, int k, float threshold, int lo, int hi,
                 int min_sep, void *stream);

/* The refusals above as a pure function: no GPU, the addresses are compared as integers and never dereferenced. */
int sa_peaks_check(int field, uint64_t in_addr, uint64_t out_addr, uint64_t count_addr, int rows, int k,
                   uint32_t threshold_bits, int lo, int hi, int min_sep);

const char *sa_peaks_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
