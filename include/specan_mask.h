/* specan_mask.h -- spectral mask test and frequency-mask trigger: every row of 16384 points held against an upper and a lower
 * limit line, one record per row (how many bins left the mask, where, and the worst bin of either limit with its value and
 * its limit), and for the call the rows that failed and the first and last of them, found on the device.
 *
 * A mask is the envelope a spectrum is allowed to be in: limit lines over the bins, with gaps where nothing is asked.  The
 * verdict per spectrum is pass or fail; the frequency-mask trigger is the first spectrum of a batch that left the mask, and the
 * margin is how far the worst bin stands from its limit.  This call reads the R rows of 16384 points a chain or a fold wrote
 * and two arrays of 16384 limits, and writes 40 bytes per row and 16 per call.  It is a pure function of device tensors: no
 * handle, no workspace, no state.  The functions are exported by libspecan_mask.so, a library of its own beside
 * libspecan_hip.so, libspecan_fold.so, libspecan_peaks.so, libspecan_rank.so, libspecan_hist.so and libspecan_bands.so that
 * links the HIP runtime and nothing else; no name of the other headers is in it, and none of those surfaces changes.  This
 * header is plain C and includes specan.h for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts and values of specan_bands.h):
 *   0  SA_MASK_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_MASK_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) -- sa_fold_point at W = 1, or the
 *                              sa_trace_point_q15 of sa_spectra_q15 -- of which the FIRST float is the point;
 *   2  SA_MASK_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Value: a[i] is the point with its sign bit cleared, a float32 (a denormal is kept, -0.0 is +0.0, a NaN stays a NaN).
 * Nothing is squared: the limits are in the unit of the points, so for layout 2 they are powers.
 * Limits: `upper` and `lower` are DEVICE pointers to float32 [16384], u and l, shared by all rows.  Either may be NULL (that
 * limit does not exist), not both.  Bin i has an upper limit when u[i] is finite and > 0 (a denormal included), a lower limit
 * when l[i] is finite and > 0; any other value -- 0, a negative number, +-inf, a NaN -- means "no limit here": that is how a
 * caller leaves gaps.  The two may be the SAME pointer (both are only read: the points must then equal the line); two limit
 * arrays that meet in any other way are refused.
 * Range: 0 <= lo < hi <= 16384; bins outside [lo, hi) do not exist for the call.
 * Per row, one record of 40 bytes:
 *   over    the number of bins with an upper limit where a[i] > u[i] (the float32 compare) or a[i] is a NaN;
 *   under   the number of bins with a lower limit where a[i] < l[i] or a[i] is a NaN;
 *   first, last   the lowest and the highest bin counted in either, or -1;
 *   up_bin  the bin with an upper limit that maximises a[i] / u[i], the ratio compared as the EXACT ratio of the two float32
 *           values: +inf is larger than every finite ratio, a NaN point stands as +inf, and equal ratios go to the lowest
 *           bin.  up_val holds the bits of a[up_bin] (of a NaN only isnan is specified), up_lim = u[up_bin].  With no such
 *           bin up_bin is -1 and both floats are +0.0;
 *   lo_bin, lo_val, lo_lim   the same for the lower limit: the bin minimising a[i] / l[i]; a NaN point stands as 0 there, and
 *           equal ratios go to the lowest bin.
 * The margin in dB is 20 log10(up_val / up_lim) on the host (10 log10 for powers); the device takes no logarithm.
 * over > 0 iff up_val > up_lim or isnan(up_val); under > 0 iff lo_val < lo_lim or isnan(lo_val).
 * The exact order: the product of two float32 values is exact in float64 (48 bits of 53, exponents -298 .. 256), so
 * a_i u_j > a_j u_i decides a_i / u_i > a_j / u_j without a rounding; that is the form the kernel and the mirror use.  A
 * correctly rounded float64 quotient orders every pair the same way (unequal ratios of 24-bit mantissas differ by at least
 * 2^-48 relative); a float32 quotient does not -- it ties and inverts near-equal ratios.  The order is total -- larger
 * ratio, then lower bin -- so the worst bin does not depend on the order in which the bins are compared.
 * Per call, when `summary` is not NULL, four int32: the rows with over > 0, the rows with under > 0, the first row with either
 * or -1, the last row with either or -1 -- the trigger.  All are integers: any order of combination gives the same bits.
 * A row depends on its own points and the limits alone; there are no atomics, and the output is bit-reproducible.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_mask_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device.  With `summary` NULL it is ONE kernel launch of one workgroup per row; with a summary a second launch of one
 * workgroup follows on the same stream, reads the records the first wrote and stores the four integers -- no atomics, no
 * memset, nothing to zero: the call can be captured into a graph at any time, every replay gives the summary of that replay's
 * input, and it may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join
 * the handle's streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_mask_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; not 0 <= lo < hi <= 16384; `upper` and `lower` both NULL: SA_EINVAL, also at rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. `in` or `rows_out` NULL; `in`, `upper` or `lower` not 16-byte aligned, `rows_out` not 8-byte aligned, `summary` not
 *      4-byte aligned; any two of
 *        [in, in + rows * 65536 * (field ? 2 : 1)),   [upper, upper + 65536),   [lower, lower + 65536),
 *        [rows_out, rows_out + rows * 40),   [summary, summary + 16)
 *      meeting, a NULL limit and a NULL summary being empty, except `upper` == `lower`: SA_EINVAL.  Buffers that merely
 *      touch are fine.  The overlap is decided on differences that cannot wrap, every size in 64-bit arithmetic (rows < 2^31:
 *      at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24, a terabyte of input) is SA_EHIP.
 * sa_mask_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3 reads 196608 bytes of points and 65536 of each limit and writes 120 + 16; field 2, rows 1
 * with `lower` and `summary` NULL reads 131072 and 65536 and writes 40 and no summary byte. */
#ifndef SPECAN_MASK_H
#define SPECAN_MASK_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_MASK_VERSION 1
int sa_mask_version(void);

#define SA_MASK_IN_MAG         0
#define SA_MASK_IN_POINT_PEAK  1
#define SA_MASK_IN_POINT_POWER 2

typedef struct { int32_t over, under, first, last, up_bin, lo_bin; float up_val, up_lim, lo_val, lo_lim; } sa_mask_row;

int sa_mask_f32(const void *in, int field, const float *upper, const float *lower, int lo, int hi, sa_mask_row *rows_out,
                int32_t *summary, int rows, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced. */
int sa_mask_check(uint64_t in_addr, int field, uint64_t upper_addr, uint64_t lower_addr, int lo, int hi, uint64_t rows_out_addr,
                  uint64_t summary_addr, int rows);

const char *sa_mask_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
