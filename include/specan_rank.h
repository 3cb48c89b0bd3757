/* specan_rank.h -- order statistics per spectrum: the value at given ranks of the sorted bins of each row, found on the device.
 *
 * The reduced outputs of specan.h, specan_ext.h, specan_fold.h and specan_peaks.h say where the signals are; every one of them
 * presupposes a noise floor (the `threshold` of sa_peaks_f32 is absolute).  The robust floor of a spectrum with lines in it is
 * an order statistic -- the median or a lower quantile of the bins of a range; a mean is dominated by the carrier -- and the
 * same primitive gives the minimum, the maximum and any percentile trace value.  This call reads the R rows of 16384 points a
 * chain or a fold wrote and writes q floats per row.  It is a pure function of a device tensor: no handle, no workspace, no
 * state.  The functions are exported by libspecan_rank.so, a library of its own beside libspecan_hip.so, libspecan_fold.so and
 * libspecan_peaks.so that links the HIP runtime and nothing else; no name of the other headers is in it, and none of those
 * surfaces changes.  This header is plain C and includes specan.h for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts and values of specan_peaks.h):
 *   0  SA_RANK_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_RANK_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) -- sa_fold_point at W = 1, or the
 *                              sa_trace_point_q15 of sa_spectra_q15 -- of which the FIRST float is the point;
 *   2  SA_RANK_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Key: point i has the key u[i], the float's bit pattern with the sign bit cleared, read as a 32-bit unsigned integer -- the
 * rule of specan_fold.h and specan_peaks.h.  It is the float order of non-negative values; +inf ranks above every finite
 * value; a NaN ranks above +inf, so it shows instead of vanishing; -0.0 counts as +0.0; the compare is an integer one, so no
 * denormal is flushed.
 * Range: 0 <= lo < hi <= 16384, m = hi - lo.  Bins outside [lo, hi) do not exist for the call.
 * Ranks: q integers ranks[0..q), 1 <= q <= SA_RANK_Q_MAX, each 0 <= ranks[j] < m, in any order, repeats allowed.  `ranks` is
 * a HOST pointer: the values travel by value in the kernel's arguments, so they are stream-ordered for free, the array may be
 * reused as soon as the call returns, and the call can be captured into a graph.
 * Output: float32 out[R, q]: out[r][j] is the float whose bits are s[ranks[j]], where s is the ascending sort of the m keys
 * of row r.  Rank 0 is the minimum, rank m - 1 the maximum; the lower median of the range is rank (m - 1) / 2.  A row depends
 * on its own m points alone.  The keys are integers and the result is one of them: nothing depends on an order of
 * evaluation, there are no atomics, and the output is bit-reproducible.
 * Consequences: rank m - 1 over [lo, hi) is peak_mag of SA_OUT_MARKER / SA_Q15_OUT_MARKER with that marker range on the same
 * frame, bit for bit; over the full range it is `mag` of sa_peaks_f32 at K = 1, threshold 0, wherever that is not zero.
 * Cost: the selection is exact and its time does not depend on the data: 31 rounds (one per bit of a key) of 64 integer
 * compares per thread and rank, about 31 * 64 * q vector compares per thread: linear in q.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_rank_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, nothing else -- it can be captured into a graph at any time and may be
 * called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's streams
 * with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_rank_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced.  Only `ranks` is read, and only after q and the range have passed:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; q outside 1..SA_RANK_Q_MAX; a range that is not 0 <= lo < hi <= 16384; `ranks` NULL; any rank
 *      outside [0, hi - lo): SA_EINVAL, also at rows 0
 *   3. rows 0: SA_OK, whatever `in` and `out` are
 *   4. `in` or `out` NULL; `in` not 16-byte aligned; `out` not 4-byte aligned;
 *        [in, in + rows * 65536 * (field ? 2 : 1))   meeting   [out, out + rows * q * 4):
 *      SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on differences that cannot wrap, every size in
 *      64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24, a terabyte of input) is SA_EHIP.
 * sa_rank_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3, q 8 reads 196608 bytes and writes 96; field 2, rows 1, q 1 reads 131072 and writes 4;
 * field 1, rows 8, q 2 reads 1048576 and writes 64. */
#ifndef SPECAN_RANK_H
#define SPECAN_RANK_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_RANK_VERSION 1
int sa_rank_version(void);

#define SA_RANK_Q_MAX 8

#define SA_RANK_IN_MAG         0
#define SA_RANK_IN_POINT_PEAK  1
#define SA_RANK_IN_POINT_POWER 2

int sa_rank_f32(const void *in, int field, float *out, int rows, int q, const int32_t *ranks, int lo, int hi, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced, `ranks` is
 * a host array of q values (read only after q and the range have passed). */
int sa_rank_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, int q, const int32_t *ranks, int lo, int hi);

const char *sa_rank_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
