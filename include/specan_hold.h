/* specan_hold.h -- percentile traces: the value at given ranks of the sorted frames of each bin, over groups of consecutive
 * frames, found on the device.
 *
 * specan_rank.h gives order statistics along the frequency axis: one number per row.  Along the time axis the project has
 * the two traces of a fold -- the max hold and the power sum of A frames (specan_fold.h, specan_ext.h) -- and the level
 * histogram.  An analyser's trace menu also has the min hold and a median or percentile trace: the mean of a fold is dragged
 * up by every burst and a max hold keeps a burst for the whole hold time, while the per-bin median over frames is the floor
 * under hopping or pulsed emitters and the true level of a stationary carrier; a low percentile is the floor under anything
 * intermittent and the min hold is its limit.  This call reads the R rows of 16384 points a chain or a fold wrote and writes
 * q rows of 16384 floats per group of A rows.  The rows it writes are plain magnitude rows (layout 0 of every header here),
 * so every other library takes them as they are.  It is a pure function of a device tensor: no handle, no workspace, no
 * state.  The functions are exported by libspecan_hold.so, a library of its own that links the HIP runtime and nothing else;
 * no name of the other headers is in it, and none of those surfaces changes.  This header is plain C and includes specan.h
 * for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts and values of specan_rank.h):
 *   0  SA_HOLD_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_HOLD_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) -- sa_fold_point at W = 1, or the
 *                              sa_trace_point_q15 of sa_spectra_q15 -- of which the FIRST float is the point;
 *   2  SA_HOLD_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Key: a point has the key u, the float's bit pattern with the sign bit cleared, read as a 32-bit unsigned integer -- the
 * rule of specan_fold.h, specan_peaks.h and specan_rank.h.  It is the float order of non-negative values; +inf ranks above
 * every finite value; a NaN ranks above +inf, so it shows instead of vanishing; -0.0 counts as +0.0; the compare is an
 * integer one, so no denormal is flushed.
 * Group: `group` = A is any integer 2 <= A <= SA_HOLD_GROUP_MAX, not only a power of two (medians of 3, 5 or 15 frames are
 * natural).  `rows` must be a multiple of A; G = rows / A, and group g is the rows [g A, (g + 1) A).
 * Ranks: q integers ranks[0..q), 1 <= q <= SA_HOLD_Q_MAX, each 0 <= ranks[j] < A, in any order, repeats allowed.  `ranks` is
 * a HOST pointer: the values travel by value in the kernel's arguments, so they are stream-ordered for free, the array may be
 * reused as soon as the call returns, and the call can be captured into a graph.
 * Output: float32 out[G, q, 16384]: out[g][j][i] is the float whose bits are s[ranks[j]], where s is the ascending sort of
 * the A keys of bin i in group g.  Rank 0 is the min hold, rank A - 1 the max hold, rank (A - 1) / 2 the lower median.  Each
 * [g][j] slice is a layout-0 row of 64 KiB.  A value depends only on its own bin in its own A rows.  The keys are integers
 * and the result is one of them: nothing depends on an order of evaluation, there are no atomics, and the output is
 * bit-reproducible.
 * Consequences: rank A - 1 is the peak (the first float) of sa_fold_mag_f32 at the same A and W = 1 on the same rows, bit for
 * bit, for every A that call takes (a power of two): both are the maximum of the same keys.  A rank equals the sort of the
 * keys along the frame axis.
 * Cost: every key is read once and sorted in registers by a fixed network of compare-exchange steps, all ranks at once: the
 * time does not depend on the data and hardly on q.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_hold_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch, nothing else -- it can be captured into a graph at any time and may be called from any thread.
 * Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's streams with sa_flush(h, stream)
 * first.
 *
 * Refusals, all before any launch, in this order; sa_hold_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced.  Only `ranks` is read, and only after `group` and q have passed:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; `group` outside 2..SA_HOLD_GROUP_MAX; q outside 1..SA_HOLD_Q_MAX; `ranks` NULL; any rank outside
 *      [0, group): SA_EINVAL, also at rows 0
 *   3. rows not a multiple of `group`: SA_ESHAPE
 *   4. rows 0: SA_OK, whatever `in` and `out` are
 *   5. `in` or `out` NULL; either not 16-byte aligned;
 *        [in, in + rows * 65536 * (field ? 2 : 1))   meeting   [out, out + (rows / group) * q * 65536):
 *      SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on differences that cannot wrap, every size in
 *      64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads along the grid's x, which holds the groups: 2^24 groups or more) is
 * SA_EHIP.  sa_hold_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 6, group 3, q 8 reads 393216 bytes and writes 1048576; field 2, rows 2, group 2, q 1 reads
 * 262144 and writes 65536; field 1, rows 256, group 128, q 2 reads 33554432 and writes 262144. */
#ifndef SPECAN_HOLD_H
#define SPECAN_HOLD_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_HOLD_VERSION 1
int sa_hold_version(void);

#define SA_HOLD_Q_MAX 8
#define SA_HOLD_GROUP_MAX 128

#define SA_HOLD_IN_MAG         0
#define SA_HOLD_IN_POINT_PEAK  1
#define SA_HOLD_IN_POINT_POWER 2

int sa_hold_f32(const void *in, int field, float *out, int rows, int group, int q, const int32_t *ranks, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced, `ranks` is
 * a host array of q values (read only after `group` and q have passed). */
int sa_hold_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, int group, int q, const int32_t *ranks);

const char *sa_hold_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
