/* specan_hist.h -- the level histogram per bin: for every column of a display and every amplitude level, how many of the
 * last A spectra passed through that cell, counted on the device.
 *
 * The reduced outputs of specan.h, specan_ext.h, specan_fold.h, specan_peaks.h and specan_rank.h keep one number per bin or
 * per row; none of them says how the spectra were distributed.  A max hold cannot tell a burst that was there once from a
 * carrier that was there always, and a mean hides the burst altogether.  The persistence (density) display of a real-time
 * analyser shows it: a count per (column, level) cell.  This call reads the rows of 16384 points a chain wrote and writes
 * those counts.  The counts are integers and add across calls, so one call per batch serves any persistence time: the host
 * adds or decays small uint32 images.  It is a pure function of a device tensor: no handle, no workspace, no state.  The
 * functions are exported by libspecan_hist.so, a library of its own beside libspecan_hip.so, libspecan_fold.so,
 * libspecan_peaks.so and libspecan_rank.so that links the HIP runtime and nothing else; no name of the other headers is in
 * it, and none of those surfaces changes.  This header is plain C and includes specan.h for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: `rows` rows of n = 16384 float32 points, [rows,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write.  The 8-byte
 * (peak, power) record layouts of the folds are out of scope for this version.
 * Key: a point's key is the float's bit pattern with the sign bit cleared, read as a 32-bit unsigned integer -- the rule of
 * specan_fold.h, specan_peaks.h and specan_rank.h.  It is the float order of non-negative values; +inf is above every finite
 * value; a NaN is above +inf; -0.0 is +0.0; the compare is an integer one, so no denormal is flushed.
 * Levels: nlev = L, 2 <= L <= SA_HIST_LEVELS_MAX.  `edges` is a HOST array of L - 1 floats; every edge has its sign bit
 * clear and is not a NaN (bits <= 0x7F800000), and the edge keys are non-decreasing: equal edges are allowed and give empty
 * levels.  The edges travel by value in the kernel's arguments, so they are stream-ordered for free, the array may be
 * reused as soon as the call returns, and the call can be captured into a graph.
 *   level(v) = #{ j : key(edges[j]) <= key(v) },   a number in 0..L-1.
 * A value equal to an edge belongs to the level above it; a NaN is always in level L - 1.
 * Columns: the bucket is W = 2^log2w bins, log2w in 0..6.  The range is 0 <= lo < hi <= 16384 with lo and hi multiples of W;
 * bins outside [lo, hi) do not exist for the call.  C = (hi - lo) / W; column c is the bins [lo + c W, lo + (c + 1) W).
 * Groups: group = A, 1 <= A <= 2^24, not necessarily a power of two; `rows` is a multiple of A; G = rows / A; group g is
 * the rows [g A, (g + 1) A).
 * Output: uint32 out[G, C, L], the L counters of a column adjacent: out[g][c][l] is the number of points (row, bin) of group
 * g and column c whose level is l.  Every counter of the output is written by the call: it needs no zeroed buffer.  For
 * every (g, c) the L counters sum to A W (at most 2^30: no counter can overflow).  The counts are integers: nothing depends
 * on an order of evaluation and the output is bit-reproducible.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_hist_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device, in one of two forms chosen from the arguments alone (never from the data):
 *   - ONE kernel launch, nothing else: no memset, no workspace, no global atomic; every output counter is stored once.  This
 *     is the form wherever G x T >= 256, T the number of 256-bin tiles that meet [lo, hi), or A < 64;
 *   - otherwise TWO kernel launches on `stream`: one that zeroes the G * C * L * 4 output bytes, then one in which
 *     min(ceil(512 / (G T)), A / 32) workgroups share a group's rows and add their counts to the output with integer
 *     global atomics.  Integer sums: the same bits as the first form, in any order of arrival.
 * Either form needs no zeroed buffer and no workspace, can be captured into a graph at any time and may be called from any
 * thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's streams with
 * sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_hist_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced.  Only `edges` is read, and only after nlev has passed:
 *   1. rows < 0: SA_ESHAPE
 *   2. group outside 1..2^24; log2w outside 0..6; nlev outside 2..SA_HIST_LEVELS_MAX; a range that is not
 *      0 <= lo < hi <= 16384 with both ends multiples of W; `edges` NULL; an edge with the sign bit set or a NaN; edge keys
 *      that decrease: SA_EINVAL, also at rows 0
 *   3. rows % group != 0: SA_ESHAPE
 *   4. rows 0: SA_OK, whatever `in` and `out` are
 *   5. `in` or `out` NULL; `in` not 16-byte aligned; `out` not 4-byte aligned;
 *        [in, in + rows * 65536)   meeting   [out, out + G * C * L * 4):
 *      SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on differences that cannot wrap, every size in
 *      64-bit arithmetic (rows < 2^31: at most 2^48 bytes read, 2^53 written).
 * A launch the runtime refuses (its limit is 2^32 threads) is SA_EHIP.
 * sa_hist_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: rows 8, group 4, log2w 4, nlev 32, the full range reads 524288 bytes and writes 262144; rows 3, group 1,
 * log2w 0, nlev 2, lo 16, hi 48 reads 196608 and writes 768. */
#ifndef SPECAN_HIST_H
#define SPECAN_HIST_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_HIST_VERSION 1
int sa_hist_version(void);

#define SA_HIST_LEVELS_MAX 64

int sa_hist_f32(const float *in, uint32_t *out, int rows, int group, int log2w, int nlev, const float *edges, int lo, int hi,
                void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced, `edges` is
 * a host array of nlev - 1 values (read only after nlev has passed). */
int sa_hist_check(uint64_t in_addr, uint64_t out_addr, int rows, int group, int log2w, int nlev, const float *edges, int lo,
                  int hi);

const char *sa_hist_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
