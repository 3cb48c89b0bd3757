/* specan_harm.h -- harmonic analysis per spectrum: the fundamental of each row, the power of its band and of the bands of its
 * harmonics where they alias to, the worst spur, and the power of everything else, in float64, found on the device.
 *
 * SFDR, THD, SINAD, SNR and ENOB of an ADC are ratios of a handful of sums and maxima over bins that sit at multiples of each
 * row's own peak, folded about n / 2: nothing a call with bands common to all rows can give.  This call reads the R rows of
 * 16384 points a chain or a fold wrote and writes one record of 168 bytes per row; the ratios are host arithmetic on the
 * records (frames.harm_metrics).  It is a pure function of a device tensor: no handle, no workspace, no state.  The functions
 * are exported by libspecan_harm.so, a library of its own beside libspecan_hip.so, libspecan_fold.so, libspecan_peaks.so,
 * libspecan_rank.so, libspecan_hist.so, libspecan_bands.so and libspecan_mask.so that links the HIP runtime and nothing else;
 * no name of the other headers is in it, and none of those surfaces changes.  This header is plain C and includes specan.h
 * for SA_N and the SA_E* codes.
 *
 * ---- the definition ---------------------------------------------------------------------------------------------------
 * Input: R rows of n = 16384 points in one of three layouts chosen by `field` (the layouts and values of specan_bands.h):
 *   0  SA_HARM_IN_MAG          float32 [R,16384]: what SA_OUT_MAG_FULL and SA_Q15_OUT_MAG write;
 *   1  SA_HARM_IN_POINT_PEAK   8-byte records [R,16384] of (float32, float32) of which the FIRST float is the point;
 *   2  SA_HARM_IN_POINT_POWER  the same records; the SECOND float is the point.  The other float is never looked at.
 * Key: u[i] is the point's bits with the sign cleared, as a uint32: a NaN is above +inf, -0.0 is +0.0, denormals are kept.
 * Value: a is the float of u[i] widened to float64 (exact).  v[i] = a * a for layouts 0 and 1 (exact in float64) and v[i] = a
 * for layout 2, which already is a power.
 * Parameters (sa_harm_cfg, int32 each; a HOST struct whose values travel in the kernel's arguments, so it may be reused as
 * soon as the call returns and the call can be captured into a graph):
 *   dc, top   the analysed bins are [dc, top), 0 <= dc < top <= 8193 (a real input mirrors above bin 8192);
 *   lo, hi    the fundamental is searched in [lo, hi), dc <= lo < hi <= top;
 *   fund      -1 searches; otherwise the fundamental is this bin, dc <= fund < top (coherent sampling);
 *   span      0..SA_HARM_SPAN_MAX: a tone's band reaches `span` bins to either side of its bin;
 *   order     H in 1..SA_HARM_MAX: harmonics 2..H are analysed; H = 1 analyses none.
 * Per row:
 *   k1        `fund` when given, else the bin of the largest key in [lo, hi), equal keys to the lowest bin (an all-zero row: lo);
 *   k_h       for h = 2..H the bin harmonic h aliases to: m = (h * k1) mod 16384, k_h = m <= 8192 ? m : 16384 - m -- the fold
 *             is about 8192 whatever `top` is;
 *   band(k)   [max(k - span, dc), min(k + span + 1, top)), which may be empty;
 *   F = band(k1), B_h = band(k_h) minus F, U = the union of the B_h (every bin once), A = [dc, top).
 * Sum of a set M: w[i] = v[i] for i in M and +0.0 outside, over the whole row; T0 = w, T(l+1)[k] = T(l)[2k] + T(l)[2k+1] for
 * l = 0..13, the sum is T14[0]: the balanced tree of adjacent pairs of specan_bands.h.  A float64 that is not rounded further;
 * of a NaN only isnan is specified.  Every sum below is a tree of its own: no identity between them holds to the last bit.
 * Largest of a set M: the largest key u[i], i in M, equal keys to the lowest bin; of an empty set (+0.0, bin -1).
 * The record (168 bytes, every byte written exactly once and nothing beyond it):
 *   power[0] = sum F; power[h-1] = sum B_h for h = 2..H; the other slots +0.0
 *   dist = sum U; nad = sum (A minus F); noise = sum (A minus F minus U)
 *   bin[0] = k1; bin[h-1] = k_h for h = 2..H; the other slots -1
 *   fund = the float of u[k1]
 *   spur, spur_bin = the largest of A minus F                       (the worst spur, harmonic or not: SFDR)
 *   nonharm, nonharm_bin = the largest of A minus F minus U         (the worst spur that is no harmonic)
 *   n_noise = the number of bins of A minus F minus U
 * A row depends on its own points below bin 8193 alone -- the call reads no other -- the order of every addition is fixed
 * above, there are no atomics, and the record is bit-reproducible.
 *
 * ---- the call ---------------------------------------------------------------------------------------------------------
 * sa_harm_f32() is asynchronous on `stream` (a hipStream_t, NULL = the default stream) of the calling thread's current
 * device: ONE kernel launch of one workgroup per row, no atomics, no memset -- it can be captured into a graph at any time
 * and may be called from any thread.  Behind sa_process_f32() on a handle in overlap mode (sa_set_overlap), join the handle's
 * streams with sa_flush(h, stream) first.
 *
 * Refusals, all before any launch, in this order; sa_harm_check() gives the same codes from the same code, with the
 * addresses as integers that are never dereferenced:
 *   1. rows < 0: SA_ESHAPE
 *   2. `field` outside 0..2; `cfg` NULL; then, in the order of the list above, a parameter outside its range: SA_EINVAL,
 *      also at rows 0
 *   3. rows 0: SA_OK, whatever the pointers are
 *   4. `in` or `out` NULL; `in` not 16-byte aligned; `out` not 8-byte aligned;
 *        [in, in + rows * 65536 * (field ? 2 : 1))   and   [out, out + rows * 168)
 *      meeting: SA_EINVAL.  Buffers that merely touch are fine.  The overlap is decided on differences that cannot wrap, every
 *      size in 64-bit arithmetic (rows < 2^31: at most 2^48 bytes).
 * A launch the runtime refuses (its limit is 2^32 threads, rows >= 2^24) is SA_EHIP.
 * sa_harm_last_error() is the text of the calling thread's last refused call ("" after a good one).
 * Known answers: field 0, rows 3 claims 196608 bytes of `in` and writes 504; field 2, rows 1 claims 131072 and writes 168.
 * With dc 4, top 8193, lo 4, hi 8193, fund -1, span 3, order 5, a row whose largest point of bins 4..8192 is at bin 6001 gives
 * bin = (6001, 4382, 1619, 7620, 2763, -1, -1, -1, -1, -1); at bin 4096, bin = (4096, 8192, 4096, 0, 4096, -1, ...), and
 * power[2] = power[3] = power[4] = +0.0: the third and fifth harmonic lie on the fundamental and the fourth below dc. */
#ifndef SPECAN_HARM_H
#define SPECAN_HARM_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_HARM_VERSION 1
int sa_harm_version(void);

#define SA_HARM_MAX      10         /* the highest harmonic: slots of power[] and bin[] */
#define SA_HARM_SPAN_MAX 64         /* the largest half width of a tone's band */
#define SA_HARM_TOP_MAX  8193       /* bins 0..8192: the spectrum of a real input */

#define SA_HARM_IN_MAG         0
#define SA_HARM_IN_POINT_PEAK  1
#define SA_HARM_IN_POINT_POWER 2

typedef struct {
    int32_t dc, top;
    int32_t lo, hi;
    int32_t fund;
    int32_t span;
    int32_t order;
} sa_harm_cfg;

typedef struct {
    double  power[SA_HARM_MAX];     /* unused slots +0.0 */
    double  dist, nad, noise;
    int32_t bin[SA_HARM_MAX];       /* k1, k_2 .. k_H; unused slots -1 */
    float   fund, spur, nonharm;
    int32_t spur_bin, nonharm_bin, n_noise;
} sa_harm_row;

int sa_harm_f32(const void *in, int field, sa_harm_row *out, int rows, const sa_harm_cfg *cfg, void *stream);

/* The refusals above as a pure function: no GPU; the addresses are compared as integers and never dereferenced, `cfg` is a
 * host struct. */
int sa_harm_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, const sa_harm_cfg *cfg);

const char *sa_harm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
