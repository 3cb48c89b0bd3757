/* specan_ext.h -- data-plane calls added after the version-4 surface of specan.h closed.
 *
 * specan.h at SA_ABI_VERSION 4 is frozen: its set of functions, the accepted values of every kind word and the answers of
 * sa_debug_check_pointers() are pinned, so that a caller built against it never meets a word that changed its meaning.  A
 * call that needs an argument list of its own therefore lives here.  The functions are exported by the same
 * libspecan_hip.so, take the same sa_handle and follow every rule of specan.h that is not restated (one thread per handle,
 * asynchronous on `stream`, error text through sa_last_error, the pointer contract).  This header is plain C and includes
 * specan.h.  sa_ext_version() returns the SA_EXT_VERSION the library was built with; a version adds functions and never
 * changes one.
 *
 * ---- full-resolution max hold and summed power over groups of A = 2^a frames (version 1) ------------------------------
 * The reduced outputs of specan.h (SA_Q15_TRACE_KIND, SA_Q15_TRACE_AVG_KIND) start at buckets of W = 2 bins.  These calls
 * keep all 16384 bins, the analyser's 61 Hz resolution, and reduce over frames alone: the input of a Welch estimate at hop
 * N/2 or N/4, or a max-hold display.  `out` is sa_trace_point_q15 [B / A, 16384]; row g, bin k covers the frames
 * gA .. gA + A - 1 of the call (with a hop: the frames of the stream as SA_Q15_HOP_KIND numbers them):
 *   - peak_mag is the maximum over those A frames of the SA_Q15_OUT_MAG value of bin k, bit for bit.  The correctly rounded
 *     root is monotone, so it is the root of the largest s = fl(fl(re re) + fl(im im)): one root per point.
 *   - power is the float32 nearest (ties to even) to the EXACT integer sum of re^2 + im^2 over the A frames, at most
 *     128 x 2^31 = 2^38: one rounding of an exact sum.  It is the SUM: A is a power of two, so the mean is power / A exactly.
 *   - an all-zero group gives (+0.0f, +0.0f).  All 16384 bins: the marker range plays no part.
 *   - consistent with SA_Q15_TRACE_AVG_KIND(k, a): the largest peak_mag of the W = 2^k records [jW, (j+1)W) of a row is that
 *     kind's peak of bucket j, and the exact sums add up to its exact sum.
 * At A = 16 the call writes 8 KiB per input frame, the volume of the W = 16 trace, at 16 times its resolution.
 *
 * sa_spectra_q15 / sa_spectra_q15_p12: sa_process_q15_out / sa_process_q15_p12 with SA_Q15_OUT_IQ -- the same kernels, all
 * four filter modes, both window modes, custom ROMs -- writing its int16 [B,16384,2] frames into a workspace of the handle,
 * and ONE more launch behind it on the same stream that folds each group of A frames bin by bin.
 *   - log2a = SA_Q15_TRACE_LOG2A_MIN .. SA_Q15_TRACE_LOG2A_MAX (1..7), A = 2..128.
 *   - hop = 0: `in` is [B,16384] int16 frames (packed: [B,24576] bytes).  hop = 8..16384, a multiple of 8: `in` is ONE
 *     stream of SA_Q15_HOP_STREAM_SAMPLES(B, hop) samples, frame b from sample b * hop on, under the rules of
 *     SA_Q15_HOP_KIND.
 *   - the workspace is 64 KiB per frame and launch slot, grown by the call itself before anything is launched and never
 *     by sa_reserve(); a cascade mode (0x00, 0xA1, 0xA2 with sections) needs the cascade's workspace too, as ever.  A
 *     captured call whose workspace is too small is SA_ESTATE with nothing launched: make one call of that batch outside
 *     the capture first.  Once grown, the call captures and replays like any other.
 *   - every overlap depth, and launch timing: one device time per call, from its first launch to the fold.
 *
 * sa_fold_iq_q15: the fold alone, on frames the caller already has: `iq` is int16 [B,16384,2] in device memory, the wire
 * frames of SA_Q15_OUT_IQ.  One launch, no workspace, capturable always.
 *
 * Refusals, all before any call state exists (nothing launched, no profiling entry), in this order:
 *   1. (sa_ext_check_pointers alone) an unknown entry: SA_EINVAL
 *   2. a negative batch: SA_ESHAPE
 *   3. log2a outside 1..7; a hop that is neither 0 nor a multiple of 8 in 8..16384; any hop != 0 for the fold:
 *      SA_EINVAL, also at batch 0
 *   4. batch 0: SA_OK
 *   5. a batch that is no multiple of A: SA_ESHAPE, before the pointers
 *   6. a NULL pointer; `in` or `out` not 16-byte aligned; [in, in + in_bytes) meeting [out, out + out_bytes): SA_EINVAL.
 *      in_bytes is what the Q15 chain reads for that input form and hop (specan.h), for the fold B * 65536; out_bytes is
 *      (B / A) * 131072.
 * Known answers: entry 0, log2a = 2, hop 0, B = 8 reads 262144 bytes and writes 262144; the same at hop 4096 reads 90112
 * bytes (45056 samples), entry 1 there 67584; entry 2, log2a = 2, B = 8 reads 524288 and writes 262144. */
#ifndef SPECAN_EXT_H
#define SPECAN_EXT_H

#include "specan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_EXT_VERSION 1
int sa_ext_version(void);

int sa_spectra_q15(sa_handle *h, const int16_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream);
int sa_spectra_q15_p12(sa_handle *h, const uint8_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream);
int sa_fold_iq_q15(sa_handle *h, const int16_t *iq, sa_trace_point_q15 *out, int batch, int log2a, void *stream);

/* Introspection for tests: the refusals above as a pure function, as sa_debug_check_pointers is for specan.h -- no handle,
 * no GPU, the addresses are compared as integers and never dereferenced.  `hop` is ignored for no entry: the fold refuses
 * any hop != 0.  The entry points themselves ask the same code. */
#define SA_EXT_ENTRY_SPECTRA_Q15     0
#define SA_EXT_ENTRY_SPECTRA_Q15_P12 1
#define SA_EXT_ENTRY_FOLD_IQ_Q15     2
#define SA_EXT_ENTRY_COUNT           3
int sa_ext_check_pointers(int entry, int log2a, int hop, uint64_t in_addr, uint64_t out_addr, int batch);

#ifdef __cplusplus
}
#endif
#endif
