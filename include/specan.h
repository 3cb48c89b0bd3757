/*
 * specan.h -- C ABI of the MI355X spectrum-analyser signal path (libspecan_hip.so).
 *
 * Drop-in boundary for the hot path of mfkiwl/fpga-real-time-fft-analyzer:
 *     hann_window  ->  filter_iir12 | filter_iir12_cust  ->  xfft_0 (16384-pt)  ->  frame bytes
 * The reference exposes no FFI; its boundary is the byte contract between the FPGA and
 * scripts/fft_analyzer_gui.py.  Every entry point below cites the reference interface it
 * replaces (paths relative to the reference root; new/ = SDR_v2.srcs/sources_1/new,
 * imp/ = SDR_v2.srcs/sources_1/imports/new, gui.py = scripts/fft_analyzer_gui.py).
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures: device pointers are `void*`-compatible raw
 *     pointers (tensor.data_ptr()), the stream is a `void*` holding a hipStream_t
 *     (torch.cuda.current_stream().cuda_stream); NULL = the null stream.
 *   - every call returns 0 (SA_OK) or a negative SA_E* code; sa_last_error() gives the text.
 *     No exception or abort crosses the ABI.  There is NO CPU fallback: without a usable GPU
 *     sa_create() fails with SA_EHIP.
 *   - the library never allocates, frees or retains caller tensors.  It owns the opaque handle,
 *     its device-side tables and (for the Q15 IIR modes) a workspace sized by sa_reserve().
 *   - pointer contract of every process and filter call (sa_process_f32, _f32_i16, _f32_p12, sa_process_q15, _q15_out,
 *     _q15_p12, sa_filter_q15, _q15_p12): the kernels move 16 bytes per lane through the two pointers and declare both
 *     `__restrict__`, so
 *       alignment   `in` is 16-byte aligned: float32, int16, packed and hop streams alike (the rules stated below for
 *                   packed input and for sample streams are instances of this one).  `out` is 16-byte aligned for
 *                   SA_OUT_MAG_FULL, SA_OUT_TIME, SA_OUT_MARKER, SA_Q15_OUT_IQ, SA_Q15_OUT_MAG, SA_Q15_OUT_MARKER, every
 *                   SA_Q15_TRACE_KIND, every SA_Q15_TRACE_AVG_KIND and the output of sa_filter_q15*.  For the two half layouts `out` is aligned to its
 *                   element: 4 bytes for SA_OUT_MAG_HALF, 8 bytes for SA_OUT_SPEC_HALF -- their rows are 32 772 and 65 544
 *                   bytes long, so every row slice out[a : a + B] of such a tensor stays valid.  Anything else is SA_EINVAL;
 *                   the message names the entry point and which pointer is at fault.
 *       no overlap  the bytes the call reads, [in, in + in_bytes), and the bytes it writes, [out, out + out_bytes), must be
 *                   disjoint; otherwise the call returns SA_EINVAL, `out == in` included (no call works in place).
 *                   in_bytes is B * 65536 for float32, B * 32768 for int16 and B * 24576 for packed input; with a hop H it
 *                   is ((B - 1) * H + 16384) * 2 for int16 and three quarters of that for packed.  out_bytes follows the
 *                   tables of output kinds below (B rows of 65536, 32772, 65544, 65536, 16 bytes for SA_OUT_*; 65536,
 *                   65536, 16 for SA_Q15_OUT_*; 131072 >> k for SA_Q15_TRACE_KIND(k); 32768 for sa_filter_q15*;
 *                   B / A rows of 131072 >> k for SA_Q15_TRACE_AVG_KIND(k, a), A = 2^a).  Buffers
 *                   that merely touch (out == in + in_bytes, or the reverse) are accepted.
 *       a refusal   launches nothing and changes no call state: launch slot, overlap counter, profiling ring, the stream
 *                   the handle remembers and workspace growth all stay as they were, and the next call on the handle
 *                   behaves as if the refused one had not been made.
 *       order       these checks come after the NULL-tensor check; an empty batch returns SA_OK before any pointer is
 *                   looked at.  sa_debug_check_pointers() below is the same rule without a handle.
 *   - a handle is not thread-safe; use one handle per (GPU, stream) -- different handles may be
 *     used from different host threads at the same time (one thread per GPU).
 *     Process calls are asynchronous on the given stream; mode / coefficient / window changes are
 *     stream-ordered: they apply to every process call issued after them and to none issued
 *     before.  No call after sa_create() synchronises the device: table uploads run on the
 *     handle's own control stream behind an event, so other handles and streams are not stalled
 *     (a window or coefficient upload may block the HOST briefly when more than four uploads are
 *     still waiting for their copies; a Q15 workspace that is outgrown is kept until sa_destroy()
 *     rather than freed, because hipFree synchronises the device).
 *   - device: a handle belongs to the GPU given to sa_create().  Every call that touches the GPU makes that
 *     device the calling thread's current HIP device (hipSetDevice) and leaves it so; the stream and the
 *     pointers passed to a process call must belong to it (not checked: a check costs more than a launch).
 *     One process per GPU (torch.distributed ranks) or one host thread per GPU both work.
 *   - stream lifetime: the library uses the stream passed to a process call only inside that call.
 *     The caller may destroy it afterwards, in any order with later calls and sa_destroy(): uploads,
 *     stream switches and sa_destroy() order themselves behind an event the handle owns, bound to
 *     the completion of the call's last kernel.
 *   - hipGraph capture: process calls are capturable in ordered mode once sa_reserve() has sized
 *     the workspace.  A captured call freezes the control state of capture time in its kernel
 *     arguments; control-plane calls are refused (SA_ESTATE, nothing changed) while that capture
 *     is open -- also when other, uncaptured calls have been made on other streams meanwhile -- and
 *     after any control-plane call graphs captured earlier must be captured again.  End a capture
 *     before destroying the capturing stream (the handle asks that stream whether it still captures).
 *     Work replayed from a graph is not tracked by the handle: order it yourself (e.g. synchronise
 *     the replay stream) before a control-plane call.
 *   - frame length is fixed: SA_N = 16384 samples (gui.py:43-44, imp/dsp_system_top.vhd:440,
 *     ip/xfft_0/xfft_0.xci:12).
 *   - frames are isolated: a frame's outputs depend only on that frame and the control state of
 *     its call, not on the other frames of the batch or on anything run earlier on the GPU.  A NaN,
 *     an Inf or a sample whose spectrum overflows float32 affects only its own frame's outputs
 *     (whose values, and marker record, are then unspecified).
 */
#ifndef SPECAN_H_
#define SPECAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_N 16384
#define SA_FRAME_BYTES 65536          /* gui.py:42  FRAME_SIZE_BYTES */
#define SA_ABI_VERSION 4

/* error codes */
#define SA_OK       0
#define SA_EINVAL  -1   /* bad argument (NULL pointer, bad enum, bad section count) */
#define SA_ESHAPE  -2   /* bad batch / shape */
#define SA_EHIP    -3   /* HIP runtime error; text in sa_last_error() */
#define SA_ESTATE  -4   /* call not valid in the current state (e.g. mode needs coefficients) */
#define SA_ENOMEM  -5

/* filter-select command bytes: gui.py:35-37, decoded in new/command_control.vhd:53-58.
 * Power-on / reset value is SA_FILTER_NONE (new/command_control.vhd:31). */
#define SA_FILTER_DEFAULT 0x00   /* fixed ALPHA/BETA cascade, imp/filter_iir12.vhd + imp/filter_pkg.vhd:54-68 */
#define SA_FILTER_CUSTOM  0xA1   /* uploaded coefficients, new/filter_iir12_cust.vhd */
#define SA_FILTER_NONE    0xB1   /* window -> FFT directly */
#define SA_FILTER_WIDE    0xA2   /* build extension (not a reference byte): 6 independent Q2.14 sections */

/* other command bytes understood by sa_feed_command_bytes(): gui.py:28-33 */
#define SA_CMD_START          0x55
#define SA_CMD_UART_REQUEST   0xA5
#define SA_CMD_RESET          0xFF
#define SA_CMD_ETHERNET_MODE  0xEF
#define SA_CMD_UART_MODE      0xFE
#define SA_CMD_FILTER_UPDATE  0xF1   /* followed by 12 coefficient bytes, new/rx_filter_coeff.vhd:45-56 */

/* Q15 window modes */
#define SA_WIN_RTL_SIGNED 0   /* new/hann8192.vhd:36-39: ROM word used as signed Q15 (FPGA-exact) */
#define SA_WIN_HANN_U16   1   /* ROM + 32768 as unsigned Q16 Hann (the evident intent) */

/* float output layouts for sa_process_f32() */
#define SA_OUT_MAG_FULL   0   /* float  [B,16384]   |X[k]|, all N bins (upper half mirrored; gui.py:294-305 plots all N) */
#define SA_OUT_MAG_HALF   1   /* float  [B,8193]    |X[k]|, k = 0..N/2 */
#define SA_OUT_SPEC_HALF  2   /* float2 [B,8193]    X[k] = (re,im), k = 0..N/2 (numpy.fft.rfft layout) */
#define SA_OUT_TIME       3   /* float  [B,16384]   FFT input: window (+ IIR) output time series */
#define SA_OUT_MARKER     4   /* sa_marker [B]: per-frame peak search + band power over the marker range */

/* SA_OUT_MARKER record: what scripts/fft_analyzer_gui.py computes for every frame it shows -- the magnitude spectrum
 * cut to the user's range (get_frequency_range_data, gui.py:294-305), then np.max / np.argmax over that slice
 * (emit_plot_data, gui.py:415-455) -- made on the device in the chain's epilogue: 16 bytes per frame instead of a
 * 64 KiB spectrum that the host would copy back and search.
 *   - bins: k indexes the full N = 16384-bin spectrum exactly as SA_OUT_MAG_FULL lays it out (gui.py numbers them so);
 *     bins above 8192 hold the mirrored |X[N-k]|.  A range inside the upper half reports an upper-half bin.
 *   - peak_mag is bit for bit the value SA_OUT_MAG_FULL writes at peak_bin, and peak_bin the LOWEST k in [lo, hi)
 *     attaining it: numpy.argmax on the MAG_FULL row slice, plus lo.  (gui.py's own 'peak_bin' is that argmax, relative
 *     to the slice.)  The mirror is a bit-identical tie, so a full-range peak on a tone at bin b reports b, not N-b.
 *   - band_power is the sum over k in [lo, hi) of |X[k]|^2 as the kernel forms it (R^2 + I^2, before the square root),
 *     summed in float32 in a fixed order: the record is bit-reproducible from run to run (no atomics).
 *   - frames with a non-finite sample give unspecified records.
 *   - `out` of SA_OUT_MARKER must be 16-byte aligned (SA_EINVAL otherwise). */
typedef struct sa_marker {
    float    peak_mag;    /* max |X[k]| over k in [lo, hi) */
    int32_t  peak_bin;    /* lowest k in [lo, hi) attaining it */
    float    band_power;  /* sum over k in [lo, hi) of |X[k]|^2 */
    uint32_t reserved;    /* written as 0 */
} sa_marker;              /* 16 bytes; one aligned store per frame */

/* output layouts for sa_process_q15_out(): three views of the integer chain's frame, each defined bit for bit */
#define SA_Q15_OUT_IQ      0   /* int16 [B,16384,2]  the 65536-byte wire frame: what sa_process_q15 writes */
#define SA_Q15_OUT_MAG     1   /* float [B,16384]    decode_mag_16iq_le of that frame (gui.py:250-260), bit for bit */
#define SA_Q15_OUT_MARKER  2   /* sa_marker_q15 [B]  peak search + band power of that decode over the marker range */

/* SA_Q15_OUT_MAG is DEFINED as the float32 evaluation gui.py:250-260 makes of the frame,
 *     np.sqrt(re.astype(np.float32)**2 + im.astype(np.float32)**2):
 * r = (float)re, i = (float)im, p = fl(r*r), q = fl(i*i), s = fl(p + q), mag = the correctly rounded sqrt(s); each of the
 * four operations rounds to float32 on its own (no fused multiply-add: |re| or |im| above 4096 has an inexact square).
 * All N bins, as gui.py:294-305 plots them.  re = im = -32768 is reachable: re^2 + im^2 goes up to 2^31.
 *
 * SA_Q15_OUT_MARKER record: what gui.py computes from that decode for every frame it shows -- the slice to the user's
 * range (get_frequency_range_data, gui.py:294-305), then np.max / np.argmax (emit_plot_data, gui.py:415-455; the peak
 * markers of gui.py:691-712) -- made in the FFT kernel's epilogue with no spectrum stored: 16 bytes per frame.
 *   - peak_mag is bit for bit the SA_Q15_OUT_MAG value at peak_bin, and peak_bin the LOWEST k in [lo, hi) attaining it:
 *     numpy.argmax on the MAG row slice, plus lo.  The comparison is on the float magnitudes, not on the integers
 *     re^2 + im^2: two bins with different integer powers can round to one float, and the lower bin is reported.
 *     Unlike the float chain, the mirror bin N-k is NOT always a bit-identical tie here (the per-stage truncation of
 *     SA-FXFFT-1 breaks the symmetry), so a full-range record may name N-b for a tone at b -- as numpy does on the frame.
 *   - band_power is the sum over k in [lo, hi) of re[k]^2 + im[k]^2 as an exact integer (at most 16384 x 2^31 = 2^45):
 *     order-free, so the record is bit-reproducible with no rule about the summation order.  No atomics.
 *   - an all-zero frame gives (+0.0f, lo, 0).
 *   - `out` of SA_Q15_OUT_MARKER must be 16-byte aligned (SA_EINVAL otherwise). */
typedef struct sa_marker_q15 {
    float    peak_mag;    /* max over k in [lo, hi) of the SA_Q15_OUT_MAG value */
    int32_t  peak_bin;    /* lowest k in [lo, hi) attaining it */
    uint64_t band_power;  /* sum over k in [lo, hi) of re[k]^2 + im[k]^2, exact */
} sa_marker_q15;          /* 16 bytes; one aligned store per frame */

/* A fourth family of output kinds of sa_process_q15_out() and sa_process_q15_p12(): the display trace (build extension; ABI
 * version 4, added compatibly).  The bucket width travels inside the kind -- SA_Q15_TRACE_KIND(k) = 0x10 | k = 17..22 for
 * W = 2^k = 2..64 bins -- so there is no control state to set and nothing a captured graph could freeze.  A display has
 * about a thousand columns; gui.py:294-305, 415-455 ship all 16384 magnitudes of a frame to one.  An analyser's detector
 * reduces the bins that fall into a column before they leave the instrument, and this kind is that detector, made in the
 * FFT kernel's epilogue with no spectrum stored: P = 16384 / W records of 8 bytes per frame (8 KiB at W = 16) instead of
 * 64 KiB.
 *   - `out` is sa_trace_point_q15 [B, P]; point j covers the bins [jW, (j+1)W) of the full N-bin spectrum as
 *     SA_Q15_OUT_MAG lays it out.  Always the whole spectrum: the handle's marker range has no part in it.
 *   - peak_mag is the maximum of the SA_Q15_OUT_MAG values of the bucket, bit for bit (the positive-peak detector).  The
 *     correctly rounded root is monotone, so this is the root of the bucket's largest s = fl(fl(r*r) + fl(i*i)).
 *   - power is the float32 nearest (ties to even) to the EXACT integer sum over the bucket of re^2 + im^2 (at most
 *     64 x 2^31 = 2^37): one rounding of an exact sum, not a float accumulation, so it is order-free and bit-reproducible
 *     (the sample detector's power, or the RMS detector's after a division by W and a root on the host).
 *   - an all-zero frame gives (+0.0f, +0.0f) in every point.
 *   - `out` must be 16-byte aligned; SA_Q15_TRACE_KIND(0), SA_Q15_TRACE_KIND(7) and every other value outside the kinds
 *     listed here are SA_EINVAL.  The float entry points refuse these values: they are kinds of the Q15 chain alone. */
#define SA_Q15_TRACE_KIND(log2w) (0x10 | (log2w))
#define SA_Q15_TRACE_LOG2W_MIN 1
#define SA_Q15_TRACE_LOG2W_MAX 6
typedef struct sa_trace_point_q15 {
    float peak_mag;       /* max over the bucket of the SA_Q15_OUT_MAG value */
    float power;          /* the exact sum over the bucket of re[k]^2 + im[k]^2, rounded once to float32 */
} sa_trace_point_q15;     /* 8 bytes; one store per bucket */

/* A fifth family of output kinds of sa_process_q15_out() and sa_process_q15_p12(): the display trace reduced over groups of
 * A = 2^a consecutive frames as well as over buckets of W = 2^k bins -- max hold and summed power across sweeps, made before
 * the data leaves the device (build extension; ABI version 4, added compatibly: no new function).
 *     SA_Q15_TRACE_AVG_KIND(log2w, log2a) = 0x80 | (log2a) << 3 | (log2w)
 *         log2w = 1..6  (W = 2..64 bins, as SA_Q15_TRACE_KIND)
 *         log2a = 1..7  (A = 2..128 frames)
 * Values run from 0x89 to 0xBE.  The kind sits in the low byte of the kind word, so it combines with SA_Q15_HOP_KIND as the
 * trace kinds do.  One record covers W bins x A frames: 512 bytes per input frame at W = 16, A = 16, against 8 KiB.
 *   - `batch` must be a multiple of A, SA_ESHAPE otherwise: checked after the kind and before the pointers, with nothing
 *     launched and no call state.  batch == 0 is SA_OK.
 *   - `out` is sa_trace_point_q15 [B / A, P], P = 16384 / W, 16-byte aligned; the call writes (B / A) * P * 8 bytes, and the
 *     pointer contract is decided on that count.
 *   - record (g, j) covers the bins [jW, (j+1)W) of the frames gA .. gA + A - 1; with a hop these are the frames of the
 *     stream as SA_Q15_HOP_KIND numbers them.
 *   - peak_mag is the maximum over the A frames of the SA_Q15_TRACE_KIND(log2w) peak of the same bucket, bit for bit: the
 *     max-hold detector.  The correctly rounded root is monotone, so it is the root of the largest s of the W x A bins.
 *   - power is the float32 nearest (ties to even) to the EXACT integer sum of re^2 + im^2 over the W x A bins (at most
 *     128 x 64 x 2^31 = 2^44): one rounding of an exact sum.  It is the SUM, not the mean: A is a power of two, so the mean
 *     is power / A exactly (short of underflow, which an integer sum cannot reach).
 *   - a group of all-zero frames gives (+0.0f, +0.0f) in every point; the marker range plays no part.
 *   - SA_EINVAL: log2a = 0 (0x81..0x86), log2w = 0 or 7, any word with bit 6 set, and any of these words on a float
 *     entry point.  Every value refused before stays refused.
 *   - everything said of sa_process_q15_out holds: all four filter modes, both window modes, custom ROMs, int16 and packed
 *     input, hop streams, every overlap depth, and launch timing (one device time per call, from the call's first launch to
 *     its last: the FFT launch leaves one 16-byte partial record per bucket and frame in a workspace of the handle, and a
 *     second launch folds each group of A of them).
 *   - capture into a graph has one difference: that workspace, B * P * 16 bytes per launch slot, is grown on demand only
 *     (sa_reserve(max_batch) does not know W and allocates nothing for a kind the handle may never use).  A captured call
 *     whose workspace is too small is SA_ESTATE with nothing launched: make one call of that kind and size outside the
 *     capture first.  Once grown, the call captures and replays like any other.
 * Known answers: SA_Q15_TRACE_AVG_KIND(1,1) = 0x89; (4,3) = 0x9C; (6,7) = 0xBE;
 * SA_Q15_HOP_KIND(SA_Q15_TRACE_AVG_KIND(4,3), 4096) = 0x2009C. */
#define SA_Q15_TRACE_AVG_KIND(log2w, log2a) (0x80 | (log2a) << 3 | (log2w))
#define SA_Q15_TRACE_LOG2A_MIN 1
#define SA_Q15_TRACE_LOG2A_MAX 7
#define SA_Q15_TRACE_AVG_LOG2W(kind) ((kind) & 7)
#define SA_Q15_TRACE_AVG_LOG2A(kind) ((kind) >> 3 & 7)
/* non-zero iff `kind`, the low byte of a kind word, is a SA_Q15_TRACE_AVG_KIND with both fields in their ranges */
#define SA_Q15_IS_TRACE_AVG_KIND(kind)                                                                       \
    (((kind) & ~0x3F) == 0x80 && SA_Q15_TRACE_AVG_LOG2W(kind) >= SA_Q15_TRACE_LOG2W_MIN &&                    \
     SA_Q15_TRACE_AVG_LOG2W(kind) <= SA_Q15_TRACE_LOG2W_MAX && SA_Q15_TRACE_AVG_LOG2A(kind) >= SA_Q15_TRACE_LOG2A_MIN)

/* precision of the float path's window and cascade (sa_set_precision) */
#define SA_PRECISION_F32       0   /* default: float32 arithmetic throughout, one fused kernel per call */
#define SA_PRECISION_F64_STATE 1   /* window, inter-section signal and DF2T recursion in float64; FFT in float32 */

typedef struct sa_handle sa_handle;

/* ---- lifetime ------------------------------------------------------------------------- */
/* Stands for "power on the board": state = filter NONE, zero custom coefficients
 * (new/filter_iir12_cust.vhd:51-52), default Hann ROM (new/hann.vhd, scripts/hann_coeff.py:3-5). */
int sa_create(int device, sa_handle **out);
int sa_destroy(sa_handle *h);
int sa_abi_version(void);
const char *sa_last_error(const sa_handle *h);   /* h may be NULL: last sa_create() failure */

/* Pre-size the internal workspace for batches up to max_batch frames (Q15 IIR modes need
 * B*32 KiB, per launch slot in overlap mode).  Optional: process calls grow it on demand (not
 * capturable into a hipGraph then). */
int sa_reserve(sa_handle *h, int max_batch);

/* Overlapped launches (opt-in; build extension).  Frames are independent -- every frame starts from a zero
 * filter state: the RTL clears the biquad history whenever i_valid = '0' (new/filter_iir_cust.vhd:142-146,
 * SURVEY quirk Q5), which this build applies once per frame -- so consecutive batches need not
 * run one after the other.  With depth d > 1, process call k runs on an internal stream of the
 * handle (k mod d), ordered after everything the caller's stream held when the call was made but
 * NOT after calls k-1 .. k-d+1: the tail of one launch runs under the head of the next (on the
 * Q15 path the FFT of batch k-1 under the filter of batch k).  Contract in this mode:
 *   - the results of call k are visible to work enqueued on the caller's stream after call
 *     k+d-1 has been made, or after sa_flush(); until then the call's input AND output tensors
 *     must not be written, freed or read by the caller;
 *   - process calls cannot be captured into a hipGraph (SA_ESTATE);
 *   - control-plane calls stay stream-ordered: they apply to all later calls and to no earlier one.
 * depth = 1 (the default) is the strictly stream-ordered mode described above.  sa_set_overlap()
 * waits on the host for the handle's own outstanding work when the depth changes.
 * The internal streams are chosen so that they execute side by side with each other AND with the caller's stream:
 * the runtime maps streams onto a few hardware queues and two streams on one queue run in order (a handle with
 * such a pair was slower in overlap mode than without it).  The mapping is not exposed, so the library probes
 * candidate streams with a 100 us one-wave kernel: in sa_set_overlap() among themselves, and in the FIRST
 * overlapped process call made from a given caller stream against that stream -- that one call waits on the host
 * for the stream's earlier work and takes about a millisecond longer.  Best effort on a GPU busy with other work.
 * The handle remembers ONE fitted caller stream (it is compared, never dereferenced: the caller may have destroyed it):
 * overlapped calls that alternate between caller streams re-run the probe at every change -- keep a handle on one
 * caller stream, as the one-handle-per-(GPU, stream) rule above says. */
int sa_set_overlap(sa_handle *h, int depth /* 1..4 */);
int sa_get_overlap(const sa_handle *h, int *depth);
/* Introspection for tests: re-runs that probe on the handle's internal streams and `stream`;
 * *side_by_side = 1 if every pair overlaps. */
int sa_debug_overlap_streams(sa_handle *h, void *stream, int *side_by_side);
/* Make `stream` wait for every outstanding overlapped call of the handle (no host wait). */
int sa_flush(sa_handle *h, void *stream);

/* Launch timing (opt-in; measurement aid, no counterpart in the reference).  With ring = n > 0 every stream-ordered
 * process call binds a pair of timing events to the BEGIN of its first kernel and the END of its last one -- the
 * events ride on the dispatch packets themselves (hipExtLaunchKernel), nothing is put between two launches, so a train
 * of calls runs as it does untimed -- and the handle keeps the pairs of the last n calls.  sa_profile_read() waits on
 * the host for those calls and writes their device times in milliseconds, oldest first, into ms[0 .. return value)
 * (at most cap).  A call with one kernel (the float chain, the bypassed integer chain) reports that kernel's duration;
 * the integer chain with a cascade reports cascade + FFT including the gap between them.  Captured calls are not
 * timed.  ring = 0 turns it off.  Refused (SA_ESTATE) while sa_set_overlap is above 1, and sa_set_overlap(d > 1) is
 * refused while it is on: kernels that run beside each other have no per-call time.  Changing the ring waits on the
 * host for the handle's own outstanding work. */
int sa_set_profiling(sa_handle *h, int ring /* 0..65536 */);
int sa_profile_read(sa_handle *h, float *ms, int cap);

/* ---- control plane of the path (what the UART bytes do) -------------------------------- */
/* new/command_control.vhd:53-58: accepts SA_FILTER_DEFAULT / CUSTOM / NONE (and SA_FILTER_WIDE). */
int sa_set_filter_mode(sa_handle *h, uint8_t cmd);
int sa_get_filter_mode(const sa_handle *h, uint8_t *cmd);

/* 12 int8 coefficients in wire order [b0,b1,b2,a0,a1,a2] x 2 (gui.py:598-605), stored into
 * COEFF_IIR_CF(0..11) (new/filter_iir12_cust.vhd:54, ports :83-94).  Semantics per the RTL:
 * stage taps B2*x[n]+B1*x[n-1]+B0*x[n-2]-A0*y[n-2]-A1*y[n-1], each product >>7, 16-bit wrap;
 * set 0 drives stages 1,3,5 and set 1 stages 2,4,6; A2 is unused (new/filter_iir_cust.vhd:96-117).
 * The float path (sa_process_f32) uses the same taps as real numbers c/128. */
int sa_load_coeffs_q7(sa_handle *h, const int8_t c[12]);
int sa_get_coeffs_q7(const sa_handle *h, int8_t c[12]);

/* Byte-stream front door: the UART RX path (imp/uart_rx.vhd -> new/rx_filter_coeff.vhd:41-66
 * + new/command_control.vhd:51-62).  0xF1 starts a 12-byte coefficient upload during which no
 * byte is interpreted as a command; 0x00/0xA1/0xB1 select the filter; 0xFF resets (filter NONE,
 * coefficients cleared); 0x55/0xA5/0xEF/0xFE are accepted and counted but have no effect on the
 * signal path.  Unknown bytes are ignored, like the RTL.  *n_frames_requested (optional) is
 * incremented once per 0xA5 seen outside a coefficient upload: the UART read request of
 * imp/sequ2.vhd:216 (0x55 only starts the acquisition, new/command_control.vhd:58-60, and is
 * reported by sa_feed_command_bytes_ex). */
int sa_feed_command_bytes(sa_handle *h, const uint8_t *bytes, size_t n, int *n_frames_requested);

/* The same front door with everything a transport shim needs to stand where imp/sequ2.vhd stands.
 * Counters are ADDED to (zero the struct first); `transport` and `control_changed` are set. */
typedef struct sa_cmd_events {
    int n_start;          /* 0x55: start_aq pulse (new/command_control.vhd:58-60, :75) */
    int n_uart_request;   /* 0xA5: UART read command (imp/sequ2.vhd:216) */
    int n_reset;          /* 0xFF: reset_n pulse (new/command_control.vhd:56-57) */
    int n_uploads;        /* completed 0xF1 + 12-byte coefficient uploads (new/rx_filter_coeff.vhd:45-56) */
    int control_changed;  /* non-zero: filter select, coefficients or a reset changed what the path computes */
    uint8_t transport;    /* SA_CMD_ETHERNET_MODE or SA_CMD_UART_MODE after the last byte (imp/sequ2.vhd:82-96);
                             reset selects Ethernet (imp/sequ2.vhd:85-86) */
} sa_cmd_events;
int sa_feed_command_bytes_ex(sa_handle *h, const uint8_t *bytes, size_t n, sa_cmd_events *ev);
int sa_get_transport(const sa_handle *h, uint8_t *cmd);

/* North-star wide formats (not in the reference): up to 6 independent sections, scipy row order
 * [b0,b1,b2,a0,a1,a2], normalised by a0 on load.  f32/f64 feed sa_process_f32 in CUSTOM mode;
 * q14 (int16 Q2.14, a0 ignored) feeds sa_process_q15 in WIDE mode. */
int sa_load_sos_f32(sa_handle *h, const float *sos, int n_sections);
int sa_load_sos_f64(sa_handle *h, const double *sos, int n_sections);
int sa_load_sos_q14(sa_handle *h, const int16_t *sos, int n_sections);

/* Window tables (host pointers, copied).  NULL restores the default generated with the formula of
 * scripts/hann_coeff.py:3-5 (the Q15 table includes the int16 wrap of entries 8178..8205).
 *
 * A float table that is a two-term cosine window, w[n] = a0 - a1 cos(2 pi n / 16383) to within 1.5e-7 of its peak
 * (a0, a1 fitted by least squares in double: Hann, Hamming, ...; the default is one, with a0 = a1 = 0.5 exactly), is
 * replaced by that formula in the kernels that compute a spectrum behind an IIR cascade (filter modes DEFAULT and CUSTOM)
 * in the float32 precision: they evaluate it in place in float32 by the angle-addition formula, two fused multiply-adds
 * per sample, and do not read the table.  The window they apply differs from the loaded table by at most
 *     A(w) = 1.5e-7 + 5 * 2^-24 * (|a0| + |a1|) / peak      (4.5e-7 for Hann)
 * of the table's peak: the fit's threshold plus five float32 roundings.  The bound is absolute, not relative: near a
 * zero of the window (Hann at n = 1 is 3.7e-8) the generated value is off by more than the table entry itself.  Any
 * other table is applied as loaded.  Bypass mode (NONE), SA_OUT_TIME and SA_PRECISION_F64_STATE always apply the table
 * itself (float32 x * w rounded once; in the float64-state precision the table widened exactly, in double). */
int sa_set_window_q15(sa_handle *h, const int16_t *w /* [16384] or NULL */);
int sa_set_window_f32(sa_handle *h, const float *w /* [16384] or NULL */);
int sa_set_window_mode_q15(sa_handle *h, int mode /* SA_WIN_* */);
int sa_get_window_q15(const sa_handle *h, int16_t *w /* [16384] */);

/* ---- data plane ----------------------------------------------------------------------- */
/* Q15 path, bit-exact integer pipeline: in [B,16384] int16 device (samples as the XADC delivers
 * them, imp/dsp_system_top.vhd:435) -> out_iq [B,16384,2] int16 device = the 65536-byte frames of
 * imp/sequ2.vhd:153 / gui.py:250-260 (re lo,hi, im lo,hi).  FFT = SA-FXFFT-1:
 * stands where ip/xfft_0 stands; 1/N scaling, truncation. */
int sa_process_q15(sa_handle *h, const int16_t *in, int16_t *out_iq, int batch, void *stream);

/* The same chain with the host's first steps on the frame made in the FFT kernel's epilogue (build extension): `out` per
 * out_kind (SA_Q15_OUT_*, above).  SA_Q15_OUT_IQ is sa_process_q15() itself; SA_Q15_OUT_MAG replaces decode_mag_16iq_le
 * (gui.py:250-260) on the host, SA_Q15_OUT_MARKER the range slice and np.max / np.argmax on top (gui.py:294-305, 415-455,
 * 691-712), 16 bytes per frame instead of 64 KiB.  Everything sa_process_q15() does holds for every kind: all four filter
 * modes, both window modes, custom ROMs, every overlap depth, launch timing, hipGraph capture once sa_reserve() has
 * sized the workspace.  SA_EINVAL for an unknown kind, a NULL tensor or a marker `out` that is not 16-byte aligned (an
 * instance of the pointer contract at the top of this file, which holds for every kind): nothing is launched and no call
 * state changes.  out_kind may also be SA_Q15_TRACE_KIND(k), k = 1..6 (above): one
 * sa_trace_point_q15 per bucket of 2^k bins, under the same rules, its `out` 16-byte aligned as well. */
int sa_process_q15_out(sa_handle *h, const int16_t *in, void *out, int batch, int out_kind, void *stream);

/* Window (+ integer IIR) only: the FFT input stream, [B,16384] int16 (fft_in16 of
 * new/command_control.vhd:90-123). */
int sa_filter_q15(sa_handle *h, const int16_t *in, int16_t *out_time, int batch, void *stream);

/* float path: in [B,16384] float32 device -> out per out_kind (SA_OUT_*), device.
 * Accuracy against the float64 oracle |rfft(sosfilt(sos, x*window))| (scipy / numpy), in ONE norm throughout: the
 * max-norm error of the magnitude spectrum of a frame relative to that spectrum's peak.
 * In the default precision (SA_PRECISION_F32) within 1e-5 wherever float32 arithmetic itself allows it: every fixture,
 * the headline 12th-order Butterworth (worst of 4096 frames 1.9e-6), 4412 of 4500 random designs (tests/fuzz_parity.py,
 * seeds 7 / 11 / 23 x 1500).  For filters whose poles sit next to the unit circle, or whose output is stop-band leakage
 * far below the input, float32 runs out: a SEQUENTIAL float32 evaluation of sosfilt's own recurrence is above 1e-5 in
 * this norm for 237 of the same 4500 designs, this path for 88 (worst 6.5e-4; two of them more than 4x the sequential
 * figure, one 15.6x -- restarting the float32 recursion from EXACT chunk start states gives the same error, so no
 * float64 predictor or scan alone helps; tools/accuracy_study.py).  tests/test_gpu_f32.py::test_random_designs pins
 * that behaviour.  Callers that need 1e-5 on such designs select SA_PRECISION_F64_STATE (sa_set_precision below).
 * The path is linear: an input scaled by 2^k gives SA_OUT_SPEC_HALF and SA_OUT_TIME scaled by exactly 2^k, bit for bit, and
 * magnitudes within 1 ulp, while every intermediate stays a normal float32 -- |X|^2 is formed in float32, so every
 * nonzero bin needs roughly 1e-19 < |X| < 1.8e19, and no nonzero sample, state or product may fall below 1.2e-38
 * (tests/test_gpu_f32_structured.py::test_power_of_two_scaling_is_exact). */
int sa_process_f32(sa_handle *h, const float *in, void *out, int batch, int out_kind, void *stream);

/* The float path fed with the ADC's samples (build extension): in [B,16384] int16 device -- the board delivers
 * 12-bit samples sign-extended to int16 (imp/dsp_system_top.vhd:435) and that is what the ingest front-end moves over
 * PCIe.  x = (float)sample * scale is rounded once in the stage-in (scale = 1/2048 maps the ADC range to [-1, 1)) and
 * then takes exactly the float32 path: the results are those of sa_process_f32() on the converted frames, bit for bit,
 * without the conversion pass and with half the input bytes (32 KiB per frame, one fetch round instead of two). */
int sa_process_f32_i16(sa_handle *h, const int16_t *in, float scale, void *out, int batch, int out_kind, void *stream);

/* The float path fed with packed 12-bit samples ("p12", build extension; ABI version 4, added compatibly).  The ADC's
 * samples are 12 bits wide -- imp/dsp_system_top.vhd:435 sign-extends adc_out(15 downto 4) -- so in int16 a quarter of
 * every byte on the link is sign extension; digitisers and capture files commonly pack two samples into three bytes.
 * The format:
 *   - a frame is SA_P12_FRAME_BYTES = 24576 bytes, a batch a contiguous [B,24576] uint8 array;
 *   - sample n of a frame (s_n in [-2048, 2047], u_n = s_n & 0xFFF) occupies bits [12n, 12n+12) of the frame read as a
 *     little-endian bit stream; for each pair i
 *         b[3i]   = u_{2i} & 0xFF
 *         b[3i+1] = (u_{2i} >> 8) | ((u_{2i+1} & 0xF) << 4)
 *         b[3i+2] = u_{2i+1} >> 4
 *   - known answers: samples [0x123, 0x456] pack to bytes 23 61 45; samples [-1, -2048] to bytes FF 0F 80;
 *   - every bit pattern is a valid frame.
 * x = (float)s_n * scale is rounded once in the stage-in and then takes exactly the float32 path: the results are those
 * of sa_process_f32_i16() on the sign-extended samples, bit for bit, for every output kind, filter mode and precision,
 * with no unpack pass, no workspace and no extra launch (24 KiB of input per frame instead of 32).  Everything said of
 * sa_process_f32_i16 holds, and one more argument check: `in` must be 16-byte aligned (SA_EINVAL otherwise, nothing is
 * launched; the stage-in issues 16-byte requests, and the frame stride of 24576 keeps every frame aligned). */
#define SA_P12_FRAME_BYTES 24576
int sa_process_f32_p12(sa_handle *h, const uint8_t *in /* [B,24576] device */, float scale, void *out, int batch,
                       int out_kind, void *stream);

/* The Q15 path fed with packed 12-bit samples (build extension; ABI version 4, added compatibly).  The integer chain is the
 * FPGA-exact mode, and its real input is exactly that 12-bit stream: imp/dsp_system_top.vhd:435 sign-extends
 * adc_out(15 downto 4) into the 16-bit sample the window takes (new/hann8192.vhd:36-39).  `in` is the p12 format defined
 * above, [B,24576] uint8, 16-byte aligned (SA_EINVAL otherwise: the rule of sa_process_f32_p12).
 *   sa_process_q15_p12: `out` per out_kind (SA_Q15_OUT_IQ, SA_Q15_OUT_MAG, SA_Q15_OUT_MARKER or SA_Q15_TRACE_KIND(k)) -- the results of
 *     sa_process_q15_out() (imp/sequ2.vhd:153 frames, gui.py:250-260 magnitudes, gui.py:294-305 / 691-712 markers) on
 *     sa_unpack_samples_p12(in), bit for bit;
 *   sa_filter_q15_p12: the FFT input stream (fft_in16 of new/command_control.vhd:90-123) -- the results of sa_filter_q15()
 *     on the same samples, bit for bit.
 * The samples are unpacked inside the kernels that read them (the window kernel, the cascades' staging waves, stage 0 of
 * the FFT in filter mode 0xB1): no unpack pass, no workspace of their own, no extra launch, 24 KiB of input per frame
 * instead of 32, and no byte outside [in, in + batch * 24576) is read.  Everything said of sa_process_q15_out() holds: all
 * four filter modes (0xA2 with no sections included), both window modes, custom ROMs, every overlap depth (the ordering of
 * the wide cascade at depth 2 included), launch timing, hipGraph capture once sa_reserve() has sized the workspace, and its
 * argument checks, made before any call state changes: SA_EINVAL for an unknown kind, a NULL tensor, a marker `out` or an
 * `in` that is not 16-byte aligned, SA_ESHAPE for a negative batch; nothing is launched then. */
int sa_process_q15_p12(sa_handle *h, const uint8_t *in /* [B,24576] device */, void *out, int batch, int out_kind,
                       void *stream);
int sa_filter_q15_p12(sa_handle *h, const uint8_t *in /* [B,24576] device */, int16_t *out_time, int batch, void *stream);

/* Overlapping frames cut on the device from ONE sample stream (build extension; ABI version 4, added compatibly).  A
 * windowed analyser that must not lose signal between frames runs at hop = N/2 or N/4; cut on the host
 * (ingest.FrameCutter), every sample then crosses the link N/hop times.  Frames are independent (history is reset per
 * frame, the window is applied per frame), so frame b of a stream is simply the 16384 samples from sample b * hop on, and
 * the kernels that read samples address it there.  The hop travels inside the out_kind word of sa_process_q15_out() and
 * sa_process_q15_p12(), as the trace width does: no control state, nothing a captured graph could freeze.
 *     SA_Q15_HOP_KIND(kind, hop) = kind | (hop / 8) << 8
 *   bits 0..7    the kind as above: SA_Q15_OUT_IQ, _MAG, _MARKER, SA_Q15_TRACE_KIND(k) = 17..22 or
 *                SA_Q15_TRACE_AVG_KIND(k, a) = 0x89..0xBE
 *   bits 8..19   the hop field h = hop / 8
 *   bits 20..30  must be zero
 *   - h = 0 is every call described so far: `in` is [B,16384] (packed: [B,24576]), frames back to back.  Every out_kind that
 *     existed keeps its value, its meaning and its kernels.
 *   - h = 1..SA_Q15_HOP_FIELD_MAX (2048): hop = 8 h samples, a multiple of 8 in 8..16384.  `in` is ONE stream of
 *     (batch - 1) * hop + 16384 samples -- int16, or packed 12-bit at 3/2 bytes per sample (the p12 bit stream above, not
 *     cut into frames) -- and frame b is its samples [b hop, b hop + 16384).  `out` is what it is for frames: [B, ...]
 *     per kind, bit for bit the result of the plain call on the B frames copied out of the stream.  h = 2048 (hop = N)
 *     gives the bits of the plain call on the same memory.
 *   - `in` must be 16-byte aligned for both input forms (SA_EINVAL otherwise; the pointer contract at the top of this file,
 *     whose message names the sample stream when h > 0).  int16: every frame is then 16-byte
 *     aligned (16 h bytes apart), which the cascades' 16-byte tile loads need.  Packed: frame b begins at byte 12 h b -- on
 *     a dword, which is all the packed loads need, and deliberately NOT on 16 bytes.  No byte outside the stream is read:
 *     the last frame ends with it.
 *   - refused with SA_EINVAL before any call state changes, nothing launched: h above 2048, any of bits 20..30 set, a low
 *     byte that is not a kind of the entry point, a misaligned `in`.  The float entry points refuse every word with h > 0,
 *     as they refuse any unknown kind; sa_process_q15, sa_filter_q15 and sa_filter_q15_p12 have no kind word and take
 *     frames only.
 *   - everything said of sa_process_q15_out() holds: all four filter modes, both window modes, custom ROMs, every overlap
 *     depth, launch timing, hipGraph capture once sa_reserve() has sized the workspace (which is sized by B as ever: with
 *     a cascade, the cascade reads the stream and writes B frames into it; in mode 0xB1 the FFT's first stage reads the
 *     stream).
 *   - known answers: SA_Q15_HOP_KIND(SA_Q15_OUT_IQ, 8192) = 0x40000; SA_Q15_HOP_KIND(SA_Q15_OUT_MARKER, 4096) = 0x20002;
 *     SA_Q15_HOP_KIND(SA_Q15_TRACE_KIND(4), 8) = 0x114; SA_Q15_HOP_KIND(SA_Q15_OUT_MAG, 16384) = 0x80001.  A batch of
 *     B = 5 at hop 4096 is a stream of SA_Q15_HOP_STREAM_SAMPLES(5, 4096) = 32768 samples: 65536 bytes of int16 or 49152
 *     packed, against 163840 and 122880 for the five frames. */
#define SA_Q15_HOP_KIND(kind, hop) ((kind) | ((hop) / 8) << 8)
#define SA_Q15_HOP_FIELD_MAX 2048
#define SA_Q15_HOP_STREAM_SAMPLES(batch, hop) (((size_t)(batch) - 1) * (size_t)(hop) + SA_N)

/* Host helpers of the p12 format: pure functions, no handle, no GPU.  n is the number of SAMPLES and must be even
 * (SA_EINVAL otherwise); `packed` holds 3n/2 bytes.  Packing a sample outside [-2048, 2047] is SA_EINVAL and nothing
 * is written.  Unpacking sign-extends to int16. */
int sa_pack_samples_p12(const int16_t *samples, size_t n, uint8_t *packed /* 3n/2 bytes */);
int sa_unpack_samples_p12(const uint8_t *packed, size_t n, int16_t *samples);

/* Introspection for tests: the pointer contract of the process and filter calls (top of this file) as a pure function -- no
 * handle, no GPU, the addresses are compared as integers and never dereferenced.  `entry` names the entry point
 * (SA_ENTRY_*), `kind_word` is its out_kind argument, a SA_Q15_HOP_KIND word where the entry point takes one (ignored by the
 * entry points that have no out_kind).  SA_OK where the call would pass its pointer checks; SA_EINVAL for a misaligned
 * `in` or `out`, overlapping byte ranges, a zero address, an unknown entry or a kind word the entry point refuses; SA_ESHAPE
 * for a negative batch and for a batch that is no multiple of the A of a SA_Q15_TRACE_AVG_KIND (after the kind, before the
 * addresses); batch == 0 is SA_OK for any addresses.  The entry points themselves ask the same code. */
#define SA_ENTRY_PROCESS_F32      0
#define SA_ENTRY_PROCESS_F32_I16  1
#define SA_ENTRY_PROCESS_F32_P12  2
#define SA_ENTRY_PROCESS_Q15      3
#define SA_ENTRY_PROCESS_Q15_OUT  4
#define SA_ENTRY_PROCESS_Q15_P12  5
#define SA_ENTRY_FILTER_Q15       6
#define SA_ENTRY_FILTER_Q15_P12   7
#define SA_ENTRY_COUNT            8
int sa_debug_check_pointers(int entry, int kind_word, uint64_t in_addr, uint64_t out_addr, int batch);

/* Host helper: view of one frame as the byte stream sequ2 emits.  On little-endian hosts the
 * Q15 output already is that stream; this copies 65536 bytes and is provided for symmetry with
 * gui.py:250-260 (decode side). */
int sa_pack_frame(const int16_t *iq_host /* [16384,2] */, uint8_t *frame_bytes /* [65536] */);

/* Introspection for tests / tuning: the float IIR plan the kernels consume (chunked-scan form of
 * the cascade: per section 5 taps, predictor taps, state-transition powers).  Writes at most `cap`
 * floats, returns the count needed (or a negative error). */
int sa_debug_iir_plan_f32(const sa_handle *h, float *out, int cap);

/* Same plan computed on the host from an SOS (scipy row order, a0-normalised here), without a
 * handle or a GPU: pure host logic, used by the CPU tests to check the chunked-scan algebra. */
int sa_iir_plan_from_sos(const double *sos, int n_sections, float *out, int cap);

/* ---- float64-state IIR (opt-in; build extension) --------------------------------------------------------------------
 * sa_set_precision(h, SA_PRECISION_F64_STATE): sa_process_f32, _i16 and _p12 in filter modes DEFAULT and CUSTOM
 * evaluate the window (x * w in double, w = the default Hann of scripts/hann_coeff.py:3-4 in double, or the table of
 * sa_set_window_f32 widened exactly), the signal between sections and the DF2T recursion of scipy.signal.sosfilt in
 * float64, and round only the cascade output y to float32.  The FFT of y is the float32 one (its own error on a float32
 * y is ~1e-6).  Within 1e-5 of the oracle above on every design of tests/fuzz_parity.py (profiles/r5_fuzz_f64.txt).
 *   - a call is TWO kernels: the float64 cascade into a float32 workspace [B,16384] of the handle, then the bypassed
 *     float chain on it (SA_OUT_TIME: the first kernel alone, writing y to `out`).  Cost: about 2x the float32 call at
 *     B = 4096 (profiles/r5_f64_cost.txt), and one write and one read of 64 KiB per frame more HBM traffic.
 *   - the workspace is per launch slot, allocated only in this mode: sa_reserve() sizes it too while the handle is in
 *     this mode, sa_set_precision() sizes it to the largest batch reserved so far, and a process call grows it on
 *     demand (SA_ESTATE inside a stream capture, as for the Q15 workspace).  Overlap depths 1..4 work as in the default
 *     precision, each slot with its own workspace.  Launch timing reports one time per call, from the start of the
 *     first kernel to the end of the second.  Captured calls replay both kernels.
 *   - filter NONE (and a CUSTOM cascade of zero sections) keeps the single bypassed launch of the default precision,
 *     bit for bit; the Q15 path ignores the setting.
 *   - control-plane call: stream-ordered (applies to later process calls only), refused while a capture is open
 *     (SA_ESTATE), SA_EINVAL for any other value.  Leaving the mode keeps its device tables until sa_destroy(). */
int sa_set_precision(sa_handle *h, int precision /* SA_PRECISION_* */);
int sa_get_precision(const sa_handle *h, int *precision);

/* ---- marker range (SA_OUT_MARKER, SA_Q15_OUT_MARKER; build extension) ------------------------------------------------
 * The full-spectrum bins [lo, hi) the SA_OUT_MARKER records of sa_process_f32 / sa_process_f32_i16 and the
 * SA_Q15_OUT_MARKER records of sa_process_q15_out cover -- one range per handle for both chains: the gui's
 * frequency range (web_config freq_range_start / freq_range_end in per mille of the N bins, gui.py:294-305) as bin
 * indices.  [0, 16384) at sa_create(), the gui's default 0..1000 per mille.  0 <= lo < hi <= SA_N, else SA_EINVAL and
 * nothing changed.  Not board state: the 0xFF reset of sa_feed_command_bytes leaves it alone.
 *   - control-plane call with the rules of sa_set_precision: stream-ordered (applies to later process calls only),
 *     refused while a capture is open (SA_ESTATE).  No upload: the range travels by value in the kernel arguments,
 *     so a captured call keeps the range of its capture time.
 *   - SA_OUT_MARKER works in filter modes NONE, DEFAULT and CUSTOM, in both precisions (in SA_PRECISION_F64_STATE the
 *     float chain on the float64 cascade's output makes the records), at every overlap depth, with launch timing and
 *     under hipGraph capture.
 *   - SA_Q15_OUT_MARKER works in filter modes NONE, DEFAULT, CUSTOM and WIDE under the same rules: the range travels by
 *     value in the FFT launch's arguments (gui.py:294-305 slices the decoded frame with the very same indices). */
int sa_set_marker_range(sa_handle *h, int lo, int hi);
int sa_get_marker_range(const sa_handle *h, int *lo, int *hi);

/* The float64 plan (iir_f64.hip, struct SaIirF64): hdr[4] (hdr[0] = padded section count 0/2/4/6) then 6 sections of
 * {c[6] = b0,b1,b2,a1,a2,0; m[16][2] predictor taps A^(15-j) Bv; A^16; A^32; A^(64 * 2^k) k < 4; A^(1024 * 2^k) k < 4;
 * A^(64 i) i < 16}, every 2x2 matrix row-major, in the DF2T coordinates of sosfilt (A = [[-a1,1],[-a2,0]],
 * Bv = [b1 - a1 b0, b2 - a2 b0]).  Write at most `cap` doubles, return the count needed (or a negative error).
 * sa_debug_iir_plan_f64: the plan the handle would launch in its current filter mode (built from its double SOS);
 * sa_iir_plan_from_sos_f64: the same from an SOS (scipy row order, a0-normalised here), no handle or GPU needed. */
int sa_debug_iir_plan_f64(const sa_handle *h, double *out, int cap);
int sa_iir_plan_from_sos_f64(const double *sos, int n_sections, double *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SPECAN_H_ */
