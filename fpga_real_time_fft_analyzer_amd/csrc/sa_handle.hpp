// sa_handle.hpp -- the opaque handle of the C ABI, its error helpers, and what specan_abi.cpp (create / destroy, setters,
// process paths) calls in sa_streams.cpp (launch and upload ordering).  Host only: no kernel unit includes it.
#pragma once
#include "../../include/specan.h"
#include "sa_common.hpp"

#include <cstdio>
#include <string>
#include <vector>

struct sa_handle {
    int device = 0;
    std::string err;
    uint8_t filter_mode = SA_FILTER_NONE;
    int8_t c12_custom[12] = {0};
    int win_mode_q15 = SA_WIN_RTL_SIGNED;
    int16_t sos_q14[SA_MAXSEC * 6] = {0};
    int nsec_q14 = 0;
    // UART byte-stream state (new/rx_filter_coeff.vhd:41-66)
    int rx_count = -1;            // -1 = IDLE, 0..11 = ACQUIRE
    int8_t rx_buf[12] = {0};
    // host tables
    std::vector<int16_t> rom;
    // One float cascade: its a0-normalised SOS (kept to rebuild on window change), the float32 plan and its device lane
    // table, and the device float64-state plan (allocated by the first sa_set_precision(F64_STATE)).
    struct Plan {
        double sos[36] = {0};
        int nsec = 0;
        SaIirK k{};
        SaIirLaneTab lt{};
        SaIirLaneTab *d_lt = nullptr;
        SaIirF64 *d_p64 = nullptr;
    };
    Plan plan_default, plan_custom;        // the fixed ALPHA/BETA cascade; the loaded one
    std::vector<float> half_win;           // 0.5 * float window, natural order
    bool win_is_cos = true;                // the float window is a0 - a1 cos(2 pi n / (N-1)) (default: Hann)
    double win_cos[2] = {0.5, 0.5};
    // device tables
    float4 *d_win_b = nullptr;
    float4 *d_win_t = nullptr;
    float4 *d_twT = nullptr, *d_twB = nullptr;
    float2 *d_twC = nullptr;
    int16_t *d_rom = nullptr;
    uint2 *d_twq = nullptr;          // SA-FXFFT-1 twiddles, {(wr, wi), (-wi, wr)} packed int16 pairs
    uint4 *d_twrec = nullptr;        // the same words regrouped per butterfly for the per-lane stages (SaQ15Tables::twrec)
    // A launch slot's workspace of `elem`-byte samples.  A workspace that is outgrown is retired, not freed (hipFree
    // synchronises the whole device; launches in flight may still use it): freed in sa_destroy.  Growth is geometric
    // so that the retired total stays below the live one.
    struct Workspace {
        void *ptr;
        int frames;
        size_t elem;
    };
    enum { kWorkQ15, kWorkF64, kWorkTraceRaw, kWorkSpectra, kWorkKinds };
    // Launch slot i (slot 0 = ordered mode; overlap mode uses slots 0..depth-1): its workspaces -- the Q15 cascade's
    // int16 output, in float64-state mode the float32 y [B,16384], and the partial records of SA_Q15_TRACE_AVG_KIND (bytes,
    // counted in units of 16384: grown by the calls of that kind alone, never by sa_reserve or a change of mode), and the
    // int16 (re, im) frames of sa_spectra_q15 (include/specan_ext.h; 64 KiB per frame, grown by those calls alone too) -- and,
    // in overlap mode, its internal stream
    struct Slot {
        Workspace work[kWorkKinds] = {{nullptr, 0, sizeof(int16_t)}, {nullptr, 0, sizeof(float)}, {nullptr, 0, 1},
                                      {nullptr, 0, 2 * sizeof(int16_t)}};
        hipStream_t stream = nullptr;
        hipEvent_t fork = nullptr, done = nullptr;
        bool used = false;                 // `done` has been recorded
        bool unjoined = false;             // ... and no caller stream waits for it yet
        unsigned seen_gen = 0;             // uploads `stream` has waited for
    };
    static constexpr int kMaxOverlap = 4;
    Slot slot[kMaxOverlap];
    std::vector<void *> retired;
    int reserved_max = 0;                  // largest batch passed to sa_reserve so far
    // ---- float64-state IIR (opt-in, sa_set_precision): everything below and the plans' d_p64 is allocated by the
    // first sa_set_precision(F64_STATE) and kept up to date only while the handle is in that mode (re-synced on entry)
    int precision = SA_PRECISION_F32;
    std::vector<double> win64;             // the window in double, natural order: default Hann or the caller's table widened
    double *d_win64 = nullptr;             // win64 transposed for iir_f64.hip: [32][256] pairs, pair (g, t) = w[64t + 2g], w[..+1]
    float4 *d_win_half = nullptr;          // constant 1/2 (the split step's factor) in the pass-A layout: the FFT launch's window
    // ---- SA_OUT_MARKER / SA_Q15_OUT_MARKER range (sa_set_marker_range): host state only, passed by value to every marker launch
    int marker_lo = 0, marker_hi = SA_NPTS;
    // ---- stream-ordered control plane (no device-wide synchronisation anywhere after sa_create)
    // Table uploads run on the handle's own control stream: it first waits for everything the handle has
    // launched so far, copies from a pinned staging slot, and records `uploaded`; the next process call makes its
    // stream wait for that event.  Other handles and other streams of the device are never stalled.
    // Ordering behind the handle's own launches: the event `launched` is bound to the completion of the last kernel
    // of every ordered-mode process call (hipExtLaunchKernel's stop event: it rides on the dispatch packet, where a
    // hipEventRecord after the launch puts a marker packet between two launches and measured 1.3-2.7 % of the step,
    // gpurun_out/ab_ov.log).  Uploads, stream switches and sa_destroy wait for that event; the caller's stream is
    // never touched after the call that passed it has returned, so the caller may destroy it at any time (touching
    // a destroyed stream crashes inside the runtime: gpurun_out/gpu_tests_b.log).  `last_stream` is compared, never
    // dereferenced; the capture query of control_allowed() touches `capture_stream` only, a stream whose capture the
    // handle has not yet seen closed (the caller ends a capture before destroying its stream: include/specan.h).
    hipStream_t ctl = nullptr;
    hipEvent_t launched = nullptr, uploaded = nullptr;
    bool launched_valid = false;           // `launched` has been bound to a launch at least once
    unsigned upload_gen = 0;               // number of uploads issued so far
    unsigned seen_gen = 0;                 // ordered mode: uploads the data stream has waited for
    hipStream_t last_stream = nullptr;     // stream of the most recent ordered-mode process call (compared, never used)
    bool have_last_stream = false;
    // a process call was captured into a graph on `capture_stream` and that capture has not been seen closed yet
    // (control_allowed): sticky across calls on OTHER streams; cleared by the query on that stream reporting "none"
    bool capture_open = false;
    hipStream_t capture_stream = nullptr;
    // ---- launch timing (opt-in, sa_set_profiling): a ring of timing-enabled event pairs; ordered-mode call k binds
    // pair k mod n to the begin of its first and the end of its last kernel (hipExtLaunchKernel: the events ride on the
    // dispatch packets, no marker packets), and `launched` aliases the pair's stop event from then on
    std::vector<hipEvent_t> prof_start, prof_stop;
    hipEvent_t launched_own = nullptr;     // the handle's own (timing-disabled) completion event
    unsigned long long prof_calls = 0;
    // ---- overlapped launches (opt-in, sa_set_overlap): consecutive process calls alternate over `overlap` internal
    // streams (Slot::stream) so that the tail of one launch runs under the head of the next; see include/specan.h
    int overlap = 1;
    hipStream_t ov_fit_stream = nullptr;      // the caller stream the internal streams were last fitted to (compared, never used)
    bool ov_fit_valid = false;
    unsigned long long ov_calls = 0;
    struct Stage {                         // a pinned staging slot (reused after kStage uploads)
        void *buf = nullptr;
        hipEvent_t done = nullptr;
        bool used = false;
    };
    static constexpr int kStage = 4;
    Stage stage[kStage];
    int stage_next = 0;
    // transport / sequencing state of imp/sequ2.vhd as far as the command bytes define it
    uint8_t transport = SA_CMD_ETHERNET_MODE;     // ether_en <= '1' on reset (imp/sequ2.vhd:85-86)
};

#pragma GCC visibility push(hidden)

constexpr size_t kStageBytes = sizeof(SaIirLaneTab);      // the largest table a handle uploads
static_assert(kStageBytes >= sizeof(float) * SA_NPTS, "a staging slot holds any table of the handle");

// One process call = begin_call, the launches on c.stream with workspace slot c.slot, end_call (see begin_call).
//   ordered mode: c.stream is the caller's stream; the call is ordered after pending table uploads and, if the
//     caller switched streams, after the handle's earlier launches; its last launch is bound to c.stop, which end_call
//     makes the handle's `launched`.
//   overlap mode (sa_set_overlap(h, d), d > 1): call k runs on internal stream k % d behind a fork event taken from
//     the caller's stream BEFORE that stream is made to wait for call k-d+1 (the join): kernel k depends on
//     what the caller enqueued before call k, not on kernels k-1 .. k-d+1, and may run beside them.
struct CallCtx {
    hipStream_t stream;
    hipEvent_t start;         // bound to the call's first kernel while sa_set_profiling is on, else null
    hipEvent_t stop;          // bound to the call's last kernel by the launcher (null inside a stream capture)
    int slot;
    int join;                 // overlap mode: the slot the caller's stream was made to wait for, else -1
    bool overlapped, captured;
};

// last sa_create() failure of the calling thread (sa_last_error(NULL)); per thread, so that concurrent creates on
// several host threads -- one per GPU, SURVEY 8(e) -- do not race on it
inline thread_local std::string g_create_error;

inline int fail(sa_handle *h, int code, const char *what, hipError_t e = hipSuccess)
{
    char buf[256];
    if (e != hipSuccess)
        std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else
        std::snprintf(buf, sizeof buf, "%s", what);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// fail() of an entry point that shares its body with another: "fn: what"
inline int fail_at(sa_handle *h, int code, const char *fn, const char *what)
{
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: %s", fn, what);
    return fail(h, code, buf);
}

#define SA_HIP(h, call)                                          \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return fail((h), SA_EHIP, #call, e_); \
    } while (0)

// ---- what specan_abi.cpp calls in sa_streams.cpp (each is explained where it is defined)
int control_allowed(sa_handle *h);
int upload(sa_handle *h, void *dst, const void *src, size_t bytes);
int grow_slots(sa_handle *h, int n, int frames, bool geometric, bool f64_only = false);
int begin_call(sa_handle *h, hipStream_t user, int work, int frames, CallCtx *c, int work2 = -1, int frames2 = 0);
int end_call(sa_handle *h, const CallCtx &c);

#pragma GCC visibility pop
