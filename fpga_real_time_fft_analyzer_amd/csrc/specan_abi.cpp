// specan_abi.cpp -- host side of the C ABI declared in include/specan.h.
//
// Owns: the opaque handle, device tables (window, twiddles, IIR plans: built by iir_plan.cpp), the launch slots and the
// command-byte state machine that mirrors new/rx_filter_coeff.vhd + new/command_control.vhd.
// Never touches caller tensors except through the pointers given to the process calls, never
// falls back to CPU compute.
#include "../../include/specan.h"
#include "iir_plan.hpp"
#include "sa_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace {

// last sa_create() failure of the calling thread (sa_last_error(NULL)); per thread, so that concurrent creates on
// several host threads -- one per GPU, SURVEY 8(e) -- do not race on it
thread_local std::string g_create_error;

}  // namespace

hipError_t sa_set_dyn_lds_once(const void *kernel, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;        // (kernel, device)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({kernel, dev})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({kernel, dev});
    return e;
}

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
    enum { kWorkQ15, kWorkF64, kWorkKinds };
    // Launch slot i (slot 0 = ordered mode; overlap mode uses slots 0..depth-1): its workspaces -- the Q15 cascade's
    // int16 output, and in float64-state mode the float32 y [B,16384] -- and, in overlap mode, its internal stream
    struct Slot {
        Workspace work[kWorkKinds] = {{nullptr, 0, sizeof(int16_t)}, {nullptr, 0, sizeof(float)}};
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

namespace {

int fail(sa_handle *h, int code, const char *what, hipError_t e = hipSuccess)
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
int fail_at(sa_handle *h, int code, const char *fn, const char *what)
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

// ---- overlap mode: which streams run beside each other ------------------------------------------------------
// The runtime maps a process's streams onto a few hardware queues (four here) and two streams that share a queue
// execute in order: a handle whose two internal streams fall on one queue gets no overlap and pays for the fork /
// join events on top (measured, tools/ubench/stream_pairs.hip and profiles/r3_overlap_streams.txt: streams 3 and 4
// created back to back share a queue; such a handle ran 144 us per batch against 135 us stream-ordered and 127 us
// with two queues).  The mapping is not exposed, so sa_set_overlap() asks the hardware: a one-wave kernel that
// waits 100 us on the constant 100 MHz counter is put on both streams; if the second finishes within 150 us of the
// first one's start they ran side by side.  The loop ends on the counter or on its iteration cap, whichever first.
__global__ void sa_spin_kernel(unsigned ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < 200000 && __builtin_amdgcn_s_memrealtime() - t0 < ticks; ++i) __builtin_amdgcn_s_sleep(8);
}

// 1 = kernels on a and b overlap, 0 = they run one after the other, negative = HIP error (text in *err)
int streams_run_side_by_side(hipStream_t a, hipStream_t b, hipError_t *err)
{
    constexpr unsigned kTicks = 10000;                   // 100 us
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&ea);
    if (e == hipSuccess) e = hipEventCreate(&eb);
    float ms = 1e9f;
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {        // pass 0 warms the launch path up (code object load)
        const unsigned ticks = pass == 0 ? 10u : kTicks;
        e = hipEventRecord(e0, a);
        if (e == hipSuccess) hipLaunchKernelGGL(sa_spin_kernel, dim3(1), dim3(64), 0, a, ticks);
        if (e == hipSuccess) hipLaunchKernelGGL(sa_spin_kernel, dim3(1), dim3(64), 0, b, ticks);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ea, a);
        if (e == hipSuccess) e = hipEventRecord(eb, b);
        if (e == hipSuccess) e = hipEventSynchronize(ea);
        if (e == hipSuccess) e = hipEventSynchronize(eb);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, eb);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (e != hipSuccess) { *err = e; return -1; }
    return ms < 0.15f ? 1 : 0;
}

// A new stream that runs beside every stream in `avoid`.  Best effort: after six candidates the last one is kept
// whatever the probe said (a GPU busy with other work can make side-by-side kernels look serial, and with four
// hardware queues five streams cannot all be apart).
int pick_stream(sa_handle *h, const hipStream_t *avoid, int navoid, hipStream_t *out)
{
    hipStream_t rejected[6];
    int nrej = 0, rc = SA_OK;
    *out = nullptr;
    for (int tries = 0; tries < 6 && !*out && rc == SA_OK; ++tries) {
        hipStream_t c = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&c, hipStreamNonBlocking);
        if (e != hipSuccess) { rc = fail(h, SA_EHIP, "overlap: hipStreamCreateWithFlags", e); break; }
        bool ok = true;
        for (int j = 0; j < navoid && ok; ++j) {
            hipError_t pe = hipSuccess;
            const int r = streams_run_side_by_side(avoid[j], c, &pe);
            if (r < 0) { rc = fail(h, SA_EHIP, "overlap: stream probe", pe); ok = false; }
            else ok = r == 1;
        }
        if (rc == SA_OK && (ok || tries == 5)) *out = c;
        else rejected[nrej++] = c;
    }
    for (int q = 0; q < nrej; ++q) (void)hipStreamDestroy(rejected[q]);
    return rc;
}

constexpr size_t kStageBytes = sizeof(SaIirLaneTab);      // the largest table a handle uploads
static_assert(kStageBytes >= sizeof(float) * SA_NPTS, "a staging slot holds any table of the handle");

// Control-plane calls change host state and device tables; a process call that is being captured into a hipGraph
// has frozen the host part (kernel arguments) but not the tables, so such calls are refused while a capture that took
// one of the handle's process calls is still open.  Checked at the top of every control-plane entry point, before
// anything is changed.  The record is sticky: a later, uncaptured call on ANOTHER stream does not clear it; only the
// query on the capturing stream does (here, or in begin_call when that stream is used again), and once it has reported
// "none" that stream is never queried again on the record's behalf.
int control_allowed(sa_handle *h)
{
    if (!h->capture_open) return SA_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->capture_stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        cs = hipStreamCaptureStatusNone;
    }
    if (cs != hipStreamCaptureStatusNone)
        return fail(h, SA_ESTATE, "control-plane call while a stream that captured one of the handle's calls is still capturing");
    h->capture_open = false;
    h->capture_stream = nullptr;
    return SA_OK;
}

// Stream-ordered table update (see sa_handle): after everything launched so far, before everything launched
// later; asynchronous for the host except when all staging slots are still waiting for their copies.
int upload(sa_handle *h, void *dst, const void *src, size_t bytes)
{
    if (bytes > kStageBytes) return fail(h, SA_EINVAL, "upload: table larger than the staging slot");
    SA_HIP(h, hipSetDevice(h->device));
    sa_handle::Stage &st = h->stage[h->stage_next];
    h->stage_next = (h->stage_next + 1) % sa_handle::kStage;
    if (st.used) SA_HIP(h, hipEventSynchronize(st.done));       // that slot's old copy has run
    std::memcpy(st.buf, src, bytes);
    if (h->launched_valid) SA_HIP(h, hipStreamWaitEvent(h->ctl, h->launched, 0));
    for (const sa_handle::Slot &s : h->slot)
        if (s.used) SA_HIP(h, hipStreamWaitEvent(h->ctl, s.done, 0));
    SA_HIP(h, hipMemcpyAsync(dst, st.buf, bytes, hipMemcpyHostToDevice, h->ctl));
    SA_HIP(h, hipEventRecord(st.done, h->ctl));
    st.used = true;
    SA_HIP(h, hipEventRecord(h->uploaded, h->ctl));
    ++h->upload_gen;
    return SA_OK;
}

// Workspace `w` grown to `frames` without touching launches in flight (see sa_handle::Workspace).
// `geometric`: grow by at least half (process calls with creeping batch sizes); exact sizing where the size is copied
// from another slot -- sa_set_overlap gave every slot max(the others, 1.5 x its own), and two slots leap-frogged each
// other by a factor 1.5 per mode change until hipMalloc failed (found by a 10-minute soak, seed 77).
int ensure_work(sa_handle *h, sa_handle::Workspace &w, int frames, bool captured, bool geometric = true)
{
    if (frames <= w.frames) return SA_OK;
    if (captured) return fail(h, SA_ESTATE, "workspace growth inside a stream capture: call sa_reserve() first");
    long want = frames, geo = (long)w.frames + w.frames / 2;
    if (geometric && geo > want) want = geo;
    void *p = nullptr;
    SA_HIP(h, hipMalloc(&p, (size_t)want * SA_NPTS * w.elem));
    if (w.ptr) h->retired.push_back(w.ptr);
    w.ptr = p;
    w.frames = (int)want;
    return SA_OK;
}

// The workspaces of slots 0..n-1 that the handle's precision launches with (`f64_only`: the float64-state one alone)
// grown to `frames`; frames < 0: exactly to the largest of that kind any slot has (slots new to overlap mode start with
// what the handle already has somewhere)
int grow_slots(sa_handle *h, int n, int frames, bool geometric, bool f64_only = false)
{
    const int k0 = f64_only ? sa_handle::kWorkF64 : sa_handle::kWorkQ15;
    const int k1 = f64_only || h->precision == SA_PRECISION_F64_STATE ? sa_handle::kWorkKinds : sa_handle::kWorkF64;
    for (int k = k0; k < k1; ++k) {
        int want = frames;
        if (want < 0)
            for (const sa_handle::Slot &s : h->slot) want = std::max(want, s.work[k].frames);
        for (int i = 0; i < n; ++i) {
            const int rc = ensure_work(h, h->slot[i].work[k], want, false, geometric);
            if (rc != SA_OK) return rc;
        }
    }
    return SA_OK;
}

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

// First overlapped call from a caller stream: an internal stream that shares a hardware queue with the CALLER's
// stream is as bad as two internal streams on one queue (the join waits of the caller's stream sit in front of
// the internal stream's next kernel: the six-handle run of profiles/r3_overlap_streams.txt), and the caller's
// stream is only known here.  Every internal stream is probed against it and replaced if they run in order.
// Costs a host wait for the caller stream's earlier work plus ~0.3 ms per internal stream, once per (handle,
// caller stream).
int fit_overlap_streams(sa_handle *h, hipStream_t user)
{
    for (int i = 0; i < h->overlap; ++i) {
        hipError_t pe = hipSuccess;
        sa_handle::Slot &s = h->slot[i];
        const int r = streams_run_side_by_side(user, s.stream, &pe);
        if (r < 0) return fail(h, SA_EHIP, "overlap: stream probe", pe);
        if (r == 1) continue;
        hipStream_t avoid[sa_handle::kMaxOverlap + 1] = {user};
        int n = 1;
        for (int j = 0; j < h->overlap; ++j)
            if (j != i) avoid[n++] = h->slot[j].stream;
        hipStream_t repl = nullptr;
        const int rc = pick_stream(h, avoid, n, &repl);
        if (rc != SA_OK) return rc;
        if (s.used) SA_HIP(h, hipEventSynchronize(s.done));                      // the old stream's work is over
        (void)hipStreamDestroy(s.stream);
        s.stream = repl;
        s.seen_gen = h->upload_gen - 1;                                          // the new stream has seen no upload
    }
    h->ov_fit_stream = user;
    h->ov_fit_valid = true;
    return SA_OK;
}

// Steps 1 and 2 of a process call: (1) decide -- capture query (it also keeps the sticky capture record), stream, slot,
// growth of the slot's workspace `work` to `frames` (work < 0: none); (2) enqueue the ordering waits.  The caller
// launches (3) and commits with end_call (4) only when every launch succeeded: a call that fails leaves `launched`,
// the profiling ring and the join state on the last launch that did happen.
int begin_call(sa_handle *h, hipStream_t user, int work, int frames, CallCtx *c)
{
    c->stream = user;
    c->start = c->stop = nullptr;
    c->slot = 0;
    c->join = -1;
    c->overlapped = h->overlap > 1;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    SA_HIP(h, hipStreamIsCapturing(user, &cs));
    c->captured = cs != hipStreamCaptureStatusNone;
    if (c->captured) {
        h->capture_open = true;
        h->capture_stream = user;
    } else if (h->capture_open && h->capture_stream == user) {
        h->capture_open = false;             // that stream's capture has ended
        h->capture_stream = nullptr;
    }
    if (c->overlapped) {
        if (c->captured)
            return fail(h, SA_ESTATE, "overlapped launches (sa_set_overlap > 1) cannot be captured into a graph");
        if (!h->ov_fit_valid || h->ov_fit_stream != user) {
            const int rc = fit_overlap_streams(h, user);
            if (rc != SA_OK) return rc;
        }
        c->slot = (int)(h->ov_calls % (unsigned)h->overlap);
        c->stream = h->slot[c->slot].stream;
        c->stop = h->slot[c->slot].done;
    } else if (!c->captured) {               // a captured record would tie the event to the graph; replays are ordered by the caller (include/specan.h)
        c->stop = h->launched;
        if (!h->prof_stop.empty()) {         // timed call: the ring's next pair
            const size_t i = (size_t)(h->prof_calls % h->prof_stop.size());
            c->start = h->prof_start[i];
            c->stop = h->prof_stop[i];
        }
    }
    if (work >= 0) { const int rc = ensure_work(h, h->slot[c->slot].work[work], frames, c->captured); if (rc != SA_OK) return rc; }
    if (c->overlapped) {
        sa_handle::Slot &s = h->slot[c->slot];
        SA_HIP(h, hipEventRecord(s.fork, user));
        // join: the call issued d-1 calls ago (the next user of the oldest slot is the call after this one)
        const int join = (c->slot + 1) % h->overlap;
        if (h->slot[join].unjoined) {
            SA_HIP(h, hipStreamWaitEvent(user, h->slot[join].done, 0));
            c->join = join;
        }
        SA_HIP(h, hipStreamWaitEvent(s.stream, s.fork, 0));
        // (ordered-mode launches made before the switch to overlap mode have completed: sa_set_overlap waited)
        if (s.seen_gen != h->upload_gen) {
            SA_HIP(h, hipStreamWaitEvent(s.stream, h->uploaded, 0));
            s.seen_gen = h->upload_gen;
        }
        return SA_OK;
    }
    if (h->have_last_stream && h->last_stream != user) {
        if (h->launched_valid) SA_HIP(h, hipStreamWaitEvent(user, h->launched, 0));
        h->seen_gen = h->upload_gen - 1;     // the new stream has not seen the last upload either
    }
    if (h->seen_gen != h->upload_gen) {
        if (h->upload_gen) SA_HIP(h, hipStreamWaitEvent(user, h->uploaded, 0));
        h->seen_gen = h->upload_gen;
    }
    h->last_stream = user;
    h->have_last_stream = true;
    return SA_OK;
}

// Step 4: every launch of the call was enqueued
int end_call(sa_handle *h, const CallCtx &c)
{
    if (c.overlapped) {
        if (c.join >= 0) h->slot[c.join].unjoined = false;
        h->slot[c.slot].used = true;
        h->slot[c.slot].unjoined = true;
        ++h->ov_calls;
    } else if (!c.captured) {
        h->launched = c.stop;
        h->launched_valid = true;
        if (!h->prof_stop.empty()) ++h->prof_calls;
    }
    return SA_OK;
}

void default_window_f64(std::vector<double> &w)
{
    w.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i)   // scripts/hann_coeff.py:3-4
        w[i] = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)i / (double)(SA_NPTS - 1)));
}

void default_rom(std::vector<int16_t> &rom)
{
    std::vector<double> w;
    default_window_f64(w);
    rom.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i) {   // scripts/hann_coeff.py:5 (rint, int16 wrap: quirk Q1)
        const double r = std::rint((w[i] - 0.5) * 65536.0);
        rom[i] = (int16_t)(uint16_t)((int32_t)r & 0xFFFF);
    }
}

// half = 0.5 * window (exact scaling, undone by the split step).  Two device copies, each arranged so
// that the kernel's loads are coalesced 16-byte accesses in the layout it computes in:
//   tr (IIR kernels, chunk layout):   tr[g][t] = w[64t + E g .. + E-1], E = 16 bytes / sizeof(T) (float: the half
//                                     window, [16][256] quads; double: the window of iir_f64.hip, [32][256] pairs)
//   pa (no-IIR kernel, pass-A layout): pa[p][t] = half[512(2p)+2t], [..+1], half[512(2p+1)+2t], [..+1]
template <class T>
void transpose_window(const std::vector<T> &w, std::vector<T> &tr)
{
    constexpr int E = 16 / sizeof(T);
    tr.resize(SA_NPTS);
    for (int t = 0; t < 256; ++t)
        for (int g = 0; g < 64 / E; ++g)
            for (int e = 0; e < E; ++e) tr[(g * 256 + t) * E + e] = w[64 * t + E * g + e];
}

void pass_a_window(const std::vector<float> &half, std::vector<float> &pa)
{
    pa.resize(SA_NPTS);
    for (int p = 0; p < 16; ++p)
        for (int t = 0; t < 256; ++t) {
            float *o = &pa[(p * 256 + t) * 4];
            o[0] = half[512 * (2 * p) + 2 * t];
            o[1] = half[512 * (2 * p) + 2 * t + 1];
            o[2] = half[512 * (2 * p + 1) + 2 * t];
            o[3] = half[512 * (2 * p + 1) + 2 * t + 1];
        }
}

// The default window, Hann (scripts/hann_coeff.py:3-4): in double, its float half, and the cosine form set to
// (0.5, 0.5) exactly (not fitted: a fitted (a0, a1) would change the bits of the generated window)
void default_window(sa_handle *h)
{
    default_window_f64(h->win64);
    h->half_win.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i) h->half_win[i] = (float)(0.5 * h->win64[i]);
    h->win_is_cos = true;
    h->win_cos[0] = h->win_cos[1] = 0.5;
}

// Is w[n] = a0 - a1 cos(2 pi n / (N-1)) to within float rounding?  Least-squares fit of (a0, a1) in double, then
// the residual against 1.5e-7 of the window's peak: Hann, Hamming and every other two-term cosine window pass,
// anything else (Blackman, Kaiser, rectangular with a taper, ...) keeps the table.
bool fit_cosine_window(const float *w, double out[2])
{
    const double theta = 2.0 * M_PI / (double)(SA_NPTS - 1);
    double s1 = 0, sc = 0, scc = 0, sw = 0, swc = 0, peak = 0;
    for (int n = 0; n < SA_NPTS; ++n) {
        const double c = -std::cos(theta * n), v = (double)w[n];
        s1 += 1.0; sc += c; scc += c * c; sw += v; swc += v * c;
        peak = std::fmax(peak, std::fabs(v));
    }
    const double det = s1 * scc - sc * sc;
    if (!(det > 0.0) || !(peak > 0.0) || !std::isfinite(peak)) return false;
    const double a0 = (sw * scc - swc * sc) / det, a1 = (s1 * swc - sc * sw) / det;
    double worst = 0;
    for (int n = 0; n < SA_NPTS; ++n) worst = std::fmax(worst, std::fabs((double)w[n] - (a0 - a1 * std::cos(theta * n))));
    if (!(worst <= 1.5e-7 * peak)) return false;
    out[0] = a0;
    out[1] = a1;
    return true;
}

// How a table reaches the device: upload() on the control plane; copy_at_create in sa_create
using CopyFn = int (*)(sa_handle *h, void *dst, const void *src, size_t bytes);

// sa_create's copies are blocking (it synchronises the device at the end) and no uploads: upload_gen stays 0
int copy_at_create(sa_handle *, void *dst, const void *src, size_t bytes)
{
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? SA_OK : fail(nullptr, SA_EHIP, "sa_create: hipMemcpy", e);
}

// Device tables of the float64-state mode from the handle's double state: both plans (from the double SOS, never from
// the float32 plan) and, with `window`, the double window.  Nothing unless the handle is in that mode or `force`.
int sync_f64(sa_handle *h, bool window, bool force = false)
{
    if (h->precision != SA_PRECISION_F64_STATE && !force) return SA_OK;
    for (sa_handle::Plan *pl : {&h->plan_default, &h->plan_custom}) {
        SaIirF64 p;
        build_plan_f64(pl->sos, pl->nsec, &p);
        const int rc = upload(h, pl->d_p64, &p, sizeof p);
        if (rc != SA_OK) return rc;
    }
    if (!window) return SA_OK;
    std::vector<double> tr;
    transpose_window(h->win64, tr);
    const size_t half = sizeof(double) * SA_NPTS / 2;     // two uploads: a staging slot holds 64 KiB, the table is 128
    const int rc = upload(h, h->d_win64, tr.data(), half);
    if (rc != SA_OK) return rc;
    return upload(h, h->d_win64 + SA_NPTS / 2, tr.data() + SA_NPTS / 2, half);
}

// The float32 plan `pl` from its SOS and the handle's window; its lane table to the device
int write_plan(sa_handle *h, sa_handle::Plan &pl, CopyFn copy)
{
    build_plan(pl.sos, pl.nsec, &pl.k, &pl.lt, h->half_win.data(), h->win_is_cos ? h->win_cos : nullptr);
    return copy(h, pl.d_lt, &pl.lt, sizeof pl.lt);
}

// The device tables that follow the float window h->half_win: its two layouts, then both plans (each carries its own
// gain-scaled copy of the window) and the float64-state tables (none in sa_create: a new handle is in float32 precision)
int write_window(sa_handle *h, CopyFn copy)
{
    std::vector<float> tr, pa;
    transpose_window(h->half_win, tr);
    pass_a_window(h->half_win, pa);
    int rc = copy(h, h->d_win_b, pa.data(), sizeof(float) * SA_NPTS);
    if (rc == SA_OK) rc = copy(h, h->d_win_t, tr.data(), sizeof(float) * SA_NPTS);
    if (rc == SA_OK) rc = write_plan(h, h->plan_default, copy);
    if (rc == SA_OK) rc = write_plan(h, h->plan_custom, copy);
    if (rc == SA_OK) rc = sync_f64(h, true);
    return rc;
}

int set_custom_plan(sa_handle *h, const double *sos_norm, int nsec)
{
    sa_handle::Plan &pl = h->plan_custom;
    std::memset(pl.sos, 0, sizeof pl.sos);
    std::memcpy(pl.sos, sos_norm, sizeof(double) * 6 * (size_t)nsec);
    pl.nsec = nsec;
    const int rc = write_plan(h, pl, upload);
    if (rc != SA_OK) return rc;
    return sync_f64(h, false);
}

// The cascade of the filter mode: the fixed one for DEFAULT, the loaded one for every other mode (what the debug
// exports show for NONE and WIDE; float launches in mode NONE run without a cascade)
const sa_handle::Plan &active_plan(const sa_handle *h)
{
    return h->filter_mode == SA_FILTER_DEFAULT ? h->plan_default : h->plan_custom;
}

}  // namespace

extern "C" {

int sa_abi_version(void) { return SA_ABI_VERSION; }

const char *sa_last_error(const sa_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int sa_create(int device, sa_handle **out)
{
    if (!out) return fail(nullptr, SA_EINVAL, "sa_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SA_EHIP, "sa_create: no usable HIP device (this library has no CPU fallback)", e);
    if (device < 0 || device >= ndev) return fail(nullptr, SA_EINVAL, "sa_create: device index out of range");
    sa_handle *h = new (std::nothrow) sa_handle();
    if (!h) return fail(nullptr, SA_ENOMEM, "sa_create: out of host memory");
    h->device = device;
#define SA_HIPC(call)                                                      \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) {                                            \
            fail(nullptr, SA_EHIP, #call, e_);                             \
            sa_destroy(h);                                                 \
            return SA_EHIP;                                                \
        }                                                                  \
    } while (0)
    SA_HIPC(hipSetDevice(device));
    SA_HIPC(hipStreamCreateWithFlags(&h->ctl, hipStreamNonBlocking));
    SA_HIPC(hipEventCreateWithFlags(&h->launched_own, hipEventDisableTiming));
    h->launched = h->launched_own;
    SA_HIPC(hipEventCreateWithFlags(&h->uploaded, hipEventDisableTiming));
    for (sa_handle::Stage &st : h->stage) {
        SA_HIPC(hipHostMalloc(&st.buf, kStageBytes, hipHostMallocDefault));
        SA_HIPC(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    }
    SA_HIPC(hipMalloc(&h->d_win_b, sizeof(float) * SA_NPTS));
    SA_HIPC(hipMalloc(&h->d_win_t, sizeof(float) * SA_NPTS));
    SA_HIPC(hipMalloc(&h->d_twT, sizeof(float4) * 6 * 256));
    SA_HIPC(hipMalloc(&h->d_twB, sizeof(float4) * 8 * 16));
    SA_HIPC(hipMalloc(&h->d_twC, sizeof(float2) * 25));
    SA_HIPC(hipMalloc(&h->plan_default.d_lt, sizeof(SaIirLaneTab)));
    SA_HIPC(hipMalloc(&h->plan_custom.d_lt, sizeof(SaIirLaneTab)));
    SA_HIPC(hipMalloc(&h->d_rom, sizeof(int16_t) * SA_NPTS));
    SA_HIPC(hipMalloc(&h->d_twq, sizeof(uint2) * SA_NPTS));
    SA_HIPC(hipMalloc(&h->d_twrec, sizeof(uint4) * 2 * kSaTwRecs));

    // float tables: the default window and the IIR plans (default = the fixed ALPHA/BETA cascade as real taps;
    // custom = cleared coefficients), then the twiddles
    sos_from_q7(kDefaultQ7, h->plan_default.sos);
    sos_from_q7(h->c12_custom, h->plan_custom.sos);
    h->plan_default.nsec = h->plan_custom.nsec = 6;
    default_window(h);
    if (write_window(h, copy_at_create) != SA_OK) {
        sa_destroy(h);
        return SA_EHIP;
    }
    {
        std::vector<float4> ta(6 * 256), tb(8 * 16);
        std::vector<float2> tc(25);
        auto w8192 = [](long e) {                          // exp(-2 pi i e / 8192), e reduced first (exact)
            const double a = -2.0 * M_PI * (double)(e % 8192) / 8192.0;
            return make_float2((float)std::cos(a), (float)std::sin(a));
        };
        for (int t = 0; t < 256; ++t) {                    // per-thread anchors (SaF32Tables::twT)
            const int k[10] = {1, 2, 3, 4, 5, 6, 7, 8, 16, 24};
            for (int i = 0; i < 5; ++i) {
                const float2 u = w8192((long)k[2 * i] * t), v = w8192((long)k[2 * i + 1] * t);
                ta[i * 256 + t] = make_float4(u.x, u.y, v.x, v.y);
            }
            const double ap = -2.0 * M_PI * (double)(4 * t) / 16384.0;
            const double an = -2.0 * M_PI * (double)(4 * ((t + 1) & 255)) / 16384.0;      // (1, 0) for t = 255
            ta[5 * 256 + t] = make_float4((float)std::cos(ap), (float)std::sin(ap), (float)std::cos(an), (float)std::sin(an));
        }
        for (int pp = 0; pp < 8; ++pp)
            for (int b = 0; b < 16; ++b) {
                const double a0 = -2.0 * M_PI * (double)(2 * pp * b) / 256.0;
                const double a1 = -2.0 * M_PI * (double)((2 * pp + 1) * b) / 256.0;
                tb[pp * 16 + b] = make_float4((float)std::cos(a0), (float)std::sin(a0), (float)std::cos(a1), (float)std::sin(a1));
            }
        for (int blk = 0; blk < 5; ++blk)                   // block 4 = bin 4096 only (the seam of the last group)
            for (int e = 0; e < 5; ++e) {
                const double ang = -2.0 * M_PI * (double)(1024 * blk + e) / 16384.0;
                tc[blk * 5 + e] = make_float2((float)std::cos(ang), (float)std::sin(ang));
            }
        SA_HIPC(hipMemcpy(h->d_twT, ta.data(), sizeof(float4) * ta.size(), hipMemcpyHostToDevice));
        SA_HIPC(hipMemcpy(h->d_twB, tb.data(), sizeof(float4) * tb.size(), hipMemcpyHostToDevice));
        SA_HIPC(hipMemcpy(h->d_twC, tc.data(), sizeof(float2) * tc.size(), hipMemcpyHostToDevice));
    }
    // integer tables
    {
        default_rom(h->rom);
        SA_HIPC(hipMemcpy(h->d_rom, h->rom.data(), sizeof(int16_t) * SA_NPTS, hipMemcpyHostToDevice));
        std::vector<uint2> tq(SA_NPTS);
        for (int m = 0; m < SA_NPTS; ++m) {   // SA-FXFFT-1 twiddles: clamp16(rint(32768 cos)), clamp16(rint(-32768 sin))
            const double a = 2.0 * M_PI * (double)m / (double)SA_NPTS;
            long wr = std::lrint(32768.0 * std::cos(a)), wi = std::lrint(-32768.0 * std::sin(a));
            wr = wr > 32767 ? 32767 : (wr < -32768 ? -32768 : wr);
            wi = wi > 32767 ? 32767 : (wi < -32768 ? -32768 : wi);
            // second word (-wi, wr): the operand of the two-term dot product for the real part.  -wi does not fit
            // for wi = -32768 (exponents 4082..4110); the kernel never takes the second word of those entries
            // (fx_butterfly: `wide1`, `wide2`, `wide3`)
            const long nwi = -wi > 32767 ? 32767 : -wi;
            // the kernel's compile-time choice of the butterflies that avoid the second word rests on this range
            // (margins: 32768 sin = 32767.528 at 4082 and 4110, 32767.458 at 4081 and 4111; the threshold is .5)
            if (wi == -32768 && (m < 4082 || m > 4110)) {
                g_create_error = "sa_create: twiddle table: wi = -32768 outside exponents 4082..4110";
                sa_destroy(h);
                return SA_ESTATE;
            }
            tq[m].x = ((uint32_t)wr & 0xFFFFu) | ((uint32_t)wi << 16);
            tq[m].y = ((uint32_t)nwi & 0xFFFFu) | ((uint32_t)wr << 16);
        }
        SA_HIPC(hipMemcpy(h->d_twq, tq.data(), sizeof(uint2) * SA_NPTS, hipMemcpyHostToDevice));
        // One 32-byte record {w(e), w(2e), w(3e), pad} per butterfly of the stages whose exponents differ from lane to
        // lane: a lane's three twiddles are one contiguous read instead of three gathers at strides 8, 16 and 24 bytes.
        std::vector<uint4> rec(2 * kSaTwRecs);
        for (int r = 0; r < kSaTwRecs; ++r) {
            const int e = r < 4096 ? r : (r < 5120 ? 4 * (r - 4096) : 16 * (r - 5120));
            rec[2 * r] = make_uint4(tq[e].x, tq[e].y, tq[2 * e].x, tq[2 * e].y);
            rec[2 * r + 1] = make_uint4(tq[3 * e].x, tq[3 * e].y, 0u, 0u);
        }
        SA_HIPC(hipMemcpy(h->d_twrec, rec.data(), sizeof(uint4) * 2 * kSaTwRecs, hipMemcpyHostToDevice));
    }
    SA_HIPC(hipDeviceSynchronize());          // creation only: the blocking copies above are complete
#undef SA_HIPC
    *out = h;
    return SA_OK;
}

int sa_destroy(sa_handle *h)
{
    if (!h) return SA_OK;
    (void)hipSetDevice(h->device);
    // this handle's work only, through handle-owned objects (the caller's streams may be gone already)
    if (h->launched_valid) (void)hipEventSynchronize(h->launched);
    for (sa_handle::Slot &s : h->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.fork) (void)hipEventDestroy(s.fork);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        for (const sa_handle::Workspace &w : s.work) (void)hipFree(w.ptr);
    }
    if (h->ctl) (void)hipStreamSynchronize(h->ctl);
    for (sa_handle::Stage &st : h->stage) {
        if (st.buf) (void)hipHostFree(st.buf);
        if (st.done) (void)hipEventDestroy(st.done);
    }
    for (hipEvent_t e : h->prof_start) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->prof_stop) (void)hipEventDestroy(e);
    if (h->launched_own) (void)hipEventDestroy(h->launched_own);
    if (h->uploaded) (void)hipEventDestroy(h->uploaded);
    if (h->ctl) (void)hipStreamDestroy(h->ctl);
    (void)hipFree(h->d_win_b);
    (void)hipFree(h->d_win_t);
    (void)hipFree(h->d_twT);
    (void)hipFree(h->d_twB);
    (void)hipFree(h->d_twC);
    (void)hipFree(h->d_rom);
    (void)hipFree(h->d_twq);
    (void)hipFree(h->d_twrec);
    for (sa_handle::Plan *pl : {&h->plan_default, &h->plan_custom}) {
        (void)hipFree(pl->d_lt);
        (void)hipFree(pl->d_p64);
    }
    (void)hipFree(h->d_win64);
    (void)hipFree(h->d_win_half);
    for (void *p : h->retired) (void)hipFree(p);
    delete h;
    return SA_OK;
}

int sa_reserve(sa_handle *h, int max_batch)
{
    if (!h) return SA_EINVAL;
    if (max_batch < 0) return fail(h, SA_ESHAPE, "sa_reserve: negative batch");
    SA_HIP(h, hipSetDevice(h->device));
    if (max_batch > h->reserved_max) h->reserved_max = max_batch;
    return grow_slots(h, h->overlap, max_batch, /*geometric=*/true);
}

int sa_set_overlap(sa_handle *h, int depth)
{
    if (!h) return SA_EINVAL;
    if (depth < 1 || depth > sa_handle::kMaxOverlap) return fail(h, SA_EINVAL, "sa_set_overlap: depth must be 1..4");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    if (depth == h->overlap) return SA_OK;
    if (depth > 1 && !h->prof_stop.empty())
        return fail(h, SA_ESTATE, "sa_set_overlap: launch timing (sa_set_profiling) is for stream-ordered launches; turn it off first");
    SA_HIP(h, hipSetDevice(h->device));
    // leave the old mode with nothing of the handle's in flight (host wait on the handle's own work only)
    if (h->launched_valid) SA_HIP(h, hipEventSynchronize(h->launched));
    for (sa_handle::Slot &s : h->slot) {
        if (s.used) SA_HIP(h, hipEventSynchronize(s.done));
        s.unjoined = false;
    }
    hipStream_t have[sa_handle::kMaxOverlap];
    for (int i = 0; i < depth; ++i) {
        sa_handle::Slot &s = h->slot[i];
        if (!s.stream) {
            const int rc = pick_stream(h, have, i, &s.stream);     // beside the streams the handle already has
            if (rc != SA_OK) return rc;
        }
        have[i] = s.stream;
        if (!s.fork) SA_HIP(h, hipEventCreateWithFlags(&s.fork, hipEventDisableTiming));
        if (!s.done) SA_HIP(h, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    { const int rc = grow_slots(h, depth, -1, /*geometric=*/false); if (rc != SA_OK) return rc; }
    h->overlap = depth;
    h->ov_calls = 0;
    h->ov_fit_valid = false;
    return SA_OK;
}

int sa_get_overlap(const sa_handle *h, int *depth)
{
    if (!h || !depth) return SA_EINVAL;
    *depth = h->overlap;
    return SA_OK;
}

int sa_debug_overlap_streams(sa_handle *h, void *stream, int *side_by_side)
{
    if (!h || !side_by_side) return SA_EINVAL;
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    SA_HIP(h, hipSetDevice(h->device));
    *side_by_side = 1;
    if (h->overlap < 2) return SA_OK;
    for (int i = 0; i < h->overlap; ++i)
        for (int j = -1; j < i; ++j) {                       // j = -1: the caller's stream
            hipError_t pe = hipSuccess;
            const int r = streams_run_side_by_side(j < 0 ? (hipStream_t)stream : h->slot[j].stream, h->slot[i].stream, &pe);
            if (r < 0) return fail(h, SA_EHIP, "sa_debug_overlap_streams", pe);
            if (r == 0) *side_by_side = 0;
        }
    return SA_OK;
}

int sa_set_profiling(sa_handle *h, int ring)
{
    if (!h) return SA_EINVAL;
    if (ring < 0 || ring > 65536) return fail(h, SA_EINVAL, "sa_set_profiling: ring must be 0..65536");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    if (ring > 0 && h->overlap > 1)
        return fail(h, SA_ESTATE, "sa_set_profiling: launch timing is for stream-ordered launches (sa_set_overlap(h, 1) first)");
    SA_HIP(h, hipSetDevice(h->device));
    // nothing of the handle's in flight while the completion event changes hands
    if (h->launched_valid) SA_HIP(h, hipEventSynchronize(h->launched));
    h->launched_valid = false;
    h->launched = h->launched_own;
    for (hipEvent_t e : h->prof_start) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->prof_stop) (void)hipEventDestroy(e);
    h->prof_start.clear();
    h->prof_stop.clear();
    h->prof_calls = 0;
    for (int i = 0; i < ring; ++i) {
        hipEvent_t a = nullptr, b = nullptr;
        hipError_t e = hipEventCreate(&a);
        if (e == hipSuccess) e = hipEventCreate(&b);
        if (e != hipSuccess) {
            if (a) (void)hipEventDestroy(a);
            return fail(h, SA_EHIP, "sa_set_profiling: hipEventCreate", e);
        }
        h->prof_start.push_back(a);
        h->prof_stop.push_back(b);
    }
    return SA_OK;
}

int sa_profile_read(sa_handle *h, float *ms, int cap)
{
    if (!h) return SA_EINVAL;
    if (cap < 0 || (cap > 0 && !ms)) return fail(h, SA_EINVAL, "sa_profile_read: bad buffer");
    if (h->prof_stop.empty()) return fail(h, SA_ESTATE, "sa_profile_read: sa_set_profiling is off");
    SA_HIP(h, hipSetDevice(h->device));
    const unsigned long long n = h->prof_stop.size();
    unsigned long long have = h->prof_calls < n ? h->prof_calls : n;
    if (have > (unsigned long long)cap) have = (unsigned long long)cap;
    for (unsigned long long j = 0; j < have; ++j) {
        const size_t i = (size_t)((h->prof_calls - have + j) % n);
        SA_HIP(h, hipEventSynchronize(h->prof_stop[i]));
        SA_HIP(h, hipEventElapsedTime(&ms[j], h->prof_start[i], h->prof_stop[i]));
    }
    return (int)have;
}

int sa_flush(sa_handle *h, void *stream)
{
    if (!h) return SA_EINVAL;
    SA_HIP(h, hipSetDevice(h->device));
    for (sa_handle::Slot &s : h->slot)
        if (s.unjoined) {
            SA_HIP(h, hipStreamWaitEvent((hipStream_t)stream, s.done, 0));
            s.unjoined = false;
        }
    return SA_OK;
}

int sa_set_filter_mode(sa_handle *h, uint8_t cmd)
{
    if (!h) return SA_EINVAL;
    if (cmd != SA_FILTER_DEFAULT && cmd != SA_FILTER_CUSTOM && cmd != SA_FILTER_NONE && cmd != SA_FILTER_WIDE)
        return fail(h, SA_EINVAL, "sa_set_filter_mode: not a filter-select byte (0x00, 0xA1, 0xB1, 0xA2)");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    h->filter_mode = cmd;
    return SA_OK;
}

int sa_get_filter_mode(const sa_handle *h, uint8_t *cmd)
{
    if (!h || !cmd) return SA_EINVAL;
    *cmd = h->filter_mode;
    return SA_OK;
}

int sa_load_coeffs_q7(sa_handle *h, const int8_t c[12])
{
    if (!h) return SA_EINVAL;
    if (!c) return fail(h, SA_EINVAL, "sa_load_coeffs_q7: NULL coefficients");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    std::memcpy(h->c12_custom, c, 12);
    double sos[36];
    sos_from_q7(h->c12_custom, sos);
    return set_custom_plan(h, sos, 6);
}

int sa_get_coeffs_q7(const sa_handle *h, int8_t c[12])
{
    if (!h || !c) return SA_EINVAL;
    std::memcpy(c, h->c12_custom, 12);
    return SA_OK;
}

int sa_feed_command_bytes_ex(sa_handle *h, const uint8_t *bytes, size_t n, sa_cmd_events *ev)
{
    if (!h) return SA_EINVAL;
    if (!bytes && n) return fail(h, SA_EINVAL, "sa_feed_command_bytes: NULL bytes");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    for (size_t i = 0; i < n; ++i) {
        const uint8_t b = bytes[i];
        if (h->rx_count >= 0) {                      // ACQUIRE: busy, byte is a coefficient; neither command_control
            h->rx_buf[h->rx_count++] = (int8_t)b;    // nor sequ_2 sees it (uart_rx_valid and not busy,
            if (h->rx_count == 12) {                 // imp/dsp_system_top.vhd:644, new/command_control.vhd:51)
                h->rx_count = -1;
                const int rc = sa_load_coeffs_q7(h, h->rx_buf);
                if (rc != SA_OK) return rc;
                if (ev) { ++ev->n_uploads; ev->control_changed = 1; }
            }
            continue;
        }
        switch (b) {                                 // IDLE: command decode (command_control.vhd:53-62, sequ2.vhd:82-96)
            case SA_CMD_FILTER_UPDATE: h->rx_count = 0; break;
            case SA_FILTER_DEFAULT:
            case SA_FILTER_CUSTOM:
            case SA_FILTER_NONE:
                if (ev && h->filter_mode != b) ev->control_changed = 1;
                h->filter_mode = b;
                break;
            case SA_CMD_RESET: {                     // rst: mode B1 (:50), coefficients cleared (filter_iir12_cust.vhd:51-52),
                h->filter_mode = SA_FILTER_NONE;     // Ethernet transport (sequ2.vhd:85-86)
                h->transport = SA_CMD_ETHERNET_MODE;
                const int8_t z[12] = {0};
                const int rc = sa_load_coeffs_q7(h, z);
                if (rc != SA_OK) return rc;
                if (ev) { ++ev->n_reset; ev->control_changed = 1; }
                break;
            }
            case SA_CMD_ETHERNET_MODE:
            case SA_CMD_UART_MODE: h->transport = b; break;
            case SA_CMD_START: if (ev) ++ev->n_start; break;
            case SA_CMD_UART_REQUEST: if (ev) ++ev->n_uart_request; break;
            default: break;                          // unknown bytes: no effect, like the RTL
        }
    }
    if (ev) ev->transport = h->transport;
    return SA_OK;
}

int sa_feed_command_bytes(sa_handle *h, const uint8_t *bytes, size_t n, int *n_frames_requested)
{
    sa_cmd_events ev;
    std::memset(&ev, 0, sizeof ev);
    const int rc = sa_feed_command_bytes_ex(h, bytes, n, &ev);
    if (n_frames_requested) *n_frames_requested += ev.n_uart_request;
    return rc;
}

int sa_get_transport(const sa_handle *h, uint8_t *cmd)
{
    if (!h || !cmd) return SA_EINVAL;
    *cmd = h->transport;
    return SA_OK;
}

int sa_load_sos_f64(sa_handle *h, const double *sos, int n_sections)
{
    if (!h) return SA_EINVAL;
    if (!sos) return fail(h, SA_EINVAL, "sa_load_sos: NULL sos");
    if (n_sections < 0 || n_sections > SA_MAXSEC) return fail(h, SA_EINVAL, "sa_load_sos: 0..6 sections");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    double norm[36];
    if (!normalise_a0(sos, n_sections, norm)) return fail(h, SA_EINVAL, "sa_load_sos: a0 must be finite and non-zero");
    return set_custom_plan(h, norm, n_sections);
}

int sa_load_sos_f32(sa_handle *h, const float *sos, int n_sections)
{
    if (!h) return SA_EINVAL;
    if (!sos) return fail(h, SA_EINVAL, "sa_load_sos: NULL sos");
    if (n_sections < 0 || n_sections > SA_MAXSEC) return fail(h, SA_EINVAL, "sa_load_sos: 0..6 sections");
    double d[36];
    for (int i = 0; i < 6 * n_sections; ++i) d[i] = (double)sos[i];
    return sa_load_sos_f64(h, d, n_sections);
}

int sa_load_sos_q14(sa_handle *h, const int16_t *sos, int n_sections)
{
    if (!h) return SA_EINVAL;
    if (!sos) return fail(h, SA_EINVAL, "sa_load_sos_q14: NULL sos");
    if (n_sections < 0 || n_sections > SA_MAXSEC) return fail(h, SA_EINVAL, "sa_load_sos_q14: 0..6 sections");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    std::memset(h->sos_q14, 0, sizeof h->sos_q14);
    std::memcpy(h->sos_q14, sos, sizeof(int16_t) * 6 * n_sections);
    h->nsec_q14 = n_sections;
    return SA_OK;
}

int sa_set_window_q15(sa_handle *h, const int16_t *w)
{
    if (!h) return SA_EINVAL;
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    if (w) h->rom.assign(w, w + SA_NPTS); else default_rom(h->rom);
    return upload(h, h->d_rom, h->rom.data(), sizeof(int16_t) * SA_NPTS);
}

int sa_get_window_q15(const sa_handle *h, int16_t *w)
{
    if (!h || !w) return SA_EINVAL;
    std::memcpy(w, h->rom.data(), sizeof(int16_t) * SA_NPTS);
    return SA_OK;
}

int sa_set_window_f32(sa_handle *h, const float *w)
{
    if (!h) return SA_EINVAL;
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    if (w) {
        h->half_win.resize(SA_NPTS);
        for (int i = 0; i < SA_NPTS; ++i) h->half_win[i] = 0.5f * w[i];
        h->win_is_cos = fit_cosine_window(w, h->win_cos);
        h->win64.assign(w, w + SA_NPTS);                    // widened exactly
    } else {
        default_window(h);
    }
    return write_window(h, upload);
}

int sa_set_window_mode_q15(sa_handle *h, int mode)
{
    if (!h) return SA_EINVAL;
    if (mode != SA_WIN_RTL_SIGNED && mode != SA_WIN_HANN_U16) return fail(h, SA_EINVAL, "sa_set_window_mode_q15: bad mode");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    h->win_mode_q15 = mode;
    return SA_OK;
}

static SaQ15Params q15_params(const sa_handle *h)
{
    SaQ15Params p;
    std::memset(&p, 0, sizeof p);
    p.win_mode = h->win_mode_q15;
    p.filter = h->filter_mode;
    p.nsec_wide = h->nsec_q14;
    std::memcpy(p.c12, h->filter_mode == SA_FILTER_DEFAULT ? kDefaultQ7 : h->c12_custom, 12);
    std::memcpy(p.sos_q14, h->sos_q14, sizeof p.sos_q14);
    if (h->filter_mode == SA_FILTER_WIDE && h->nsec_q14 == 0) p.filter = SA_FILTER_NONE;   // no sections = wire
    return p;
}

// sa_filter_q15 (`fft` false: window + integer cascade into `out`, out_kind unused) and sa_process_q15 / sa_process_q15_out
// (`out` per out_kind, SA_Q15_OUT_*: the FFT launch's epilogue makes it); `fn` names the entry point
static int process_q15(sa_handle *h, const char *fn, const int16_t *in, void *out, int batch, int out_kind, void *stream,
                       bool fft)
{
    if (!h) return SA_EINVAL;
    if (batch < 0) return fail_at(h, SA_ESHAPE, fn, "negative batch");
    if (out_kind < SA_Q15_OUT_IQ || out_kind > SA_Q15_OUT_MARKER) return fail_at(h, SA_EINVAL, fn, "bad out_kind");
    if (batch == 0) return SA_OK;
    if (!in || !out) return fail_at(h, SA_EINVAL, fn, "NULL tensor");
    if (out_kind == SA_Q15_OUT_MARKER && ((uintptr_t)out & 15u) != 0)
        return fail_at(h, SA_EINVAL, fn, "SA_Q15_OUT_MARKER output must be 16-byte aligned");
    SA_HIP(h, hipSetDevice(h->device));
    const SaQ15Params p = q15_params(h);
    const bool staged = fft && p.filter != SA_FILTER_NONE;      // cascade into the slot's workspace, then the FFT
    CallCtx c;
    { const int rc = begin_call(h, (hipStream_t)stream, staged ? sa_handle::kWorkQ15 : -1, batch, &c); if (rc != SA_OK) return rc; }
    const SaQ15Tables t = {h->d_rom, h->d_twq, h->d_twrec, h->marker_lo, h->marker_hi};
    if (!staged) {
        SA_HIP(h, fft ? sa_launch_fft_q15(in, out, batch, out_kind, true, p, t, c.stream, {c.start, c.stop})
                      : sa_launch_filter_q15(in, (int16_t *)out, batch, p, t, c.stream, {c.start, c.stop}));
        return end_call(h, c);
    }
    // The WIDE cascade does not gain from overlapped launches (tools/q15_overlap_modes.py, profiles/r4_q15_helper_waves.txt):
    // its step is made of packed dot products, the integer FFT's twiddle products are too, and side by side the two starve
    // each other -- 7.5-7.9 M frames/s at depth 2 when left free against 8.3 M stream-ordered.  At depth 2 its cascade
    // therefore waits for the previous call of the handle (8.0 M; at depth 3 it runs free: 7.9-8.2 M).
    if (c.overlapped && p.filter == SA_FILTER_WIDE && h->overlap == 2) {
        const sa_handle::Slot &prev = h->slot[(c.slot + h->overlap - 1) % h->overlap];
        if (prev.used) SA_HIP(h, hipStreamWaitEvent(c.stream, prev.done, 0));
    }
    int16_t *ws = (int16_t *)h->slot[c.slot].work[sa_handle::kWorkQ15].ptr;
    SA_HIP(h, sa_launch_filter_q15(in, ws, batch, p, t, c.stream, {c.start, nullptr}));
    SA_HIP(h, sa_launch_fft_q15(ws, out, batch, out_kind, false, p, t, c.stream, {nullptr, c.stop}));
    return end_call(h, c);
}

int sa_filter_q15(sa_handle *h, const int16_t *in, int16_t *out_time, int batch, void *stream)
{
    return process_q15(h, "sa_filter_q15", in, out_time, batch, SA_Q15_OUT_IQ, stream, false);
}

int sa_process_q15(sa_handle *h, const int16_t *in, int16_t *out_iq, int batch, void *stream)
{
    return process_q15(h, "sa_process_q15", in, out_iq, batch, SA_Q15_OUT_IQ, stream, true);
}

int sa_process_q15_out(sa_handle *h, const int16_t *in, void *out, int batch, int out_kind, void *stream)
{
    return process_q15(h, "sa_process_q15_out", in, out, batch, out_kind, stream, true);
}

// sa_process_f32 (float frames) and sa_process_f32_i16 (int16 samples times `scale`); `fn` names the entry point.
// The float32 path: one launch of the fused chain.  The section coefficients and predictor taps travel by value in the
// kernel arguments (stream-ordered by construction); the per-lane matrices and the window live in device memory
// (stream-ordered uploads).
// The float64-state path (SA_PRECISION_F64_STATE with a cascade: DEFAULT, or CUSTOM with at least one section):
// iir_f64.hip (window + cascade in double, y rounded once) into the slot's workspace, then the bypassed float chain on
// y with the constant 1/2 window (exact).  SA_OUT_TIME is the first launch alone, into `out`.  Timed as one call: the
// start event rides on the first kernel, the stop event on the last.
static int process_float(sa_handle *h, const char *fn, const void *in, bool i16, float scale, void *out, int batch,
                         int out_kind, void *stream)
{
    if (!h) return SA_EINVAL;
    if (batch < 0) return fail_at(h, SA_ESHAPE, fn, "negative batch");
    if (out_kind < SA_OUT_MAG_FULL || out_kind > SA_OUT_MARKER) return fail_at(h, SA_EINVAL, fn, "bad out_kind");
    if (!(scale == scale) || scale - scale != 0.f) return fail_at(h, SA_EINVAL, fn, "scale is not finite");
    if (batch == 0) return SA_OK;
    if (!in || !out) return fail_at(h, SA_EINVAL, fn, "NULL tensor");
    if (out_kind == SA_OUT_MARKER && ((uintptr_t)out & 15u) != 0)
        return fail_at(h, SA_EINVAL, fn, "SA_OUT_MARKER output must be 16-byte aligned");
    if (h->filter_mode == SA_FILTER_WIDE)
        return fail_at(h, SA_ESTATE, fn, "filter mode 0xA2 (Q2.14) belongs to the Q15 path; use 0xA1 with sa_load_sos_f32");
    SA_HIP(h, hipSetDevice(h->device));
    const sa_handle::Plan &pl = active_plan(h);
    const bool cascade = h->filter_mode != SA_FILTER_NONE;
    const bool f64 = h->precision == SA_PRECISION_F64_STATE && cascade && pl.k.nsec > 0;
    const bool two = f64 && out_kind != SA_OUT_TIME;
    CallCtx c;
    { const int rc = begin_call(h, (hipStream_t)stream, two ? sa_handle::kWorkF64 : -1, batch, &c); if (rc != SA_OK) return rc; }
    SaF32Tables t = {h->d_win_b, h->d_win_t, h->d_twT, h->d_twB, h->d_twC, pl.d_lt, cascade ? &pl.k : nullptr,
                     h->marker_lo, h->marker_hi};
    if (!f64) {
        SA_HIP(h, i16 ? sa_launch_chain_f32_i16((const int16_t *)in, scale, out, batch, out_kind, t, c.stream, {c.start, c.stop})
                      : sa_launch_chain_f32((const float *)in, out, batch, out_kind, t, c.stream, {c.start, c.stop}));
        return end_call(h, c);
    }
    float *y = two ? (float *)h->slot[c.slot].work[sa_handle::kWorkF64].ptr : (float *)out;
    SA_HIP(h, sa_launch_iir_f64(in, i16, scale, y, batch, pl.k.nsec, pl.d_p64, h->d_win64, c.stream,
                                {c.start, two ? nullptr : c.stop}));
    if (two) {
        t = {h->d_win_half, h->d_win_t, h->d_twT, h->d_twB, h->d_twC, h->plan_custom.d_lt, nullptr, h->marker_lo, h->marker_hi};
        SA_HIP(h, sa_launch_chain_f32(y, out, batch, out_kind, t, c.stream, {nullptr, c.stop}));
    }
    return end_call(h, c);
}

int sa_process_f32(sa_handle *h, const float *in, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, "sa_process_f32", in, false, 1.f, out, batch, out_kind, stream);
}

int sa_process_f32_i16(sa_handle *h, const int16_t *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, "sa_process_f32_i16", in, true, scale, out, batch, out_kind, stream);
}

int sa_pack_frame(const int16_t *iq_host, uint8_t *frame_bytes)
{
    if (!iq_host || !frame_bytes) return SA_EINVAL;
    for (int i = 0; i < SA_NPTS * 2; ++i) {          // explicit little-endian, independent of the host
        const uint16_t v = (uint16_t)iq_host[i];
        frame_bytes[2 * i] = (uint8_t)(v & 0xFF);
        frame_bytes[2 * i + 1] = (uint8_t)(v >> 8);
    }
    return SA_OK;
}

int sa_debug_iir_plan_f32(const sa_handle *h, float *out, int cap)
{
    if (!h) return SA_EINVAL;
    const sa_handle::Plan &pl = active_plan(h);
    return export_plan(pl.k, pl.lt, out, cap);
}

int sa_iir_plan_from_sos(const double *sos, int n_sections, float *out, int cap)
{
    if (!sos || n_sections < 0 || n_sections > SA_MAXSEC) return SA_EINVAL;
    double norm[36];
    if (!normalise_a0(sos, n_sections, norm)) return SA_EINVAL;
    SaIirK p;
    std::vector<SaIirLaneTab> lt(1);
    build_plan(norm, n_sections, &p, &lt[0], nullptr);
    return export_plan(p, lt[0], out, cap);
}

int sa_set_precision(sa_handle *h, int precision)
{
    if (!h) return SA_EINVAL;
    if (precision != SA_PRECISION_F32 && precision != SA_PRECISION_F64_STATE)
        return fail(h, SA_EINVAL, "sa_set_precision: SA_PRECISION_F32 (0) or SA_PRECISION_F64_STATE (1)");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    if (precision == h->precision) return SA_OK;
    if (precision == SA_PRECISION_F32) {        // the float64 tables and workspaces are kept (hipFree synchronises the device)
        h->precision = precision;
        return SA_OK;
    }
    SA_HIP(h, hipSetDevice(h->device));
    for (sa_handle::Plan *pl : {&h->plan_default, &h->plan_custom})
        if (!pl->d_p64) SA_HIP(h, hipMalloc(&pl->d_p64, sizeof(SaIirF64)));
    if (!h->d_win64) SA_HIP(h, hipMalloc(&h->d_win64, sizeof(double) * SA_NPTS));
    if (!h->d_win_half) SA_HIP(h, hipMalloc(&h->d_win_half, sizeof(float) * SA_NPTS));
    // the FFT launch's window: 1/2 everywhere, laid out by the code that lays out the handle's own window table
    std::vector<float> half(SA_NPTS, 0.5f), pa;
    pass_a_window(half, pa);
    int rc = upload(h, h->d_win_half, pa.data(), sizeof(float) * SA_NPTS);
    if (rc == SA_OK) rc = sync_f64(h, true, /*force=*/true);      // tables were not kept up to date outside the mode
    if (rc == SA_OK) rc = grow_slots(h, h->overlap, h->reserved_max, /*geometric=*/false, /*f64_only=*/true);
    if (rc != SA_OK) return rc;
    h->precision = precision;
    return SA_OK;
}

int sa_get_precision(const sa_handle *h, int *precision)
{
    if (!h || !precision) return SA_EINVAL;
    *precision = h->precision;
    return SA_OK;
}

int sa_set_marker_range(sa_handle *h, int lo, int hi)
{
    if (!h) return SA_EINVAL;
    if (lo < 0 || lo >= hi || hi > SA_NPTS) return fail(h, SA_EINVAL, "sa_set_marker_range: need 0 <= lo < hi <= 16384");
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    h->marker_lo = lo;
    h->marker_hi = hi;
    return SA_OK;
}

int sa_get_marker_range(const sa_handle *h, int *lo, int *hi)
{
    if (!h || !lo || !hi) return SA_EINVAL;
    *lo = h->marker_lo;
    *hi = h->marker_hi;
    return SA_OK;
}

int sa_debug_iir_plan_f64(const sa_handle *h, double *out, int cap)
{
    if (!h || cap < 0) return SA_EINVAL;
    const sa_handle::Plan &pl = active_plan(h);
    SaIirF64 p;
    build_plan_f64(pl.sos, pl.nsec, &p);
    if (out && cap > 0) std::memcpy(out, &p, sizeof(double) * (size_t)(cap < kSaIirF64Doubles ? cap : kSaIirF64Doubles));
    return kSaIirF64Doubles;
}

int sa_iir_plan_from_sos_f64(const double *sos, int n_sections, double *out, int cap)
{
    if (!sos || n_sections < 0 || n_sections > SA_MAXSEC || cap < 0) return SA_EINVAL;
    double norm[36];
    if (!normalise_a0(sos, n_sections, norm)) return SA_EINVAL;
    SaIirF64 p;
    build_plan_f64(norm, n_sections, &p);
    if (out && cap > 0) std::memcpy(out, &p, sizeof(double) * (size_t)(cap < kSaIirF64Doubles ? cap : kSaIirF64Doubles));
    return kSaIirF64Doubles;
}

}  // extern "C"
