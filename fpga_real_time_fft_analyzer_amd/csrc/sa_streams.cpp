// sa_streams.cpp -- launch and upload ordering of a handle: which stream a process call runs on and what it waits for
// (begin_call / end_call), the stream-ordered table uploads, the launch slots' workspaces, overlapped launches with
// their stream probe, the capture record and the launch-timing ring, with the entry points that only drive them.
// No device-wide synchronisation anywhere; the state it keeps is described in sa_handle.hpp.
#include "sa_handle.hpp"

#include <algorithm>
#include <cstring>

namespace {

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

// Workspace `w` grown to `frames` without touching launches in flight (see sa_handle::Workspace).
// `geometric`: grow by at least half (process calls with creeping batch sizes); exact sizing where the size is copied
// from another slot -- sa_set_overlap gave every slot max(the others, 1.5 x its own), and two slots leap-frogged each
// other by a factor 1.5 per mode change until hipMalloc failed (found by a 10-minute soak, seed 77).
// `on_demand`: null, or for a workspace sa_reserve does not size (kWorkTraceRaw, kWorkSpectra) the refusal inside a capture,
// which names the other remedy.
int ensure_work(sa_handle *h, sa_handle::Workspace &w, int frames, bool captured, bool geometric = true,
                const char *on_demand = nullptr)
{
    if (frames <= w.frames) return SA_OK;
    if (captured)
        return fail(h, SA_ESTATE, on_demand ? on_demand : "workspace growth inside a stream capture: call sa_reserve() first");
    long want = frames, geo = (long)w.frames + w.frames / 2;
    if (geometric && geo > want) want = geo;
    void *p = nullptr;
    SA_HIP(h, hipMalloc(&p, (size_t)want * SA_NPTS * w.elem));
    if (w.ptr) h->retired.push_back(w.ptr);
    w.ptr = p;
    w.frames = (int)want;
    return SA_OK;
}

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

// the capture the sticky record (sa_handle::capture_open) stands for has ended
void capture_closed(sa_handle *h)
{
    h->capture_open = false;
    h->capture_stream = nullptr;
}

}  // namespace

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
    capture_closed(h);
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

// The workspaces of slots 0..n-1 that the handle's precision launches with (`f64_only`: the float64-state one alone)
// grown to `frames`; frames < 0: exactly to the largest of that kind any slot has (slots new to overlap mode start with
// what the handle already has somewhere)
int grow_slots(sa_handle *h, int n, int frames, bool geometric, bool f64_only)
{
    const int k0 = f64_only ? sa_handle::kWorkF64 : sa_handle::kWorkQ15;
    const int k1 = f64_only || h->precision == SA_PRECISION_F64_STATE ? sa_handle::kWorkF64 + 1 : sa_handle::kWorkF64;
    static_assert(sa_handle::kWorkQ15 == 0 && sa_handle::kWorkF64 == 1, "the two kinds sized here; kWorkTraceRaw and kWorkSpectra grow on demand");
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

// Steps 1 and 2 of a process call: (1) decide -- capture query (it also keeps the sticky capture record), stream, slot,
// growth of the slot's workspace `work` to `frames` (work < 0: none) and of a second one, `work2` to `frames2`, for the
// calls that need two; (2) enqueue the ordering waits.  The caller
// launches (3) and commits with end_call (4) only when every launch succeeded: a call that fails leaves `launched`,
// the profiling ring and the join state on the last launch that did happen.
int begin_call(sa_handle *h, hipStream_t user, int work, int frames, CallCtx *c, int work2, int frames2)
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
        capture_closed(h);                   // that stream's capture has ended
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
    if (work2 >= 0) {
        const char *remedy =
            work2 == sa_handle::kWorkTraceRaw  ? "workspace growth inside a stream capture: make one SA_Q15_TRACE_AVG_KIND call of this "
                                                 "bucket width and batch outside the capture first (sa_reserve does not size it)"
            : work2 == sa_handle::kWorkSpectra ? "workspace growth inside a stream capture: make one sa_spectra_q15 call of this batch "
                                                 "outside the capture first (sa_reserve does not size it)"
                                               : nullptr;
        const int rc = ensure_work(h, h->slot[c->slot].work[work2], frames2, c->captured, true, remedy);
        if (rc != SA_OK) return rc;
    }
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

extern "C" {

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

}  // extern "C"
