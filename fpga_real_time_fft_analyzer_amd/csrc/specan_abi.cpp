// specan_abi.cpp -- host side of the C ABI declared in include/specan.h.
//
// Owns: the handle's creation and destruction, its device tables (window and twiddles: filled by sa_tables.cpp; IIR
// plans: built by iir_plan.cpp), the setters, the process paths and the command-byte state machine that mirrors
// new/rx_filter_coeff.vhd + new/command_control.vhd.  The handle itself is sa_handle.hpp; how its launches and uploads
// are ordered is sa_streams.cpp.
// Never touches caller tensors except through the pointers given to the process calls, never
// falls back to CPU compute.
#include "iir_plan.hpp"
#include "sa_handle.hpp"
#include "sa_pointers.hpp"
#include "sa_tables.hpp"

#include "../../include/specan_ext.h"

#include <array>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <utility>

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

namespace {

// The default window, Hann (scripts/hann_coeff.py:3-4): in double, its float half, and the cosine form set to
// (0.5, 0.5) exactly (not fitted: a fitted (a0, a1) would change the bits of the generated window)
void default_window(sa_handle *h)
{
    default_window_f64(h->win64);
    half_window(h->win64, h->half_win);
    h->win_is_cos = true;
    h->win_cos[0] = h->win_cos[1] = 0.5;
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

// Every device table of the handle.  sa_create allocates the first kTablesAtCreate, the first
// sa_set_precision(F64_STATE) the rest; sa_destroy frees them all (a null pointer, as in a partially created handle or
// one that never entered the float64-state mode, is skipped by hipFree).
struct DevTable {
    void **ptr;
    size_t bytes;
};
constexpr int kTablesAtCreate = 10, kTables = 14;

std::array<DevTable, kTables> device_tables(sa_handle *h)
{
    return {{{(void **)&h->d_win_b, sizeof(float) * SA_NPTS},
             {(void **)&h->d_win_t, sizeof(float) * SA_NPTS},
             {(void **)&h->d_twT, sizeof(float4) * 6 * 256},
             {(void **)&h->d_twB, sizeof(float4) * 8 * 16},
             {(void **)&h->d_twC, sizeof(float2) * 25},
             {(void **)&h->plan_default.d_lt, sizeof(SaIirLaneTab)},
             {(void **)&h->plan_custom.d_lt, sizeof(SaIirLaneTab)},
             {(void **)&h->d_rom, sizeof(int16_t) * SA_NPTS},
             {(void **)&h->d_twq, sizeof(uint2) * SA_NPTS},
             {(void **)&h->d_twrec, sizeof(uint4) * 2 * kSaTwRecs},
             // float64-state mode
             {(void **)&h->plan_default.d_p64, sizeof(SaIirF64)},
             {(void **)&h->plan_custom.d_p64, sizeof(SaIirF64)},
             {(void **)&h->d_win64, sizeof(double) * SA_NPTS},
             {(void **)&h->d_win_half, sizeof(float) * SA_NPTS}}};
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
    // destroyed again on every early return below: sa_destroy takes a partially created handle
    std::unique_ptr<sa_handle, int (*)(sa_handle *)> guard(new (std::nothrow) sa_handle(), sa_destroy);
    sa_handle *h = guard.get();
    if (!h) return fail(nullptr, SA_ENOMEM, "sa_create: out of host memory");
    h->device = device;
    SA_HIP(nullptr, hipSetDevice(device));
    SA_HIP(nullptr, hipStreamCreateWithFlags(&h->ctl, hipStreamNonBlocking));
    SA_HIP(nullptr, hipEventCreateWithFlags(&h->launched_own, hipEventDisableTiming));
    h->launched = h->launched_own;
    SA_HIP(nullptr, hipEventCreateWithFlags(&h->uploaded, hipEventDisableTiming));
    for (sa_handle::Stage &st : h->stage) {
        SA_HIP(nullptr, hipHostMalloc(&st.buf, kStageBytes, hipHostMallocDefault));
        SA_HIP(nullptr, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    }
    const auto tables = device_tables(h);
    for (int i = 0; i < kTablesAtCreate; ++i) SA_HIP(nullptr, hipMalloc(tables[i].ptr, tables[i].bytes));

    // float tables: the default window and the IIR plans (default = the fixed ALPHA/BETA cascade as real taps;
    // custom = cleared coefficients), then the twiddles
    sos_from_q7(kDefaultQ7, h->plan_default.sos);
    sos_from_q7(h->c12_custom, h->plan_custom.sos);
    h->plan_default.nsec = h->plan_custom.nsec = 6;
    default_window(h);
    if (write_window(h, copy_at_create) != SA_OK) return SA_EHIP;
    std::vector<float4> ta, tb;
    std::vector<float2> tc;
    float_twiddles(ta, tb, tc);
    SA_HIP(nullptr, hipMemcpy(h->d_twT, ta.data(), sizeof(float4) * ta.size(), hipMemcpyHostToDevice));
    SA_HIP(nullptr, hipMemcpy(h->d_twB, tb.data(), sizeof(float4) * tb.size(), hipMemcpyHostToDevice));
    SA_HIP(nullptr, hipMemcpy(h->d_twC, tc.data(), sizeof(float2) * tc.size(), hipMemcpyHostToDevice));
    // integer tables
    default_rom(h->rom);
    SA_HIP(nullptr, hipMemcpy(h->d_rom, h->rom.data(), sizeof(int16_t) * SA_NPTS, hipMemcpyHostToDevice));
    std::vector<uint2> tq;
    std::vector<uint4> rec;
    if (!q15_twiddles(tq, rec))
        return fail(nullptr, SA_ESTATE, "sa_create: twiddle table: wi = -32768 outside exponents 4082..4110");
    SA_HIP(nullptr, hipMemcpy(h->d_twq, tq.data(), sizeof(uint2) * SA_NPTS, hipMemcpyHostToDevice));
    SA_HIP(nullptr, hipMemcpy(h->d_twrec, rec.data(), sizeof(uint4) * 2 * kSaTwRecs, hipMemcpyHostToDevice));
    SA_HIP(nullptr, hipDeviceSynchronize());          // creation only: the blocking copies above are complete
    *out = guard.release();
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
    for (const DevTable &t : device_tables(h)) (void)hipFree(*t.ptr);
    for (void *p : h->retired) (void)hipFree(p);
    delete h;
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

// the argument checks of sa_load_sos_f64 and sa_load_sos_f32
static int check_sos(sa_handle *h, const void *sos, int n_sections)
{
    if (!h) return SA_EINVAL;
    if (!sos) return fail(h, SA_EINVAL, "sa_load_sos: NULL sos");
    if (n_sections < 0 || n_sections > SA_MAXSEC) return fail(h, SA_EINVAL, "sa_load_sos: 0..6 sections");
    return SA_OK;
}

int sa_load_sos_f64(sa_handle *h, const double *sos, int n_sections)
{
    { const int rc = check_sos(h, sos, n_sections); if (rc != SA_OK) return rc; }
    { const int rc = control_allowed(h); if (rc != SA_OK) return rc; }
    double norm[36];
    if (!normalise_a0(sos, n_sections, norm)) return fail(h, SA_EINVAL, "sa_load_sos: a0 must be finite and non-zero");
    return set_custom_plan(h, norm, n_sections);
}

int sa_load_sos_f32(sa_handle *h, const float *sos, int n_sections)
{
    { const int rc = check_sos(h, sos, n_sections); if (rc != SA_OK) return rc; }
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

// The argument checks of process_q15 and process_float, made before anything else; callers of the ABI see their order.
// The output kinds of both chains run from 0 to `marker`, the marker records (`marker_name` in the message).
// `trace`: the entry point also takes the SA_Q15_TRACE_KIND(k) family (the Q15 FFT calls; never the float chain).
// `grouped`: it also takes SA_Q15_TRACE_AVG_KIND(k, a) -- the two entry points with a kind word alone; a batch that is no
// multiple of A = 2^a is SA_ESHAPE, after the kind and before the pointers.
// `scale_finite`: what process_float found of its scale, which is refused between the kind and the empty batch (process_q15
// has no scale: true).  An empty batch returns SA_OK here, and the caller returns it at once.
// `hop`: null, or where the entry point's word is a SA_Q15_HOP_KIND: the word is taken apart before anything else, *hop is
// its hop in samples (0: frames) and the kind checked below is its low byte.  An entry point without one (every float one)
// sees a word with a hop field as the unknown kind it is there.
// Last, the pointer contract of include/specan.h: `chain` names the family of outputs, sa_pointers.cpp holds the rule.  The
// alignment rules that were there before it (marker and trace `out`, packed `in`, a stream `in`) are instances of it and
// keep their messages; all of this before any call state exists.
static int check_process_args(sa_handle *h, const char *fn, const void *in, SaInKind kind, const void *out, int batch,
                              int out_kind, SaChain chain, int marker, const char *marker_name, bool trace, bool scale_finite,
                              int *hop = nullptr, bool grouped = false)
{
    static_assert((int)SaInKind::F32 == kSaInF32 && (int)SaInKind::I16 == kSaInI16 && (int)SaInKind::P12 == kSaInP12,
                  "sa_pointers.hpp numbers the input forms as SaInKind does");
    static_assert(SA_OUT_MAG_FULL == 0 && SA_Q15_OUT_IQ == 0, "the kinds of both chains are 0 .. marker");
    int field = 0;
    bool bad_word = false;
    if (hop && out_kind >= 0) {                                    // a negative word is the bad kind it always was
        field = (out_kind >> 8) & 0xFFF;
        bad_word = (out_kind >> 20) != 0 || field > SA_Q15_HOP_FIELD_MAX;
        out_kind &= 0xFF;
    }
    if (!h) return SA_EINVAL;
    if (batch < 0) return fail_at(h, SA_ESHAPE, fn, "negative batch");
    if (bad_word) return fail_at(h, SA_EINVAL, fn, "bad out_kind: hop field above 2048 or bits 20..30 set");
    const bool is_trace = trace && out_kind >= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MIN) &&
                          out_kind <= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MAX);
    const bool is_avg = grouped && out_kind >= 0 && SA_Q15_IS_TRACE_AVG_KIND(out_kind);
    if (!is_trace && !is_avg && (out_kind < 0 || out_kind > marker)) return fail_at(h, SA_EINVAL, fn, "bad out_kind");
    if (!scale_finite) return fail_at(h, SA_EINVAL, fn, "scale is not finite");
    if (batch == 0) return SA_OK;
    if (is_avg && batch % sa_frames_per_row(chain, out_kind))
        return fail_at(h, SA_ESHAPE, fn, "SA_Q15_TRACE_AVG_KIND: batch must be a multiple of the group size A");
    if (!in || !out) return fail_at(h, SA_EINVAL, fn, "NULL tensor");
    SaCallSpan span;
    if (!sa_call_span(chain, (int)kind, out_kind, 8 * field, batch, &span)) return fail_at(h, SA_EINVAL, fn, "bad out_kind");
    const unsigned faults = sa_pointer_faults(span, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out);
    char msg[96];
    if ((out_kind == marker || is_trace || is_avg) && (faults & kSaPtrOutAlign)) {
        std::snprintf(msg, sizeof msg, "%s output must be 16-byte aligned",
                      is_avg ? "SA_Q15_TRACE_AVG_KIND" : is_trace ? "SA_Q15_TRACE_KIND" : marker_name);
        return fail_at(h, SA_EINVAL, fn, msg);
    }
    if (faults & kSaPtrInAlign)       // the stage-ins and tile loads issue 16-byte requests; every frame is then aligned (int16
        return fail_at(h, SA_EINVAL, fn,     // streams: 16 h bytes apart; packed streams need a dword per frame and have it)
                       kind == SaInKind::P12 ? "packed input must be 16-byte aligned"
                       : field != 0          ? "a sample stream (SA_Q15_HOP_KIND) must be 16-byte aligned"
                                             : "`in` must be 16-byte aligned");
    if (faults & kSaPtrOutAlign) {
        std::snprintf(msg, sizeof msg, "`out` must be %u-byte aligned", span.out_align);
        return fail_at(h, SA_EINVAL, fn, msg);
    }
    if (faults & kSaPtrOverlap) {
        std::snprintf(msg, sizeof msg, "`in` (%llu bytes read) and `out` (%llu bytes written) overlap",
                      (unsigned long long)span.in_bytes, (unsigned long long)span.out_bytes);
        return fail_at(h, SA_EINVAL, fn, msg);
    }
    if (hop) *hop = 8 * field;
    return SA_OK;
}

// What a Q15 call launches behind its FFT: nothing, the fold of SA_Q15_TRACE_AVG_KIND(k, a)'s partial records
// (trace_fold_q15.hip), or the bin-by-bin fold of sa_spectra_q15's IQ frames (spectra_fold_q15.hip, include/specan_ext.h).
// With a fold the FFT launch writes into a workspace of the slot and the fold writes `out`.
struct Q15Fold {
    enum What { None, Trace, Spectra } what;
    int log2w, log2a;
};

// The launches of a Q15 call whose arguments have passed their checks (batch > 0): sa_filter_q15 (`fft` false: window +
// integer cascade into `out`, out_kind unused), sa_process_q15 / sa_process_q15_out (`out` per out_kind, SA_Q15_OUT_* or
// SA_Q15_TRACE_KIND(k): the FFT launch's epilogue makes it; SA_Q15_TRACE_AVG_KIND(k, a): the epilogue's partial records and a
// fold launch behind it) and sa_spectra_q15 (out_kind SA_Q15_OUT_IQ into a workspace and its fold behind it), on int16 samples
// or on packed 12-bit samples (`kind`: I16 or P12); `fn` names the entry point.  With a hop, `in` is one stream and whichever
// launch reads the samples -- the cascade, or the FFT in mode 0xB1 -- is its _hop sibling.  Everything else is the frame call.
static int launch_q15(sa_handle *h, const char *fn, const void *in, SaInKind kind, void *out, int batch, int out_kind,
                      void *stream, bool fft, int hop, Q15Fold fold)
{
    SA_HIP(h, hipSetDevice(h->device));
    const SaQ15Params p = q15_params(h);
    const bool staged = fft && p.filter != SA_FILTER_NONE;      // cascade into the slot's workspace, then the FFT
    // SA_Q15_TRACE_AVG_KIND(k, a): the FFT launch writes partial records [B, 16384 >> k] into a workspace of its own and one
    // more launch folds them into `out`.  B (16384 >> k) records of kSaTraceRawBytes are ceil(16 B / W) "frames" of the
    // workspace's one-byte elements.  sa_spectra_q15: the FFT launch writes B IQ frames into a workspace of 4-byte elements.
    // Grown here, on demand, with the cascade's workspace and before the first launch; never by sa_reserve, which does not
    // know W and sizes nothing for a call the handle may never make.
    const bool folded = fold.what != Q15Fold::None;
    const int work2 = fold.what == Q15Fold::Trace ? sa_handle::kWorkTraceRaw : folded ? sa_handle::kWorkSpectra : -1;
    const long long frames2 = fold.what == Q15Fold::Trace ? ((long long)batch * kSaTraceRawBytes + (1 << fold.log2w) - 1) >> fold.log2w
                              : folded                    ? batch
                                                          : 0;
    if (frames2 > 0x7FFFFFFF) return fail_at(h, SA_ESHAPE, fn, "SA_Q15_TRACE_AVG_KIND: batch too large for the workspace");
    CallCtx c;
    { const int rc = begin_call(h, (hipStream_t)stream, staged ? sa_handle::kWorkQ15 : -1, batch, &c, work2, (int)frames2);
      if (rc != SA_OK) return rc; }
    const SaQ15Tables t = {h->d_rom, h->d_twq, h->d_twrec, h->marker_lo, h->marker_hi};
    // what the FFT launch writes, and the event its completion is bound to: the fold launch, where there is one, is the call's last
    void *fft_out = folded ? h->slot[c.slot].work[work2].ptr : out;
    hipEvent_t fft_stop = folded ? nullptr : c.stop;
    const auto launch_fold = [&]() {
        return fold.what == Q15Fold::Trace
                   ? sa_launch_trace_fold_q15(fft_out, out, batch, fold.log2w, fold.log2a, c.stream, {nullptr, c.stop})
                   : sa_launch_spectra_fold_q15(fft_out, out, batch, fold.log2a, c.stream, {nullptr, c.stop});
    };
    if (!staged) {
        SA_HIP(h, hop   ? sa_launch_fft_q15_hop(in, kind, hop, fft_out, batch, out_kind, p, t, c.stream, {c.start, fft_stop})
                  : fft ? sa_launch_fft_q15(in, kind, fft_out, batch, out_kind, true, p, t, c.stream, {c.start, fft_stop})
                        : sa_launch_filter_q15(in, kind, (int16_t *)out, batch, p, t, c.stream, {c.start, c.stop}));
        if (folded) SA_HIP(h, launch_fold());
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
    // the packed form is read by the first launch alone: the workspace holds int16 samples whatever came in
    SA_HIP(h, hop ? sa_launch_filter_q15_hop(in, kind, hop, ws, batch, p, t, c.stream, {c.start, nullptr})
                  : sa_launch_filter_q15(in, kind, ws, batch, p, t, c.stream, {c.start, nullptr}));
    SA_HIP(h, sa_launch_fft_q15(ws, SaInKind::I16, fft_out, batch, out_kind, false, p, t, c.stream, {nullptr, fft_stop}));
    if (folded) SA_HIP(h, launch_fold());
    return end_call(h, c);
}

// sa_filter_q15 (`fft` false), sa_process_q15 / sa_process_q15_out and their _p12 siblings: the argument checks, then
// launch_q15.  `hop_word`: out_kind is a SA_Q15_HOP_KIND (sa_process_q15_out, sa_process_q15_p12).
static int process_q15(sa_handle *h, const char *fn, const void *in, SaInKind kind, void *out, int batch, int out_kind,
                       void *stream, bool fft, bool hop_word = false)
{
    int hop = 0;
    { const int rc = check_process_args(h, fn, in, kind, out, batch, out_kind, fft ? SaChain::Q15 : SaChain::Q15Filter,
                                        SA_Q15_OUT_MARKER, "SA_Q15_OUT_MARKER", fft, true, hop_word ? &hop : nullptr, hop_word);
      if (rc != SA_OK || batch == 0) return rc; }
    if (hop_word) out_kind &= 0xFF;
    const bool avg = hop_word && SA_Q15_IS_TRACE_AVG_KIND(out_kind);
    const Q15Fold fold = {avg ? Q15Fold::Trace : Q15Fold::None, SA_Q15_TRACE_AVG_LOG2W(out_kind), SA_Q15_TRACE_AVG_LOG2A(out_kind)};
    return launch_q15(h, fn, in, kind, out, batch, out_kind, stream, fft, hop, fold);
}

// The calls of include/specan_ext.h.  Every refusal comes from sa_ext_check (sa_pointers.cpp) before any call state exists.
static int ext_q15(sa_handle *h, const char *fn, int entry, const void *in, void *out, int batch, int log2a, int hop, void *stream)
{
    if (!h) return SA_EINVAL;
    SaExtWhy why;
    SaCallSpan span;
    const int rc = sa_ext_check(entry, log2a, hop, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, batch, &why, &span);
    if (rc != SA_OK) {
        char msg[112];
        const char *what = msg;
        switch (why) {
            case kSaExtBatch: what = "negative batch"; break;
            case kSaExtLog2a: what = "log2a must be 1..7 (groups of A = 2..128 frames)"; break;
            case kSaExtHop:
                what = entry == SA_EXT_ENTRY_FOLD_IQ_Q15 ? "the fold takes frames: no hop" : "hop must be 0 or a multiple of 8 in 8..16384";
                break;
            case kSaExtGroup: what = "batch must be a multiple of the group size A"; break;
            case kSaExtNull: what = "NULL tensor"; break;
            case kSaExtInAlign:
                what = entry == SA_EXT_ENTRY_SPECTRA_Q15_P12 ? "packed input must be 16-byte aligned"
                       : hop != 0                            ? "a sample stream must be 16-byte aligned"
                                                             : "`in` must be 16-byte aligned";
                break;
            case kSaExtOutAlign: what = "`out` must be 16-byte aligned"; break;
            case kSaExtOverlap:
                std::snprintf(msg, sizeof msg, "`in` (%llu bytes read) and `out` (%llu bytes written) overlap",
                              (unsigned long long)span.in_bytes, (unsigned long long)span.out_bytes);
                break;
            default: what = "bad argument"; break;
        }
        return fail_at(h, rc, fn, what);
    }
    if (batch == 0) return SA_OK;
    if (entry != SA_EXT_ENTRY_FOLD_IQ_Q15)
        return launch_q15(h, fn, in, entry == SA_EXT_ENTRY_SPECTRA_Q15_P12 ? SaInKind::P12 : SaInKind::I16, out, batch, SA_Q15_OUT_IQ,
                          stream, true, hop, {Q15Fold::Spectra, 0, log2a});
    SA_HIP(h, hipSetDevice(h->device));                          // the fold alone: one launch, no workspace
    CallCtx c;
    { const int rc2 = begin_call(h, (hipStream_t)stream, -1, batch, &c); if (rc2 != SA_OK) return rc2; }
    SA_HIP(h, sa_launch_spectra_fold_q15(in, out, batch, log2a, c.stream, {c.start, c.stop}));
    return end_call(h, c);
}

int sa_ext_version(void) { return SA_EXT_VERSION; }

int sa_spectra_q15(sa_handle *h, const int16_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream)
{
    return ext_q15(h, "sa_spectra_q15", SA_EXT_ENTRY_SPECTRA_Q15, in, out, batch, log2a, hop, stream);
}

int sa_spectra_q15_p12(sa_handle *h, const uint8_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream)
{
    return ext_q15(h, "sa_spectra_q15_p12", SA_EXT_ENTRY_SPECTRA_Q15_P12, in, out, batch, log2a, hop, stream);
}

int sa_fold_iq_q15(sa_handle *h, const int16_t *iq, sa_trace_point_q15 *out, int batch, int log2a, void *stream)
{
    return ext_q15(h, "sa_fold_iq_q15", SA_EXT_ENTRY_FOLD_IQ_Q15, iq, out, batch, log2a, 0, stream);
}

int sa_filter_q15(sa_handle *h, const int16_t *in, int16_t *out_time, int batch, void *stream)
{
    return process_q15(h, "sa_filter_q15", in, SaInKind::I16, out_time, batch, SA_Q15_OUT_IQ, stream, false);
}

int sa_process_q15(sa_handle *h, const int16_t *in, int16_t *out_iq, int batch, void *stream)
{
    return process_q15(h, "sa_process_q15", in, SaInKind::I16, out_iq, batch, SA_Q15_OUT_IQ, stream, true);
}

int sa_process_q15_out(sa_handle *h, const int16_t *in, void *out, int batch, int out_kind, void *stream)
{
    return process_q15(h, "sa_process_q15_out", in, SaInKind::I16, out, batch, out_kind, stream, true, true);
}

int sa_process_q15_p12(sa_handle *h, const uint8_t *in, void *out, int batch, int out_kind, void *stream)
{
    return process_q15(h, "sa_process_q15_p12", in, SaInKind::P12, out, batch, out_kind, stream, true, true);
}

int sa_filter_q15_p12(sa_handle *h, const uint8_t *in, int16_t *out_time, int batch, void *stream)
{
    return process_q15(h, "sa_filter_q15_p12", in, SaInKind::P12, out_time, batch, SA_Q15_OUT_IQ, stream, false);
}

// sa_process_f32 (float frames), sa_process_f32_i16 (int16 samples times `scale`) and sa_process_f32_p12 (the same
// samples packed to 12 bits); `fn` names the entry point.
// The float32 path: one launch of the fused chain.  The section coefficients and predictor taps travel by value in the
// kernel arguments (stream-ordered by construction); the per-lane matrices and the window live in device memory
// (stream-ordered uploads).
// The float64-state path (SA_PRECISION_F64_STATE with a cascade: DEFAULT, or CUSTOM with at least one section):
// iir_f64.hip (window + cascade in double, y rounded once) into the slot's workspace, then the bypassed float chain on
// y with the constant 1/2 window (exact).  SA_OUT_TIME is the first launch alone, into `out`.  Timed as one call: the
// start event rides on the first kernel, the stop event on the last.
static int process_float(sa_handle *h, const char *fn, const void *in, SaInKind kind, float scale, void *out, int batch,
                         int out_kind, void *stream)
{
    const bool scale_finite = scale == scale && scale - scale == 0.f;
    { const int rc = check_process_args(h, fn, in, kind, out, batch, out_kind, SaChain::Float, SA_OUT_MARKER, "SA_OUT_MARKER", false,
                                        scale_finite);
      if (rc != SA_OK || batch == 0) return rc; }
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
        const SaLaunchEv ev = {c.start, c.stop};
        SA_HIP(h, kind == SaInKind::I16   ? sa_launch_chain_f32_i16((const int16_t *)in, scale, out, batch, out_kind, t, c.stream, ev)
                  : kind == SaInKind::P12 ? sa_launch_chain_f32_p12((const uint8_t *)in, scale, out, batch, out_kind, t, c.stream, ev)
                                          : sa_launch_chain_f32((const float *)in, out, batch, out_kind, t, c.stream, ev));
        return end_call(h, c);
    }
    float *y = two ? (float *)h->slot[c.slot].work[sa_handle::kWorkF64].ptr : (float *)out;
    SA_HIP(h, sa_launch_iir_f64(in, kind, scale, y, batch, pl.k.nsec, pl.d_p64, h->d_win64, c.stream,
                                {c.start, two ? nullptr : c.stop}));
    if (two) {
        t = {h->d_win_half, h->d_win_t, h->d_twT, h->d_twB, h->d_twC, h->plan_custom.d_lt, nullptr, h->marker_lo, h->marker_hi};
        SA_HIP(h, sa_launch_chain_f32(y, out, batch, out_kind, t, c.stream, {nullptr, c.stop}));
    }
    return end_call(h, c);
}

int sa_process_f32(sa_handle *h, const float *in, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, "sa_process_f32", in, SaInKind::F32, 1.f, out, batch, out_kind, stream);
}

int sa_process_f32_i16(sa_handle *h, const int16_t *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, "sa_process_f32_i16", in, SaInKind::I16, scale, out, batch, out_kind, stream);
}

int sa_process_f32_p12(sa_handle *h, const uint8_t *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, "sa_process_f32_p12", in, SaInKind::P12, scale, out, batch, out_kind, stream);
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
    const auto tables = device_tables(h);
    for (int i = kTablesAtCreate; i < kTables; ++i)
        if (!*tables[i].ptr) SA_HIP(h, hipMalloc(tables[i].ptr, tables[i].bytes));
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
    return export_plan_f64(pl.sos, pl.nsec, out, cap);
}

int sa_iir_plan_from_sos_f64(const double *sos, int n_sections, double *out, int cap)
{
    if (!sos || n_sections < 0 || n_sections > SA_MAXSEC || cap < 0) return SA_EINVAL;
    double norm[36];
    if (!normalise_a0(sos, n_sections, norm)) return SA_EINVAL;
    return export_plan_f64(norm, n_sections, out, cap);
}

}  // extern "C"
