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

// The argument check of every data-plane call is made before anything else and before any call state exists.  The rules,
// their order and their words are sa_pointers.cpp's (sa_check_call, sa_refusal_text), for the entry points of
// include/specan.h and of include/specan_ext.h alike; callers of the ABI see that order.  A NULL handle is SA_EINVAL without
// a message, before the check; an empty batch that passes is SA_OK, and the caller returns it at once.  refused(): a
// refusal of the check leaves "<entry point>: <words>" in sa_last_error.
static int refused(sa_handle *h, int entry, const SaChecked &r)
{
    static_assert((int)SaInKind::F32 == kSaInF32 && (int)SaInKind::I16 == kSaInI16 && (int)SaInKind::P12 == kSaInP12,
                  "sa_pointers.hpp numbers the input forms as SaInKind does");
    static_assert(SA_OUT_MAG_FULL == 0 && SA_Q15_OUT_IQ == 0, "the kinds of both chains are 0 .. marker");
    static_assert(kSaTraceRawBytes == kSaTraceRawRecord, "sa_pointers.hpp sizes the partial records as the kernels do");
    char msg[112];
    sa_refusal_text(entry, r, msg, sizeof msg);
    return fail_at(h, r.code, sa_entry(entry).name, msg);
}

// The launches of a Q15 call of entry point `e` whose arguments have passed their check (batch > 0), as `r` decoded them:
// sa_filter_q15* (window + integer cascade into `out`, r.kind unused), sa_process_q15* (`out` per r.kind, SA_Q15_OUT_* or
// SA_Q15_TRACE_KIND(k): the FFT launch's epilogue makes it; SA_Q15_TRACE_AVG_KIND(k, a), r.fold Trace: the epilogue's partial
// records and a fold launch behind it -- trace_fold_q15.hip), sa_spectra_q15* (r.fold Spectra: r.kind SA_Q15_OUT_IQ into a
// workspace and its bin-by-bin fold behind it -- spectra_fold_q15.hip, include/specan_ext.h) and sa_fold_iq_q15 (that fold
// with nothing in front of it: `in` holds the IQ frames), on int16 samples or on packed 12-bit samples.  With a fold behind
// an FFT, the FFT launch writes into a workspace of the slot and the fold writes `out`.  With a hop, `in` is one stream and
// whichever launch reads the samples -- the cascade, or the FFT in mode 0xB1 -- is handed the hop.  Everything else is the
// frame call.
static int launch_q15(sa_handle *h, const SaEntry &e, const void *in, void *out, int batch, void *stream,
                      const SaChecked &r)
{
    const SaInKind kind = e.in_form == kSaInP12 ? SaInKind::P12 : SaInKind::I16;
    const bool bare = e.in_form == kSaInIQ;                         // the fold alone: nothing in front of it, no workspace
    const bool fft = e.chain == SaChain::Q15 && !bare;
    const int out_kind = r.kind, hop = r.hop;
    SA_HIP(h, hipSetDevice(h->device));
    const SaQ15Params p = q15_params(h);
    const bool staged = fft && p.filter != SA_FILTER_NONE;      // cascade into the slot's workspace, then the FFT
    // SA_Q15_TRACE_AVG_KIND(k, a): the FFT launch writes partial records [B, 16384 >> k] into a workspace of its own and one
    // more launch folds them into `out`.  B (16384 >> k) records of kSaTraceRawBytes are ceil(16 B / W) "frames" of the
    // workspace's one-byte elements (an int: sa_check_call refuses a batch past it).  sa_spectra_q15: the FFT launch writes B
    // IQ frames into a workspace of 4-byte elements.  Grown here, on demand, with the cascade's workspace and before the first
    // launch; never by sa_reserve, which does not know W and sizes nothing for a call the handle may never make.
    const bool folded = fft && r.fold != SaFold::None;
    const int work2 = !folded ? -1 : r.fold == SaFold::Trace ? sa_handle::kWorkTraceRaw : sa_handle::kWorkSpectra;
    const long long frames2 = !folded                  ? 0
                              : r.fold == SaFold::Trace ? ((long long)batch * kSaTraceRawBytes + (1 << r.log2w) - 1) >> r.log2w
                                                        : batch;
    CallCtx c;
    { const int rc = begin_call(h, (hipStream_t)stream, staged ? sa_handle::kWorkQ15 : -1, batch, &c, work2, (int)frames2);
      if (rc != SA_OK) return rc; }
    const SaQ15Tables t = {h->d_rom, h->d_twq, h->d_twrec, h->marker_lo, h->marker_hi};
    // what the FFT launch writes, and the event its completion is bound to: the fold launch, where there is one, is the call's last
    void *fft_out = folded ? h->slot[c.slot].work[work2].ptr : out;
    hipEvent_t fft_stop = folded ? nullptr : c.stop;
    const auto launch_fold = [&](const void *from, hipEvent_t start) {
        return r.fold == SaFold::Trace ? sa_launch_trace_fold_q15(from, out, batch, r.log2w, r.log2a, c.stream, {start, c.stop})
                                       : sa_launch_spectra_fold_q15(from, out, batch, r.log2a, c.stream, {start, c.stop});
    };
    if (bare) {
        SA_HIP(h, launch_fold(in, c.start));
        return end_call(h, c);
    }
    if (!staged) {
        SA_HIP(h, fft ? sa_launch_fft_q15(in, kind, hop, fft_out, batch, out_kind, true, p, t, c.stream, {c.start, fft_stop})
                      : sa_launch_filter_q15(in, kind, hop, (int16_t *)out, batch, p, t, c.stream, {c.start, c.stop}));
        if (folded) SA_HIP(h, launch_fold(fft_out, nullptr));
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
    SA_HIP(h, sa_launch_filter_q15(in, kind, hop, ws, batch, p, t, c.stream, {c.start, nullptr}));
    SA_HIP(h, sa_launch_fft_q15(ws, SaInKind::I16, 0, fft_out, batch, out_kind, false, p, t, c.stream, {nullptr, fft_stop}));
    if (folded) SA_HIP(h, launch_fold(fft_out, nullptr));
    return end_call(h, c);
}

// Every Q15 call, of include/specan.h (`kind_word`: its out_kind where it has one) and of include/specan_ext.h (`log2a`,
// `hop`): the argument check, then launch_q15 on what the check decoded.  One instance per entry point, so that each of
// them is the check and, for a call that launches, a jump to the shared launch_q15.
extern "C++" template <int kEntry>
static int call_q15(sa_handle *h, const void *in, void *out, int batch, int kind_word, int log2a, int hop, void *stream)
{
    SaChecked r;
    const SaCall call = {kEntry, kind_word, log2a, hop, batch, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, true};
    if (!h) return SA_EINVAL;
    if (sa_check_call(call, &r) != SA_OK) return refused(h, call.entry, r);
    if (batch == 0) return SA_OK;
    return launch_q15(h, sa_entry(kEntry), in, out, batch, stream, r);
}

int sa_ext_version(void) { return SA_EXT_VERSION; }

int sa_spectra_q15(sa_handle *h, const int16_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream)
{
    return call_q15<kSaEntryExt + SA_EXT_ENTRY_SPECTRA_Q15>(h, in, out, batch, 0, log2a, hop, stream);
}

int sa_spectra_q15_p12(sa_handle *h, const uint8_t *in, sa_trace_point_q15 *out, int batch, int log2a, int hop, void *stream)
{
    return call_q15<kSaEntryExt + SA_EXT_ENTRY_SPECTRA_Q15_P12>(h, in, out, batch, 0, log2a, hop, stream);
}

int sa_fold_iq_q15(sa_handle *h, const int16_t *iq, sa_trace_point_q15 *out, int batch, int log2a, void *stream)
{
    return call_q15<kSaEntryExt + SA_EXT_ENTRY_FOLD_IQ_Q15>(h, iq, out, batch, 0, log2a, 0, stream);
}

int sa_filter_q15(sa_handle *h, const int16_t *in, int16_t *out_time, int batch, void *stream)
{
    return call_q15<SA_ENTRY_FILTER_Q15>(h, in, out_time, batch, 0, 0, 0, stream);
}

int sa_process_q15(sa_handle *h, const int16_t *in, int16_t *out_iq, int batch, void *stream)
{
    return call_q15<SA_ENTRY_PROCESS_Q15>(h, in, out_iq, batch, 0, 0, 0, stream);
}

int sa_process_q15_out(sa_handle *h, const int16_t *in, void *out, int batch, int out_kind, void *stream)
{
    return call_q15<SA_ENTRY_PROCESS_Q15_OUT>(h, in, out, batch, out_kind, 0, 0, stream);
}

int sa_process_q15_p12(sa_handle *h, const uint8_t *in, void *out, int batch, int out_kind, void *stream)
{
    return call_q15<SA_ENTRY_PROCESS_Q15_P12>(h, in, out, batch, out_kind, 0, 0, stream);
}

int sa_filter_q15_p12(sa_handle *h, const uint8_t *in, int16_t *out_time, int batch, void *stream)
{
    return call_q15<SA_ENTRY_FILTER_Q15_P12>(h, in, out_time, batch, 0, 0, 0, stream);
}

// sa_process_f32 (float frames), sa_process_f32_i16 (int16 samples times `scale`) and sa_process_f32_p12 (the same
// samples packed to 12 bits), by `entry`.
// The float32 path: one launch of the fused chain.  The section coefficients and predictor taps travel by value in the
// kernel arguments (stream-ordered by construction); the per-lane matrices and the window live in device memory
// (stream-ordered uploads).
// The float64-state path (SA_PRECISION_F64_STATE with a cascade: DEFAULT, or CUSTOM with at least one section):
// iir_f64.hip (window + cascade in double, y rounded once) into the slot's workspace, then the bypassed float chain on
// y with the constant 1/2 window (exact).  SA_OUT_TIME is the first launch alone, into `out`.  Timed as one call: the
// start event rides on the first kernel, the stop event on the last.
static int process_float(sa_handle *h, int entry, const void *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    const bool scale_finite = scale == scale && scale - scale == 0.f;
    SaChecked r;
    const SaCall call = {entry, out_kind, 0, 0, batch, (uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, scale_finite};
    if (!h) return SA_EINVAL;
    if (sa_check_call(call, &r) != SA_OK) return refused(h, call.entry, r);
    if (batch == 0) return SA_OK;
    const char *fn = sa_entry(entry).name;
    const SaInKind kind = (SaInKind)sa_entry(entry).in_form;
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
    return process_float(h, SA_ENTRY_PROCESS_F32, in, 1.f, out, batch, out_kind, stream);
}

int sa_process_f32_i16(sa_handle *h, const int16_t *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, SA_ENTRY_PROCESS_F32_I16, in, scale, out, batch, out_kind, stream);
}

int sa_process_f32_p12(sa_handle *h, const uint8_t *in, float scale, void *out, int batch, int out_kind, void *stream)
{
    return process_float(h, SA_ENTRY_PROCESS_F32_P12, in, scale, out, batch, out_kind, stream);
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
