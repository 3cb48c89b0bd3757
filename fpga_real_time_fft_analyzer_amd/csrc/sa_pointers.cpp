// sa_pointers.cpp -- the pointer contract of the process and filter calls as pure host arithmetic (sa_pointers.hpp), and
// its handle-free debug export.  Every byte count is 64 bits wide (40 000 float frames are 2.6 GB) and addresses are
// compared as integers, never dereferenced.
#include "sa_pointers.hpp"

#include "../../include/specan_ext.h"

namespace {

constexpr uint64_t kN = SA_N;

// bytes of one frame of input, by input form
bool in_frame_bytes(int in_form, uint64_t *bytes)
{
    switch (in_form) {
        case kSaInF32: *bytes = kN * 4; return true;                    // SA_FRAME_BYTES
        case kSaInI16: *bytes = kN * 2; return true;
        case kSaInP12: *bytes = SA_P12_FRAME_BYTES; return true;
        default: return false;
    }
}

// bytes of one row of output (one frame's, or one group's of sa_frames_per_row frames) and the alignment of `out`, by chain and kind: the table of kinds of include/specan.h
bool out_frame_bytes(SaChain chain, int out_kind, uint64_t *bytes, unsigned *align)
{
    *align = 16;
    if (chain == SaChain::Q15Filter) { *bytes = kN * 2; return true; }                // int16 [B,16384]
    if (chain == SaChain::Float) {
        switch (out_kind) {
            case SA_OUT_MAG_FULL:
            case SA_OUT_TIME: *bytes = kN * 4; return true;                           // float [B,16384]
            case SA_OUT_MAG_HALF: *bytes = (kN / 2 + 1) * 4; *align = 4; return true;  // float [B,8193]: rows 32 772 bytes apart
            case SA_OUT_SPEC_HALF: *bytes = (kN / 2 + 1) * 8; *align = 8; return true; // float2 [B,8193]: rows 65 544 bytes apart
            case SA_OUT_MARKER: *bytes = sizeof(sa_marker); return true;
            default: return false;
        }
    }
    if (out_kind >= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MIN) && out_kind <= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MAX)) {
        *bytes = (kN >> (out_kind & 0xF)) * sizeof(sa_trace_point_q15);
        return true;
    }
    if (SA_Q15_IS_TRACE_AVG_KIND(out_kind)) {                                         // one row per A frames (sa_frames_per_row)
        *bytes = (kN >> SA_Q15_TRACE_AVG_LOG2W(out_kind)) * sizeof(sa_trace_point_q15);
        return true;
    }
    switch (out_kind) {
        case SA_Q15_OUT_IQ:
        case SA_Q15_OUT_MAG: *bytes = kN * 4; return true;                            // int16 [B,16384,2], float [B,16384]
        case SA_Q15_OUT_MARKER: *bytes = sizeof(sa_marker_q15); return true;
        default: return false;
    }
}

}  // namespace

int sa_frames_per_row(SaChain chain, int out_kind)
{
    return chain == SaChain::Q15 && SA_Q15_IS_TRACE_AVG_KIND(out_kind) ? 1 << SA_Q15_TRACE_AVG_LOG2A(out_kind) : 1;
}

bool sa_call_span(SaChain chain, int in_form, int out_kind, int hop, int batch, SaCallSpan *s)
{
    uint64_t in_frame = 0, out_frame = 0;
    if (batch <= 0 || !in_frame_bytes(in_form, &in_frame) || !out_frame_bytes(chain, out_kind, &out_frame, &s->out_align))
        return false;
    if (in_form == kSaInF32 && chain != SaChain::Float) return false;
    if (hop != 0 && (chain != SaChain::Q15 || hop < 8 || hop > SA_N || hop % 8 != 0)) return false;
    const uint64_t B = (uint64_t)batch;
    s->in_align = 16;
    s->out_bytes = B / (uint64_t)sa_frames_per_row(chain, out_kind) * out_frame;
    if (hop == 0) {
        s->in_bytes = B * in_frame;
    } else {                                   // one stream: the last frame ends with it
        const uint64_t samples = (B - 1) * (uint64_t)hop + kN;
        s->in_bytes = in_form == kSaInP12 ? samples / 2 * 3 : samples * 2;      // hop is even: so is `samples`
    }
    return true;
}

unsigned sa_pointer_faults(const SaCallSpan &s, uint64_t in, uint64_t out)
{
    unsigned faults = 0;
    if (in & (uint64_t)(s.in_align - 1)) faults |= kSaPtrInAlign;
    if (out & (uint64_t)(s.out_align - 1)) faults |= kSaPtrOutAlign;
    // [in, in + in_bytes) and [out, out + out_bytes) meet iff the higher base lies less than the lower range's length
    // above the lower base: a difference, so that no sum of an address and a length can wrap
    if (in <= out ? out - in < s.in_bytes : in - out < s.out_bytes) faults |= kSaPtrOverlap;
    return faults;
}

namespace {

struct EntryInfo {
    SaChain chain;
    int in_form;
    bool has_kind, hop_word;
};

// index = SA_ENTRY_* of include/specan.h
constexpr EntryInfo kEntries[] = {
    {SaChain::Float, kSaInF32, true, false},        // sa_process_f32
    {SaChain::Float, kSaInI16, true, false},        // sa_process_f32_i16
    {SaChain::Float, kSaInP12, true, false},        // sa_process_f32_p12
    {SaChain::Q15, kSaInI16, false, false},         // sa_process_q15
    {SaChain::Q15, kSaInI16, true, true},           // sa_process_q15_out
    {SaChain::Q15, kSaInP12, true, true},           // sa_process_q15_p12
    {SaChain::Q15Filter, kSaInI16, false, false},   // sa_filter_q15
    {SaChain::Q15Filter, kSaInP12, false, false},   // sa_filter_q15_p12
};
static_assert(sizeof kEntries / sizeof kEntries[0] == SA_ENTRY_COUNT, "one row per SA_ENTRY_*");
static_assert(SA_ENTRY_PROCESS_F32 == 0 && SA_ENTRY_PROCESS_Q15 == 3 && SA_ENTRY_FILTER_Q15_P12 == 7, "the rows above");

}  // namespace

extern "C" int sa_debug_check_pointers(int entry, int kind_word, uint64_t in_addr, uint64_t out_addr, int batch)
{
    if (entry < 0 || entry >= SA_ENTRY_COUNT) return SA_EINVAL;
    const EntryInfo &e = kEntries[entry];
    if (batch < 0) return SA_ESHAPE;
    int kind = e.has_kind ? kind_word : SA_Q15_OUT_IQ, hop = 0;
    if (e.has_kind && e.hop_word && kind_word >= 0) {
        const int field = (kind_word >> 8) & 0xFFF;
        if ((kind_word >> 20) != 0 || field > SA_Q15_HOP_FIELD_MAX) return SA_EINVAL;
        kind = kind_word & 0xFF;
        hop = 8 * field;
    }
    SaCallSpan s;
    if (!sa_call_span(e.chain, e.in_form, kind, hop, batch == 0 ? 1 : batch, &s)) return SA_EINVAL;    // a kind is checked
    if (batch == 0) return SA_OK;                                                                    // before the pointers
    if (batch % sa_frames_per_row(e.chain, kind)) return SA_ESHAPE;                                  // and so is the group
    if (in_addr == 0 || out_addr == 0) return SA_EINVAL;
    return sa_pointer_faults(s, in_addr, out_addr) ? SA_EINVAL : SA_OK;
}

// ---- include/specan_ext.h ---------------------------------------------------------------------------------------------

int sa_ext_check(int entry, int log2a, int hop, uint64_t in, uint64_t out, int batch, SaExtWhy *why, SaCallSpan *span)
{
    static_assert(SA_EXT_ENTRY_SPECTRA_Q15 == 0 && SA_EXT_ENTRY_SPECTRA_Q15_P12 == 1 && SA_EXT_ENTRY_FOLD_IQ_Q15 == 2 &&
                      SA_EXT_ENTRY_COUNT == 3, "the entries told apart below");
    *why = kSaExtEntry;
    if (entry < 0 || entry >= SA_EXT_ENTRY_COUNT) return SA_EINVAL;
    const bool fold = entry == SA_EXT_ENTRY_FOLD_IQ_Q15;
    *why = kSaExtBatch;
    if (batch < 0) return SA_ESHAPE;
    *why = kSaExtLog2a;
    if (log2a < SA_Q15_TRACE_LOG2A_MIN || log2a > SA_Q15_TRACE_LOG2A_MAX) return SA_EINVAL;
    *why = kSaExtHop;
    if (hop != 0 && (fold || hop < 8 || hop > SA_N || hop % 8 != 0)) return SA_EINVAL;
    *why = kSaExtNone;
    if (batch == 0) return SA_OK;
    *why = kSaExtGroup;
    if (batch & ((1 << log2a) - 1)) return SA_ESHAPE;
    *why = kSaExtNull;
    const uint64_t B = (uint64_t)batch;
    if (fold) {
        span->in_bytes = B * kN * 4;                                // int16 [B,16384,2]
        span->in_align = 16;
    } else if (!sa_call_span(SaChain::Q15, entry == SA_EXT_ENTRY_SPECTRA_Q15_P12 ? kSaInP12 : kSaInI16, SA_Q15_OUT_IQ, hop, batch,
                             span)) {
        *why = kSaExtHop;                                           // unreachable: the hop was checked above
        return SA_EINVAL;
    }
    span->out_bytes = (B >> log2a) * kN * sizeof(sa_trace_point_q15);
    span->out_align = 16;
    if (in == 0 || out == 0) return SA_EINVAL;
    const unsigned faults = sa_pointer_faults(*span, in, out);
    *why = faults & kSaPtrInAlign ? kSaExtInAlign : faults & kSaPtrOutAlign ? kSaExtOutAlign : faults ? kSaExtOverlap : kSaExtNone;
    return faults ? SA_EINVAL : SA_OK;
}

extern "C" int sa_ext_check_pointers(int entry, int log2a, int hop, uint64_t in_addr, uint64_t out_addr, int batch)
{
    SaExtWhy why;
    SaCallSpan s;
    return sa_ext_check(entry, log2a, hop, in_addr, out_addr, batch, &why, &s);
}
