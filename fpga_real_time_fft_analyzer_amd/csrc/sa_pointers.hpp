// sa_pointers.hpp -- the argument check of every data-plane call: the eight process and filter calls of include/specan.h
// and the three calls of include/specan_ext.h.  sa_check_call() (here, with sa_check_addresses in sa_pointers.cpp as its
// second half) is the one place that takes a kind word apart, orders the
// refusals (both headers list them) and sizes the call: how many bytes it reads through `in` and writes through `out`, the
// alignment each must have, and the test that the two byte ranges are disjoint.  Pure integer arithmetic on addresses that
// are never dereferenced: no handle, no stream and no HIP runtime call.  The entry points (specan_abi.cpp) run it before any
// call state exists and launch what it decoded; sa_debug_check_pointers and sa_ext_check_pointers return its code, so
// tests/test_pointer_contract_cpu.py, tests/test_q15_spectra_cpu.py and the stand-alone programs under tests/cpp run, without
// a GPU, the code the entry points run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/specan_ext.h"

#pragma GCC visibility push(hidden)

// which family of outputs the entry point has: the float chain (SA_OUT_*), the integer chain with its FFT (SA_Q15_OUT_*,
// SA_Q15_TRACE_KIND, SA_Q15_TRACE_AVG_KIND) or the integer chain without it (sa_filter_q15*: one output, no kind)
enum class SaChain { Float, Q15, Q15Filter };

// what `in` points to; the first three are the values of SaInKind (sa_common.hpp), which this unit does not include: it
// pulls in the HIP runtime.  kSaInIQ: the int16 [B,16384,2] frames sa_fold_iq_q15 folds, with nothing in front of the fold.
enum { kSaInF32 = 0, kSaInI16 = 1, kSaInP12 = 2, kSaInIQ = 3 };

// The entry points, numbered for this unit: SA_ENTRY_* of include/specan.h as they are, SA_EXT_ENTRY_* of
// include/specan_ext.h behind them.
constexpr int kSaEntryExt = 8, kSaEntryCount = 11;

// bytes of one partial record of SA_Q15_TRACE_AVG_KIND in its workspace: kSaTraceRawBytes of sa_common.hpp (as kSaIn* above)
constexpr int kSaTraceRawRecord = 16;

// what follows `batch` in the argument list: nothing, a kind, a kind word that may carry a hop (SA_Q15_HOP_KIND) and name
// the grouped kinds (SA_Q15_TRACE_AVG_KIND), or log2a and hop as plain ints (include/specan_ext.h)
enum class SaArgs { NoKind, Kind, HopWord, Ext };

struct SaEntry {
    const char *name;
    SaChain chain;
    int in_form;
    SaArgs args;
    bool ext_hop;               // SaArgs::Ext: the call takes a hop (the fold takes frames alone)
    int marker;                 // the kind whose `out` holds marker records, with its name; -1 where there is none
    const char *marker_name;
};

// A data-plane call as the caller wrote it.  `kind_word` is read for SaArgs::Kind and HopWord, `log2a` and `hop` for
// SaArgs::Ext; `scale_finite` is true for the entry points that have no scale.
struct SaCall {
    int entry, kind_word, log2a, hop, batch;
    uint64_t in, out;
    bool scale_finite;
};

struct SaCallSpan {
    uint64_t in_bytes, out_bytes;      // the call reads [in, in + in_bytes) and writes [out, out + out_bytes)
    unsigned in_align, out_align;      // powers of two
};

// which rule refused, in the order the rules are asked (SaArgs::Ext has log2a and hop where the others have the hop word,
// the kind and the scale); kSaNone with SA_OK.  A marker, trace or grouped-trace `out` that is misaligned is named before a
// misaligned `in`, as it always was; every other kind names `in` first.
enum SaRule { kSaNone, kSaEntryRule, kSaBatch, kSaHopWord, kSaLog2a, kSaHop, kSaKind, kSaScale, kSaGroup, kSaNull, kSaInAlign,
              kSaOutAlign, kSaOverlap, kSaWorkspace };

// what a Q15 call launches behind its FFT: nothing, the fold of SA_Q15_TRACE_AVG_KIND(k, a)'s partial records, or the
// bin-by-bin fold of include/specan_ext.h
enum class SaFold { None, Trace, Spectra };

struct SaChecked {
    int code;                   // SA_OK, SA_EINVAL or SA_ESHAPE
    SaRule rule;
    // what the call says, as far as the rules before `rule` have read it; all of it with SA_OK
    int kind;                   // the low byte of the kind word; SA_Q15_OUT_IQ for an entry point without one
    int hop;                    // in samples, 0: frames
    SaFold fold;
    int log2w, log2a;           // of the fold
    SaCallSpan span;            // from kSaInAlign on, and with SA_OK at batch > 0
};

constexpr uint64_t kSaN = SA_N;

// one row per entry point: index = SA_ENTRY_* of include/specan.h, then kSaEntryExt + SA_EXT_ENTRY_* of include/specan_ext.h
inline constexpr SaEntry kSaEntries[] = {
    {"sa_process_f32", SaChain::Float, kSaInF32, SaArgs::Kind, false, SA_OUT_MARKER, "SA_OUT_MARKER"},
    {"sa_process_f32_i16", SaChain::Float, kSaInI16, SaArgs::Kind, false, SA_OUT_MARKER, "SA_OUT_MARKER"},
    {"sa_process_f32_p12", SaChain::Float, kSaInP12, SaArgs::Kind, false, SA_OUT_MARKER, "SA_OUT_MARKER"},
    {"sa_process_q15", SaChain::Q15, kSaInI16, SaArgs::NoKind, false, -1, nullptr},
    {"sa_process_q15_out", SaChain::Q15, kSaInI16, SaArgs::HopWord, false, SA_Q15_OUT_MARKER, "SA_Q15_OUT_MARKER"},
    {"sa_process_q15_p12", SaChain::Q15, kSaInP12, SaArgs::HopWord, false, SA_Q15_OUT_MARKER, "SA_Q15_OUT_MARKER"},
    {"sa_filter_q15", SaChain::Q15Filter, kSaInI16, SaArgs::NoKind, false, -1, nullptr},
    {"sa_filter_q15_p12", SaChain::Q15Filter, kSaInP12, SaArgs::NoKind, false, -1, nullptr},
    {"sa_spectra_q15", SaChain::Q15, kSaInI16, SaArgs::Ext, true, -1, nullptr},
    {"sa_spectra_q15_p12", SaChain::Q15, kSaInP12, SaArgs::Ext, true, -1, nullptr},
    {"sa_fold_iq_q15", SaChain::Q15, kSaInIQ, SaArgs::Ext, false, -1, nullptr},
};
static_assert(sizeof kSaEntries / sizeof kSaEntries[0] == kSaEntryCount && kSaEntryExt == SA_ENTRY_COUNT &&
                  kSaEntryCount == SA_ENTRY_COUNT + SA_EXT_ENTRY_COUNT, "one row per SA_ENTRY_* and SA_EXT_ENTRY_*");
static_assert(SA_ENTRY_PROCESS_F32 == 0 && SA_ENTRY_PROCESS_Q15 == 3 && SA_ENTRY_FILTER_Q15_P12 == 7 &&
                  SA_EXT_ENTRY_SPECTRA_Q15 == 0 && SA_EXT_ENTRY_SPECTRA_Q15_P12 == 1 && SA_EXT_ENTRY_FOLD_IQ_Q15 == 2,
              "the rows above");

inline const SaEntry &sa_entry(int entry) { return kSaEntries[entry]; }       // entry = 0 .. kSaEntryCount - 1

inline bool sa_is_trace(const SaEntry &e, int kind)
{
    return e.chain == SaChain::Q15 && kind >= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MIN) &&
           kind <= SA_Q15_TRACE_KIND(SA_Q15_TRACE_LOG2W_MAX);
}

inline bool sa_is_trace_avg(const SaEntry &e, int kind)
{
    return e.chain == SaChain::Q15 && kind >= 0 && SA_Q15_IS_TRACE_AVG_KIND(kind);
}

// bytes of one row of output (one frame's, or one group's of frames) and the alignment of `out`, by entry point and kind:
// the tables of kinds of include/specan.h.  False for a kind the chain does not have.
inline bool sa_out_row_bytes(const SaEntry &e, int kind, uint64_t *bytes, unsigned *align)
{
    *align = 16;
    if (e.args == SaArgs::Ext) { *bytes = kSaN * sizeof(sa_trace_point_q15); return true; }  // one record per bin and group
    if (e.chain == SaChain::Q15Filter) { *bytes = kSaN * 2; return true; }                   // int16 [B,16384]
    if (e.chain == SaChain::Float) {
        switch (kind) {
            case SA_OUT_MAG_FULL:
            case SA_OUT_TIME: *bytes = kSaN * 4; return true;                           // float [B,16384]
            case SA_OUT_MAG_HALF: *bytes = (kSaN / 2 + 1) * 4; *align = 4; return true;   // float [B,8193]: 32 772-byte rows
            case SA_OUT_SPEC_HALF: *bytes = (kSaN / 2 + 1) * 8; *align = 8; return true;  // float2 [B,8193]: 65 544-byte rows
            case SA_OUT_MARKER: *bytes = sizeof(sa_marker); return true;
            default: return false;
        }
    }
    if (sa_is_trace(e, kind)) { *bytes = (kSaN >> (kind & 0xF)) * sizeof(sa_trace_point_q15); return true; }
    if (sa_is_trace_avg(e, kind)) {
        *bytes = (kSaN >> SA_Q15_TRACE_AVG_LOG2W(kind)) * sizeof(sa_trace_point_q15);
        return true;
    }
    switch (kind) {
        case SA_Q15_OUT_IQ:
        case SA_Q15_OUT_MAG: *bytes = kSaN * 4; return true;                            // int16 [B,16384,2], float [B,16384]
        case SA_Q15_OUT_MARKER: *bytes = sizeof(sa_marker_q15); return true;
        default: return false;
    }
}

inline int sa_refuse(SaChecked &r, int code, SaRule rule)
{
    r.rule = rule;
    return r.code = code;
}

// The second half of the check (sa_pointers.cpp), for a batch > 0 that is a multiple of its group
int sa_check_addresses(const SaCall &c, const SaEntry &e, uint64_t out_row, SaChecked &r);

// The check: fills *r and returns r->code.  Its first half, up to the empty batch and the group, is inline and forced so: an
// entry point passes a constant entry, its row of the table folds, and what is left in it are the few compares of its own
// rules (left to itself the compiler keeps one generic copy out of line, measurably slower per call than the code this
// replaced: profiles/r15_call_check.txt).  The exports instantiate it for an entry known at run time.
__attribute__((always_inline)) inline int sa_check_call(const SaCall &c, SaChecked *out)
{
    SaChecked &r = *out;
    r = {SA_OK, kSaNone, SA_Q15_OUT_IQ, 0, SaFold::None, 0, 0, {0, 0, 16, 16}};
    if (c.entry < 0 || c.entry >= kSaEntryCount) return sa_refuse(r, SA_EINVAL, kSaEntryRule);
    const SaEntry &e = kSaEntries[c.entry];
    if (c.batch < 0) return sa_refuse(r, SA_ESHAPE, kSaBatch);
    if (e.args == SaArgs::Ext) {
        if (c.log2a < SA_Q15_TRACE_LOG2A_MIN || c.log2a > SA_Q15_TRACE_LOG2A_MAX) return sa_refuse(r, SA_EINVAL, kSaLog2a);
        if (c.hop != 0 && (!e.ext_hop || c.hop < 8 || c.hop > SA_N || c.hop % 8 != 0))
            return sa_refuse(r, SA_EINVAL, kSaHop);
        r.hop = c.hop;
        r.fold = SaFold::Spectra;
        r.log2a = c.log2a;
    } else if (e.args != SaArgs::NoKind) {
        r.kind = c.kind_word;
        if (e.args == SaArgs::HopWord && c.kind_word >= 0) {       // a negative word is the bad kind it always was
            const int field = (c.kind_word >> 8) & 0xFFF;
            if ((c.kind_word >> 20) != 0 || field > SA_Q15_HOP_FIELD_MAX) return sa_refuse(r, SA_EINVAL, kSaHopWord);
            r.kind = c.kind_word & 0xFF;
            r.hop = 8 * field;
        }
    }
    uint64_t out_row = 0;
    if (!sa_out_row_bytes(e, r.kind, &out_row, &r.span.out_align)) return sa_refuse(r, SA_EINVAL, kSaKind);
    if (!c.scale_finite) return sa_refuse(r, SA_EINVAL, kSaScale);
    if (sa_is_trace_avg(e, r.kind)) {
        r.fold = SaFold::Trace;
        r.log2w = SA_Q15_TRACE_AVG_LOG2W(r.kind);
        r.log2a = SA_Q15_TRACE_AVG_LOG2A(r.kind);
    }
    if (c.batch == 0) return SA_OK;                                   // before the addresses are looked at
    if (c.batch & ((1 << r.log2a) - 1)) return sa_refuse(r, SA_ESHAPE, kSaGroup);    // log2a is 0 without a fold
    return sa_check_addresses(c, e, out_row, r);
}

// The words sa_last_error gives behind "<entry name>: " for a refusal of sa_check_call; "" for kSaNone and kSaEntryRule
void sa_refusal_text(int entry, const SaChecked &r, char *buf, size_t cap);

#pragma GCC visibility pop
