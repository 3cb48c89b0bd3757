// Stand-alone host test of the one argument check behind the eleven data-plane entry points (sa_check_call and
// sa_refusal_text in csrc/sa_pointers.cpp; the rules and their order are stated in include/specan.h and include/specan_ext.h).
// No GPU, no library: compiled together with sa_pointers.cpp by tests/test_pointer_contract_cpu.py, under the address and
// undefined-behaviour sanitizers where they link.  For every entry point, one argument tuple per rule the entry point can
// reach, tripping that rule alone: the code, the rule and the words of sa_last_error, which are written out here as the entry
// points have always given them and never taken from the code under test.  Then tuples that trip two rules, where the
// earlier one must win, and accepted calls with what the check decodes from them.  For every tuple the handle-free exports
// sa_debug_check_pointers and sa_ext_check_pointers must return the code of the check.  Prints "ok <checks>" and returns 0,
// or names the first failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../fpga_real_time_fft_analyzer_amd/csrc/sa_pointers.hpp"
#include "../../include/specan_ext.h"

static int g_checks = 0;

static const uint64_t IN = 1ull << 40, OUT = 1ull << 41;       // 16-byte aligned and 1 TiB apart
static const int B = 4, A4 = 2;                                  // log2a = 2: groups of A = 4 frames
static const int F32 = SA_ENTRY_PROCESS_F32, F32_I16 = SA_ENTRY_PROCESS_F32_I16, F32_P12 = SA_ENTRY_PROCESS_F32_P12,
                 Q15 = SA_ENTRY_PROCESS_Q15, Q15_OUT = SA_ENTRY_PROCESS_Q15_OUT, Q15_P12 = SA_ENTRY_PROCESS_Q15_P12,
                 FILT = SA_ENTRY_FILTER_Q15, FILT_P12 = SA_ENTRY_FILTER_Q15_P12, SPEC = 8 + SA_EXT_ENTRY_SPECTRA_Q15,
                 SPEC_P12 = 8 + SA_EXT_ENTRY_SPECTRA_Q15_P12, FOLD = 8 + SA_EXT_ENTRY_FOLD_IQ_Q15;
static const char *const NAMES[] = {"sa_process_f32", "sa_process_f32_i16", "sa_process_f32_p12", "sa_process_q15",
                                    "sa_process_q15_out", "sa_process_q15_p12", "sa_filter_q15", "sa_filter_q15_p12",
                                    "sa_spectra_q15", "sa_spectra_q15_p12", "sa_fold_iq_q15"};
static const int MARKER = SA_Q15_OUT_MARKER, TRACE = SA_Q15_TRACE_KIND(4), AVG = SA_Q15_TRACE_AVG_KIND(4, 2);
static const int HOP = 4096, HOPW = (HOP / 8) << 8;              // the hop field of a SA_Q15_HOP_KIND word

struct T {
    int entry, word, log2a, hop, batch;
    uint64_t in, out;
    bool finite;
    int code;
    SaRule rule;
    const char *text;
};

// the words of the entry points
#define NEG "negative batch"
#define HOPWORD "bad out_kind: hop field above 2048 or bits 20..30 set"
#define KIND "bad out_kind"
#define SCALE "scale is not finite"
#define GROUP "SA_Q15_TRACE_AVG_KIND: batch must be a multiple of the group size A"
#define XGROUP "batch must be a multiple of the group size A"
#define NUL "NULL tensor"
#define IN16 "`in` must be 16-byte aligned"
#define PACKED "packed input must be 16-byte aligned"
#define STREAM "a sample stream (SA_Q15_HOP_KIND) must be 16-byte aligned"
#define XSTREAM "a sample stream must be 16-byte aligned"
#define OUT16 "`out` must be 16-byte aligned"
#define WORKSPACE "SA_Q15_TRACE_AVG_KIND: batch too large for the workspace"
#define LOG2A "log2a must be 1..7 (groups of A = 2..128 frames)"
#define XHOP "hop must be 0 or a multiple of 8 in 8..16384"
#define FOLDHOP "the fold takes frames: no hop"
#define OVERLAP(r, w) "`in` (" #r " bytes read) and `out` (" #w " bytes written) overlap"

static const T kCases[] = {
    // ---- sa_process_f32: one tuple per rule
    {F32, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {F32, 5, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32, -1, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32, 0x40000, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},                   // a hop word is an unknown kind here
    {F32, TRACE, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32, AVG, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32, 0, 0, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {F32, 0, 0, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {F32, 0, 0, 0, B, IN + 4, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {F32, SA_OUT_MAG_FULL, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {F32, SA_OUT_TIME, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, OUT16},
    {F32, SA_OUT_MAG_HALF, 0, 0, B, IN, OUT + 2, true, SA_EINVAL, kSaOutAlign, "`out` must be 4-byte aligned"},
    {F32, SA_OUT_SPEC_HALF, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, "`out` must be 8-byte aligned"},
    {F32, SA_OUT_MARKER, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_OUT_MARKER output must be 16-byte aligned"},
    {F32, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 262144)},
    {F32, SA_OUT_MAG_HALF, 0, 0, B, IN, IN + 262144 - 4, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 131088)},
    {F32, SA_OUT_SPEC_HALF, 0, 0, B, IN, IN - 262176 + 8, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 262176)},
    {F32, SA_OUT_MARKER, 0, 0, B, IN, IN + 16, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 64)},
    // ---- sa_process_f32_i16
    {F32_I16, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {F32_I16, 5, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32_I16, 0, 0, 0, B, IN, OUT, false, SA_EINVAL, kSaScale, SCALE},
    {F32_I16, 0, 0, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {F32_I16, 0, 0, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {F32_I16, 0, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {F32_I16, SA_OUT_MAG_HALF, 0, 0, B, IN, OUT + 1, true, SA_EINVAL, kSaOutAlign, "`out` must be 4-byte aligned"},
    {F32_I16, SA_OUT_MARKER, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, "SA_OUT_MARKER output must be 16-byte aligned"},
    {F32_I16, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 262144)},
    // ---- sa_process_f32_p12
    {F32_P12, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {F32_P12, 5, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {F32_P12, 0, 0, 0, B, IN, OUT, false, SA_EINVAL, kSaScale, SCALE},
    {F32_P12, 0, 0, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {F32_P12, 0, 0, 0, B, IN + 1, OUT, true, SA_EINVAL, kSaInAlign, PACKED},
    {F32_P12, 0, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {F32_P12, SA_OUT_SPEC_HALF, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, "`out` must be 8-byte aligned"},
    {F32_P12, SA_OUT_MARKER, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_OUT_MARKER output must be 16-byte aligned"},
    {F32_P12, 0, 0, 0, B, IN, IN + 98304 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(98304, 262144)},
    // ---- sa_process_q15: no kind, the word is not read
    {Q15, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {Q15, 0, 0, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {Q15, 99, 0, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15, MARKER, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {Q15, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 262144)},
    // ---- sa_process_q15_out
    {Q15_OUT, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {Q15_OUT, 0 | 2049 << 8, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {Q15_OUT, 1 << 20, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {Q15_OUT, 1 << 30, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {Q15_OUT, 3, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, -1, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, SA_Q15_TRACE_KIND(0), 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, SA_Q15_TRACE_KIND(7), 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, 0x80, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, 0x88, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},                  // log2a = 1, log2w = 0
    {Q15_OUT, 0xC9, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, 3 | HOPW, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, AVG, 0, 0, 5, IN, OUT, true, SA_ESHAPE, kSaGroup, GROUP},
    {Q15_OUT, AVG | HOPW, 0, 0, 5, IN, OUT, true, SA_ESHAPE, kSaGroup, GROUP},
    {Q15_OUT, 0, 0, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {Q15_OUT, AVG, 0, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {Q15_OUT, 0, 0, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15_OUT, MARKER, 0, 0, B, IN + 8, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15_OUT, 0 | HOPW, 0, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, STREAM},
    {Q15_OUT, AVG | HOPW, 0, 0, B, IN + 8, OUT, true, SA_EINVAL, kSaInAlign, STREAM},
    {Q15_OUT, SA_Q15_OUT_IQ, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {Q15_OUT, SA_Q15_OUT_MAG | HOPW, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, OUT16},
    {Q15_OUT, MARKER, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_OUT_MARKER output must be 16-byte aligned"},
    {Q15_OUT, TRACE, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_KIND output must be 16-byte aligned"},
    {Q15_OUT, AVG | HOPW, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_AVG_KIND output must be 16-byte aligned"},
    {Q15_OUT, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 262144)},
    {Q15_OUT, MARKER, 0, 0, B, IN, IN + 131072 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 64)},
    {Q15_OUT, TRACE, 0, 0, B, IN, IN - 32768 + 16, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 32768)},
    {Q15_OUT, AVG, 0, 0, B, IN, IN - 8192 + 16, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 8192)},
    {Q15_OUT, 0 | HOPW, 0, 0, B, IN, IN + 57344 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(57344, 262144)},
    {Q15_OUT, SA_Q15_TRACE_AVG_KIND(1, 1), 0, 0, 1 << 28, 1ull << 45, 1ull << 46, true, SA_ESHAPE, kSaWorkspace, WORKSPACE},
    // ---- sa_process_q15_p12
    {Q15_P12, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {Q15_P12, MARKER | 2049 << 8, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {Q15_P12, 23, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_P12, AVG, 0, 0, 6, IN, OUT, true, SA_ESHAPE, kSaGroup, GROUP},
    {Q15_P12, 0, 0, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {Q15_P12, 0, 0, 0, B, IN + 1, OUT, true, SA_EINVAL, kSaInAlign, PACKED},
    {Q15_P12, TRACE | HOPW, 0, 0, B, IN + 4, OUT, true, SA_EINVAL, kSaInAlign, PACKED},    // packed wins over "stream"
    {Q15_P12, SA_Q15_OUT_MAG, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {Q15_P12, MARKER | HOPW, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_OUT_MARKER output must be 16-byte aligned"},
    {Q15_P12, TRACE, 0, 0, B, IN, OUT + 4, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_KIND output must be 16-byte aligned"},
    {Q15_P12, AVG, 0, 0, B, IN, OUT + 12, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_AVG_KIND output must be 16-byte aligned"},
    {Q15_P12, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(98304, 262144)},
    {Q15_P12, AVG | HOPW, 0, 0, B, IN, IN + 43008 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(43008, 8192)},
    {Q15_P12, SA_Q15_TRACE_AVG_KIND(2, 7), 0, 0, 1 << 29, 1ull << 46, 1ull << 47, true, SA_ESHAPE, kSaWorkspace, WORKSPACE},
    // ---- sa_filter_q15, sa_filter_q15_p12: no kind
    {FILT, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {FILT, 0, 0, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {FILT, 99, 0, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {FILT, MARKER, 0, 0, B, IN, OUT + 2, true, SA_EINVAL, kSaOutAlign, OUT16},
    {FILT, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 131072)},
    {FILT_P12, 0, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {FILT_P12, 0, 0, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {FILT_P12, 0, 0, 0, B, IN + 3, OUT, true, SA_EINVAL, kSaInAlign, PACKED},
    {FILT_P12, 0, 0, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {FILT_P12, 0, 0, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(98304, 131072)},
    // ---- sa_spectra_q15
    {SPEC, 0, A4, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {SPEC, 0, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {SPEC, 0, 8, 0, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {SPEC, 0, A4, 4, B, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC, 0, A4, 12, B, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC, 0, A4, 16392, B, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC, 0, A4, -8, B, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC, 0, A4, 0, 5, IN, OUT, true, SA_ESHAPE, kSaGroup, XGROUP},
    {SPEC, 0, A4, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {SPEC, 0, A4, 0, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {SPEC, 0, A4, HOP, B, IN + 2, OUT, true, SA_EINVAL, kSaInAlign, XSTREAM},
    {SPEC, 0, A4, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {SPEC, 0, A4, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(131072, 131072)},
    {SPEC, 0, A4, HOP, B, IN, IN + 57344 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(57344, 131072)},
    // ---- sa_spectra_q15_p12
    {SPEC_P12, 0, A4, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {SPEC_P12, 0, -1, 0, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {SPEC_P12, 0, A4, 4100, B, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC_P12, 0, A4, 0, 5, IN, OUT, true, SA_ESHAPE, kSaGroup, XGROUP},
    {SPEC_P12, 0, A4, 0, B, IN, 0, true, SA_EINVAL, kSaNull, NUL},
    {SPEC_P12, 0, A4, 0, B, IN + 1, OUT, true, SA_EINVAL, kSaInAlign, PACKED},
    {SPEC_P12, 0, A4, HOP, B, IN + 4, OUT, true, SA_EINVAL, kSaInAlign, PACKED},
    {SPEC_P12, 0, A4, HOP, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {SPEC_P12, 0, A4, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(98304, 131072)},
    {SPEC_P12, 0, A4, HOP, B, IN, IN - 131072 + 16, true, SA_EINVAL, kSaOverlap, OVERLAP(43008, 131072)},
    // ---- sa_fold_iq_q15
    {FOLD, 0, A4, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {FOLD, 0, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {FOLD, 0, A4, HOP, B, IN, OUT, true, SA_EINVAL, kSaHop, FOLDHOP},
    {FOLD, 0, A4, 4, B, IN, OUT, true, SA_EINVAL, kSaHop, FOLDHOP},
    {FOLD, 0, A4, 0, 5, IN, OUT, true, SA_ESHAPE, kSaGroup, XGROUP},
    {FOLD, 0, A4, 0, B, 0, OUT, true, SA_EINVAL, kSaNull, NUL},
    {FOLD, 0, A4, 0, B, IN + 4, OUT, true, SA_EINVAL, kSaInAlign, IN16},
    {FOLD, 0, A4, 0, B, IN, OUT + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {FOLD, 0, A4, 0, B, IN, IN, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 131072)},
    {FOLD, 0, A4, 0, B, IN, IN + 262144 - 16, true, SA_EINVAL, kSaOverlap, OVERLAP(262144, 131072)},
    // ---- an entry there is not
    {-1, 0, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaEntryRule, ""},
    {11, 0, A4, 0, B, IN, OUT, true, SA_EINVAL, kSaEntryRule, ""},

    // ---- order: each tuple trips two rules or more, the earlier one wins
    // a negative batch before a bad kind, a bad hop word, a scale, bad pointers
    {F32, 99, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {F32_I16, 99, 0, 0, -1, 0, 0, false, SA_ESHAPE, kSaBatch, NEG},
    {Q15_OUT, 99, 0, 0, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {Q15_OUT, 1 << 20, 0, 0, -1, 0, 0, true, SA_ESHAPE, kSaBatch, NEG},
    {Q15_P12, AVG, 0, 0, -3, IN + 1, OUT + 1, true, SA_ESHAPE, kSaBatch, NEG},
    // a bad hop word before a bad kind, at any batch
    {Q15_OUT, 99 | 2049 << 8, 0, 0, B, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {Q15_P12, 3 | 1 << 20, 0, 0, 0, 0, 0, true, SA_EINVAL, kSaHopWord, HOPWORD},
    // a bad kind before a scale that is not finite
    {F32_I16, 99, 0, 0, B, IN, OUT, false, SA_EINVAL, kSaKind, KIND},
    {F32_P12, -1, 0, 0, 0, IN, OUT, false, SA_EINVAL, kSaKind, KIND},
    // a bad kind, a bad hop word and a bad scale at batch 0: refused, the empty batch comes after them
    {F32, 5, 0, 0, 0, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, 3, 0, 0, 0, 0, 0, true, SA_EINVAL, kSaKind, KIND},
    {Q15_P12, 0x88, 0, 0, 0, IN, OUT, true, SA_EINVAL, kSaKind, KIND},
    {Q15_OUT, 0 | 2049 << 8, 0, 0, 0, IN, OUT, true, SA_EINVAL, kSaHopWord, HOPWORD},
    {F32_I16, 0, 0, 0, 0, IN, OUT, false, SA_EINVAL, kSaScale, SCALE},
    // a scale that is not finite before the group, NULL and the pointers
    {F32_P12, 0, 0, 0, B, 0, 0, false, SA_EINVAL, kSaScale, SCALE},
    {F32_I16, SA_OUT_MARKER, 0, 0, B, IN + 2, OUT + 8, false, SA_EINVAL, kSaScale, SCALE},
    // the group before NULL and the pointers
    {Q15_OUT, AVG, 0, 0, 5, 0, 0, true, SA_ESHAPE, kSaGroup, GROUP},
    {Q15_P12, AVG | HOPW, 0, 0, 7, IN + 1, IN + 3, true, SA_ESHAPE, kSaGroup, GROUP},
    {Q15_OUT, AVG, 0, 0, 1, IN, IN, true, SA_ESHAPE, kSaGroup, GROUP},
    // NULL before alignment, overlap and the workspace
    {F32, 0, 0, 0, B, 0, OUT + 1, true, SA_EINVAL, kSaNull, NUL},
    {Q15_OUT, MARKER, 0, 0, B, IN + 2, 0, true, SA_EINVAL, kSaNull, NUL},
    {Q15_OUT, SA_Q15_TRACE_AVG_KIND(1, 1), 0, 0, 1 << 28, 0, 1ull << 46, true, SA_EINVAL, kSaNull, NUL},
    // a marker, a trace and a grouped trace name a misaligned `out` before a misaligned `in` ...
    {F32, SA_OUT_MARKER, 0, 0, B, IN + 4, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_OUT_MARKER output must be 16-byte aligned"},
    {F32_P12, SA_OUT_MARKER, 0, 0, B, IN + 1, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_OUT_MARKER output must be 16-byte aligned"},
    {Q15_OUT, MARKER, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_OUT_MARKER output must be 16-byte aligned"},
    {Q15_OUT, TRACE | HOPW, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_KIND output must be 16-byte aligned"},
    {Q15_P12, AVG, 0, 0, B, IN + 1, OUT + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_TRACE_AVG_KIND output must be 16-byte aligned"},
    // ... every other kind names `in` first, then `out`, then the overlap
    {F32, SA_OUT_MAG_FULL, 0, 0, B, IN + 4, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {F32, SA_OUT_MAG_HALF, 0, 0, B, IN + 4, OUT + 2, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15, 0, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15_OUT, SA_Q15_OUT_IQ, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {Q15_OUT, SA_Q15_OUT_MAG | HOPW, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, STREAM},
    {Q15_P12, SA_Q15_OUT_IQ, 0, 0, B, IN + 1, OUT + 8, true, SA_EINVAL, kSaInAlign, PACKED},
    {FILT, 0, 0, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {SPEC, 0, A4, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {FOLD, 0, A4, 0, B, IN + 2, OUT + 8, true, SA_EINVAL, kSaInAlign, IN16},
    {F32, 0, 0, 0, B, IN + 4, IN + 4, true, SA_EINVAL, kSaInAlign, IN16},                // misaligned and overlapping
    {F32, 0, 0, 0, B, IN, IN + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {Q15_OUT, MARKER, 0, 0, B, IN, IN + 8, true, SA_EINVAL, kSaOutAlign, "SA_Q15_OUT_MARKER output must be 16-byte aligned"},
    {FILT_P12, 0, 0, 0, B, IN, IN + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    {SPEC_P12, 0, A4, 0, B, IN, IN + 8, true, SA_EINVAL, kSaOutAlign, OUT16},
    // the pointers before the workspace
    {Q15_OUT, SA_Q15_TRACE_AVG_KIND(1, 1), 0, 0, 1 << 28, 1ull << 45, (1ull << 45) + 16, true, SA_EINVAL, kSaOverlap,
     OVERLAP(8796093022208, 8796093022208)},
    // ext: a negative batch before a bad log2a and a bad hop; log2a before the hop; both also at batch 0; the group before NULL
    {SPEC, 0, 0, 4, -1, 0, 0, true, SA_ESHAPE, kSaBatch, NEG},
    {SPEC_P12, 0, 8, 0, -128, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {FOLD, 0, 0, HOP, -1, IN, OUT, true, SA_ESHAPE, kSaBatch, NEG},
    {SPEC, 0, 0, 4, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {FOLD, 0, 9, HOP, B, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {SPEC, 0, 0, 0, 0, IN, OUT, true, SA_EINVAL, kSaLog2a, LOG2A},
    {SPEC, 0, A4, 12, 0, IN, OUT, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC_P12, 0, A4, 16392, 0, 0, 0, true, SA_EINVAL, kSaHop, XHOP},
    {FOLD, 0, A4, 8, 0, IN, OUT, true, SA_EINVAL, kSaHop, FOLDHOP},
    {SPEC, 0, A4, 12, 5, 0, 0, true, SA_EINVAL, kSaHop, XHOP},
    {SPEC, 0, A4, HOP, 5, 0, 0, true, SA_ESHAPE, kSaGroup, XGROUP},
    {SPEC_P12, 0, A4, 0, 3, IN + 1, IN + 3, true, SA_ESHAPE, kSaGroup, XGROUP},
    {FOLD, 0, A4, 0, 6, 0, OUT, true, SA_ESHAPE, kSaGroup, XGROUP},
    {SPEC, 0, A4, 0, B, 0, OUT + 8, true, SA_EINVAL, kSaNull, NUL},
    {FOLD, 0, A4, 0, B, IN + 2, 0, true, SA_EINVAL, kSaNull, NUL},
};

// accepted calls, with what the check decodes from them
struct Ok {
    int entry, word, log2a, hop, batch;
    uint64_t in, out;
    int kind, dhop;
    SaFold fold;
    int log2w, dlog2a;
    uint64_t in_bytes, out_bytes;
    unsigned out_align;
};

static const Ok kAccepted[] = {
    {F32, SA_OUT_MAG_FULL, 0, 0, B, IN, OUT, 0, 0, SaFold::None, 0, 0, 262144, 262144, 16},
    {F32, SA_OUT_MAG_HALF, 0, 0, 8, IN, OUT + 4, 1, 0, SaFold::None, 0, 0, 524288, 262176, 4},
    {F32_I16, SA_OUT_SPEC_HALF, 0, 0, B, IN, OUT + 8, 2, 0, SaFold::None, 0, 0, 131072, 262176, 8},
    {F32_P12, SA_OUT_MARKER, 0, 0, B, IN, OUT, 4, 0, SaFold::None, 0, 0, 98304, 64, 16},
    {F32, 0, 0, 0, B, IN, IN + 262144, 0, 0, SaFold::None, 0, 0, 262144, 262144, 16},        // touching, in both orders
    {F32, 0, 0, 0, B, IN, IN - 262144, 0, 0, SaFold::None, 0, 0, 262144, 262144, 16},
    {Q15, 12345, 0, 0, B, IN, OUT, 0, 0, SaFold::None, 0, 0, 131072, 262144, 16},            // the word is not read
    {Q15_OUT, MARKER, 0, 0, B, IN, OUT, 2, 0, SaFold::None, 0, 0, 131072, 64, 16},
    {Q15_OUT, 0x40000, 0, 0, 5, IN, OUT, 0, 8192, SaFold::None, 0, 0, 98304, 327680, 16},
    {Q15_OUT, 0x114, 0, 0, B, IN, OUT, 0x14, 8, SaFold::None, 0, 0, 32816, 32768, 16},
    {Q15_OUT, 0 | 2048 << 8, 0, 0, B, IN, OUT, 0, 16384, SaFold::None, 0, 0, 131072, 262144, 16},
    {Q15_OUT, 0x2009C, 0, 0, 8, IN, OUT, 0x9C, 4096, SaFold::Trace, 4, 3, 90112, 8192, 16},
    {Q15_P12, 0x20002, 0, 0, 5, IN, OUT, 2, 4096, SaFold::None, 0, 0, 49152, 80, 16},
    {Q15_P12, SA_Q15_TRACE_AVG_KIND(6, 7), 0, 0, 256, IN, OUT, 0xBE, 0, SaFold::Trace, 6, 7, 6291456, 4096, 16},
    {Q15_OUT, SA_Q15_TRACE_AVG_KIND(1, 1), 0, 0, (1 << 28) - 2, 1ull << 45, 1ull << 46, 0x89, 0, SaFold::Trace, 1, 1,
     8796092956672, 8796092956672, 16},                                                       // the largest batch of W = 2
    {FILT, 77, 0, 0, B, IN, OUT, 0, 0, SaFold::None, 0, 0, 131072, 131072, 16},
    {FILT_P12, 0, 0, 0, B, IN, OUT, 0, 0, SaFold::None, 0, 0, 98304, 131072, 16},
    {SPEC, 0, 2, 0, 8, IN, IN + 262144, 0, 0, SaFold::Spectra, 0, 2, 262144, 262144, 16},     // the known answers of the header
    {SPEC, 0, 2, 4096, 8, IN, IN + 90112, 0, 4096, SaFold::Spectra, 0, 2, 90112, 262144, 16},
    {SPEC_P12, 0, 2, 4096, 8, IN, IN + 67584, 0, 4096, SaFold::Spectra, 0, 2, 67584, 262144, 16},
    {FOLD, 0, 2, 0, 8, IN, IN - 262144, 0, 0, SaFold::Spectra, 0, 2, 524288, 262144, 16},
    {FOLD, 0, 7, 0, 128, IN, OUT, 0, 0, SaFold::Spectra, 0, 7, 8388608, 131072, 16},
};

// the handle-free export of the entry's header on the same arguments (it has no scale: the check with a finite one)
static int exported(int entry, int word, int log2a, int hop, uint64_t in, uint64_t out, int batch)
{
    return entry >= 8 ? sa_ext_check_pointers(entry - 8, log2a, hop, in, out, batch) : sa_debug_check_pointers(entry, word, in, out, batch);
}

int main()
{
    static_assert(kSaEntryExt == 8 && kSaEntryCount == 11, "the numbering this file writes out");
    for (int e = 0; e < kSaEntryCount; ++e) {
        ++g_checks;
        if (std::strcmp(sa_entry(e).name, NAMES[e]) != 0) {
            std::printf("FAILED entry %d is named %s\n", e, sa_entry(e).name);
            return 1;
        }
    }
    int n = 0;
    for (const T &t : kCases) {
        ++n;
        const SaCall call = {t.entry, t.word, t.log2a, t.hop, t.batch, t.in, t.out, t.finite};
        SaChecked r;
        const int code = sa_check_call(call, &r);
        char text[160] = "?";
        if (t.entry >= 0 && t.entry < kSaEntryCount) sa_refusal_text(t.entry, r, text, sizeof text);
        else text[0] = 0;
        ++g_checks;
        if (code != r.code || r.code != t.code || r.rule != t.rule || std::strcmp(text, t.text) != 0) {
            std::printf("FAILED case %d (entry %d word %#x log2a %d hop %d batch %d): code %d rule %d \"%s\", want %d %d \"%s\"\n", n,
                        t.entry, t.word, t.log2a, t.hop, t.batch, r.code, (int)r.rule, text, t.code, (int)t.rule, t.text);
            return 1;
        }
        SaCall finite = call;
        finite.scale_finite = true;
        SaChecked f;
        const int want = sa_check_call(finite, &f);
        ++g_checks;
        if (t.finite && want != t.code) {
            std::printf("FAILED case %d: the check is not a function of its arguments\n", n);
            return 1;
        }
        // 11 is no entry of either header: -1 stands for it at both exports
        const int got = t.entry == 11 ? sa_ext_check_pointers(3, t.log2a, t.hop, t.in, t.out, t.batch) | sa_debug_check_pointers(8, t.word, t.in, t.out, t.batch)
                        : t.entry < 0 ? sa_ext_check_pointers(-1, t.log2a, t.hop, t.in, t.out, t.batch) | sa_debug_check_pointers(-1, t.word, t.in, t.out, t.batch)
                                      : exported(t.entry, t.word, t.log2a, t.hop, t.in, t.out, t.batch);
        ++g_checks;
        if (got != want) {
            std::printf("FAILED case %d (entry %d): the export returns %d, the check %d\n", n, t.entry, got, want);
            return 1;
        }
    }
    n = 0;
    for (const Ok &k : kAccepted) {
        ++n;
        SaChecked r;
        sa_check_call({k.entry, k.word, k.log2a, k.hop, k.batch, k.in, k.out, true}, &r);
        char text[160] = "?";
        sa_refusal_text(k.entry, r, text, sizeof text);
        ++g_checks;
        if (r.code != SA_OK || r.rule != kSaNone || text[0] != 0 || r.kind != k.kind || r.hop != k.dhop || r.fold != k.fold ||
            r.log2w != k.log2w || r.log2a != k.dlog2a || r.span.in_bytes != k.in_bytes || r.span.out_bytes != k.out_bytes ||
            r.span.in_align != 16 || r.span.out_align != k.out_align) {
            std::printf("FAILED accepted call %d (entry %d): code %d rule %d kind %#x hop %d fold %d log2w %d log2a %d, %llu read, %llu "
                        "written, `out` aligned to %u\n", n, k.entry, r.code, (int)r.rule, r.kind, r.hop, (int)r.fold, r.log2w, r.log2a,
                        (unsigned long long)r.span.in_bytes, (unsigned long long)r.span.out_bytes, r.span.out_align);
            return 1;
        }
        ++g_checks;
        if (exported(k.entry, k.word, k.log2a, k.hop, k.in, k.out, k.batch) != SA_OK) {
            std::printf("FAILED accepted call %d (entry %d): refused by the export\n", n, k.entry);
            return 1;
        }
        // the empty batch of the same call: SA_OK whatever the addresses are, with the word decoded all the same
        SaChecked z;
        sa_check_call({k.entry, k.word, k.log2a, k.hop, 0, 7, 7, true}, &z);
        ++g_checks;
        if (z.code != SA_OK || z.rule != kSaNone || z.kind != k.kind || z.hop != k.dhop || z.fold != k.fold ||
            exported(k.entry, k.word, k.log2a, k.hop, 0, 0, 0) != SA_OK) {
            std::printf("FAILED accepted call %d (entry %d) at batch 0\n", n, k.entry);
            return 1;
        }
    }
    std::printf("ok %d\n", g_checks);
    return 0;
}
