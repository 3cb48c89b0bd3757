// sa_pointers.hpp -- the pointer contract of the process and filter calls (include/specan.h, "pointer contract"): how many
// bytes a call reads through `in` and writes through `out`, the alignment each must have, and the test that the two byte
// ranges are disjoint.  Pure integer arithmetic on addresses that are never dereferenced: no handle, no stream and no HIP
// runtime call, so tests/test_pointer_contract_cpu.py (through sa_debug_check_pointers) and tests/cpp/test_sa_pointers.cpp
// run the whole matrix without a GPU.  check_process_args (specan_abi.cpp) asks the same two functions before any call
// state exists.  The calls of include/specan_ext.h have their argument and pointer checks here too (sa_ext_check, with
// sa_ext_check_pointers as its export and tests/cpp/test_sa_ext_pointers.cpp as its stand-alone test).
#pragma once
#include <stdint.h>

#pragma GCC visibility push(hidden)

// which family of outputs the entry point has: the float chain (SA_OUT_*), the integer chain with its FFT (SA_Q15_OUT_*,
// SA_Q15_TRACE_KIND, SA_Q15_TRACE_AVG_KIND) or the integer chain without it (sa_filter_q15*: one output, no kind)
enum class SaChain { Float, Q15, Q15Filter };

// what `in` points to; the values of SaInKind (sa_common.hpp), which this unit does not include: it pulls in the HIP runtime
enum { kSaInF32 = 0, kSaInI16 = 1, kSaInP12 = 2 };

struct SaCallSpan {
    uint64_t in_bytes, out_bytes;      // the call reads [in, in + in_bytes) and writes [out, out + out_bytes)
    unsigned in_align, out_align;      // powers of two
};

// The span of a call on `batch` > 0 frames: `out_kind` is a kind of `chain` (ignored for Q15Filter), `hop` 0 for frames or
// the hop in samples (8..16384) of a stream, which holds (batch - 1) * hop + 16384 samples.  False for an input form, a
// kind or a hop the chain does not have.
bool sa_call_span(SaChain chain, int in_form, int out_kind, int hop, int batch, SaCallSpan *s);

// The number of frames one row of `out` stands for: A = 2^a for SA_Q15_TRACE_AVG_KIND(k, a) of the Q15 chain, 1 for every
// other kind there is (and for one there is not: sa_call_span is what refuses a kind).  A call's batch must be a multiple
// of it (SA_ESHAPE), and sa_call_span counts batch / A rows of output.
int sa_frames_per_row(SaChain chain, int out_kind);

// What is wrong with the pair of addresses, as a set: every fault is reported, the caller chooses which one to name
enum : unsigned { kSaPtrInAlign = 1u, kSaPtrOutAlign = 2u, kSaPtrOverlap = 4u };
unsigned sa_pointer_faults(const SaCallSpan &s, uint64_t in, uint64_t out);

// ---- the calls of include/specan_ext.h (sa_spectra_q15, sa_spectra_q15_p12, sa_fold_iq_q15; `entry` = SA_EXT_ENTRY_*): every
// refusal the header lists, in its order, as one function.  Returns SA_OK, SA_EINVAL or SA_ESHAPE; `why` says which rule
// refused (the entry points choose their message by it; kSaExtNone with SA_OK) and, from kSaExtNull on, `span` holds the byte
// counts of the call: what the Q15 chain reads for that input form and hop (the fold: batch * 65536) and
// (batch >> log2a) * 131072 written.  batch == 0 that passes the argument checks is SA_OK with the addresses unread.
enum SaExtWhy { kSaExtNone, kSaExtEntry, kSaExtBatch, kSaExtLog2a, kSaExtHop, kSaExtGroup, kSaExtNull, kSaExtInAlign, kSaExtOutAlign,
                kSaExtOverlap };
int sa_ext_check(int entry, int log2a, int hop, uint64_t in, uint64_t out, int batch, SaExtWhy *why, SaCallSpan *span);

#pragma GCC visibility pop
