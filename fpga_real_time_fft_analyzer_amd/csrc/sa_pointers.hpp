// sa_pointers.hpp -- the pointer contract of the process and filter calls (include/specan.h, "pointer contract"): how many
// bytes a call reads through `in` and writes through `out`, the alignment each must have, and the test that the two byte
// ranges are disjoint.  Pure integer arithmetic on addresses that are never dereferenced: no handle, no stream and no HIP
// runtime call, so tests/test_pointer_contract_cpu.py (through sa_debug_check_pointers) and tests/cpp/test_sa_pointers.cpp
// run the whole matrix without a GPU.  check_process_args (specan_abi.cpp) asks the same two functions before any call
// state exists.
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

#pragma GCC visibility pop
