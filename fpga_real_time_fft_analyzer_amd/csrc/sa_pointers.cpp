// sa_pointers.cpp -- of the argument check of every data-plane call (sa_check_call, sa_pointers.hpp): the half that looks at
// the addresses, the words of its refusals and its two handle-free debug exports.  Every byte count is 64 bits wide
// (40 000 float frames are 2.6 GB) and addresses are compared as integers, never dereferenced.
#include "sa_pointers.hpp"

#include <stdio.h>

namespace {

// bytes of one frame of input, by input form
uint64_t in_frame_bytes(int in_form)
{
    return in_form == kSaInF32 || in_form == kSaInIQ ? kSaN * 4 : in_form == kSaInI16 ? kSaN * 2 : SA_P12_FRAME_BYTES;
}

// the name under which a misaligned `out` of this kind is refused before a misaligned `in`; null for every other kind
const char *named_out(const SaEntry &e, int kind)
{
    return sa_is_trace_avg(e, kind) ? "SA_Q15_TRACE_AVG_KIND"
           : sa_is_trace(e, kind) ? "SA_Q15_TRACE_KIND"
           : kind == e.marker    ? e.marker_name
                                 : nullptr;
}

}  // namespace

// The second half of the check, for a batch > 0 that is a multiple of its group: NULL, the byte counts, alignment, overlap
// and the workspace of the grouped trace.  `out_row` is what sa_out_row_bytes gave for r.kind.
int sa_check_addresses(const SaCall &c, const SaEntry &e, uint64_t out_row, SaChecked &r)
{
    if (c.in == 0 || c.out == 0) return sa_refuse(r, SA_EINVAL, kSaNull);
    const uint64_t B = (uint64_t)c.batch;
    r.span.out_bytes = (B >> r.log2a) * out_row;
    if (r.hop == 0) {
        r.span.in_bytes = B * in_frame_bytes(e.in_form);
    } else {                                   // one stream: the last frame ends with it
        const uint64_t samples = (B - 1) * (uint64_t)r.hop + kSaN;
        r.span.in_bytes = e.in_form == kSaInP12 ? samples / 2 * 3 : samples * 2;      // hop is even: so is `samples`
    }
    const bool in_off = c.in & (uint64_t)(r.span.in_align - 1), out_off = c.out & (uint64_t)(r.span.out_align - 1);
    if (out_off && named_out(e, r.kind)) return sa_refuse(r, SA_EINVAL, kSaOutAlign);
    if (in_off) return sa_refuse(r, SA_EINVAL, kSaInAlign);
    if (out_off) return sa_refuse(r, SA_EINVAL, kSaOutAlign);
    // [in, in + in_bytes) and [out, out + out_bytes) meet iff the higher base lies less than the lower range's length
    // above the lower base: a difference, so that no sum of an address and a length can wrap
    if (c.in <= c.out ? c.out - c.in < r.span.in_bytes : c.in - c.out < r.span.out_bytes)
        return sa_refuse(r, SA_EINVAL, kSaOverlap);
    // the FFT launch of SA_Q15_TRACE_AVG_KIND(k, a) writes B (16384 >> k) partial records into a workspace that the handle
    // sizes in frames of 16384 elements, here ceil(16 B / W) frames of bytes, and that count is an int
    if (r.fold == SaFold::Trace && ((B * kSaTraceRawRecord + (1u << r.log2w) - 1) >> r.log2w) > 0x7FFFFFFF)
        return sa_refuse(r, SA_ESHAPE, kSaWorkspace);
    return SA_OK;
}

void sa_refusal_text(int entry, const SaChecked &r, char *buf, size_t cap)
{
    if (r.rule == kSaNone || r.rule == kSaEntryRule) {         // the entry itself may be what is out of range
        snprintf(buf, cap, "%s", "");
        return;
    }
    const SaEntry &e = kSaEntries[entry];
    const bool ext = e.args == SaArgs::Ext;
    const char *what = "";
    switch (r.rule) {
        case kSaBatch: what = "negative batch"; break;
        case kSaHopWord: what = "bad out_kind: hop field above 2048 or bits 20..30 set"; break;
        case kSaLog2a: what = "log2a must be 1..7 (groups of A = 2..128 frames)"; break;
        case kSaHop: what = e.ext_hop ? "hop must be 0 or a multiple of 8 in 8..16384" : "the fold takes frames: no hop"; break;
        case kSaKind: what = "bad out_kind"; break;
        case kSaScale: what = "scale is not finite"; break;
        case kSaGroup:
            what = ext ? "batch must be a multiple of the group size A"
                       : "SA_Q15_TRACE_AVG_KIND: batch must be a multiple of the group size A";
            break;
        case kSaNull: what = "NULL tensor"; break;
        case kSaInAlign:      // the stage-ins and tile loads issue 16-byte requests; every frame is then aligned (int16
            what = e.in_form == kSaInP12 ? "packed input must be 16-byte aligned"      // streams: 16 h bytes apart; packed
                   : r.hop == 0          ? "`in` must be 16-byte aligned"      // streams need a dword per frame and have it)
                   : ext                 ? "a sample stream must be 16-byte aligned"
                                         : "a sample stream (SA_Q15_HOP_KIND) must be 16-byte aligned";
            break;
        case kSaOutAlign:
            if (const char *name = named_out(e, r.kind)) snprintf(buf, cap, "%s output must be 16-byte aligned", name);
            else snprintf(buf, cap, "`out` must be %u-byte aligned", r.span.out_align);
            return;
        case kSaOverlap:
            snprintf(buf, cap, "`in` (%llu bytes read) and `out` (%llu bytes written) overlap",
                     (unsigned long long)r.span.in_bytes, (unsigned long long)r.span.out_bytes);
            return;
        case kSaWorkspace: what = "SA_Q15_TRACE_AVG_KIND: batch too large for the workspace"; break;
        default: break;
    }
    snprintf(buf, cap, "%s", what);
}

extern "C" int sa_debug_check_pointers(int entry, int kind_word, uint64_t in_addr, uint64_t out_addr, int batch)
{
    if (entry < 0 || entry >= SA_ENTRY_COUNT) return SA_EINVAL;
    SaChecked r;
    return sa_check_call({entry, kind_word, 0, 0, batch, in_addr, out_addr, true}, &r);
}

extern "C" int sa_ext_check_pointers(int entry, int log2a, int hop, uint64_t in_addr, uint64_t out_addr, int batch)
{
    if (entry < 0 || entry >= SA_EXT_ENTRY_COUNT) return SA_EINVAL;
    SaChecked r;
    return sa_check_call({kSaEntryExt + entry, 0, log2a, hop, batch, in_addr, out_addr, true}, &r);
}
