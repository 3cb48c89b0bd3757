// sa_signals_check.cpp -- the argument check of sa_signals_f32 (include/specan_signals.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_signals_check.cpp).
#include "sa_signals.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_overlap[160];

struct Range {
    const char *name;
    uint64_t base, bytes;
};

// [a, a + na) and [b, b + nb) meet iff the higher base lies less than the lower range's length above the lower base: a
// difference, so that no sum of an address and a length can wrap.  An empty range (no `thr`) meets nothing.
bool meet(const Range &a, const Range &b)
{
    if (a.bytes == 0 || b.bytes == 0) return false;
    return a.base <= b.base ? b.base - a.base < a.bytes : a.base - b.base < b.bytes;
}

}  // namespace

void sa_signals_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_signals_check_call(int field, uint64_t in_addr, uint64_t thr_addr, uint32_t threshold_bits, uint64_t out_addr,
                          uint64_t stats_addr, int rows, int k, int lo, int hi, int gap, int min_width, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_SIGNALS_IN_MAG || field > SA_SIGNALS_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (k < 1 || k > SA_SIGNALS_K_MAX) return *why = "k must be 1..32", SA_EINVAL;
    if (thr_addr == 0 && threshold_bits > 0x7F800000u)
        return *why = "threshold must be +0.0 .. +inf: no NaN, no sign bit", SA_EINVAL;
    if (lo < 0 || lo >= hi || hi > SA_N) return *why = "the range must be 0 <= lo < hi <= 16384", SA_EINVAL;
    if (gap < 0 || gap > kSigGapMax) return *why = "gap must be 0..16383", SA_EINVAL;
    if (min_width < 1 || min_width > SA_N) return *why = "min_width must be 1..16384", SA_EINVAL;
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0 || stats_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 7) return *why = "`out` must be 8-byte aligned", SA_EINVAL;
    if (stats_addr & 3) return *why = "`stats` must be 4-byte aligned", SA_EINVAL;
    if (thr_addr & 3) return *why = "`thr` must be 4-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const Range r[4] = {{"out", out_addr, R * (uint64_t)k * sizeof(sa_signal)},
                        {"stats", stats_addr, R * (3 * sizeof(int32_t))},
                        {"in", in_addr, R * (SA_N * sizeof(float)) * (field ? 2u : 1u)},
                        {"thr", thr_addr, thr_addr ? R * sizeof(float) : 0}};
    // a written range against every other one; `in` and `thr` are only read and may meet
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (meet(r[a], r[b])) {
                snprintf(t_overlap, sizeof t_overlap, "`%s` (%llu bytes) and `%s` (%llu bytes) overlap", r[a].name,
                         (unsigned long long)r[a].bytes, r[b].name, (unsigned long long)r[b].bytes);
                return *why = t_overlap, SA_EINVAL;
            }
    return SA_OK;
}

extern "C" int sa_signals_check(int field, uint64_t in_addr, uint64_t thr_addr, uint32_t threshold_bits, uint64_t out_addr,
                                uint64_t stats_addr, int rows, int k, int lo, int hi, int gap, int min_width)
{
    const char *why;
    return sa_signals_check_call(field, in_addr, thr_addr, threshold_bits, out_addr, stats_addr, rows, k, lo, hi, gap, min_width,
                                 &why);
}

extern "C" const char *sa_signals_last_error(void)
{
    return t_error;
}
