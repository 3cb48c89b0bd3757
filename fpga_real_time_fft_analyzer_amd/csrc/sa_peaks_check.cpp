// sa_peaks_check.cpp -- the argument check of sa_peaks_f32 (include/specan_peaks.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_peaks_check.cpp).
#include "sa_peaks.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_overlap[160];

struct Range {
    const char *name;
    uint64_t base, bytes;
};

// [a, a + na) and [b, b + nb) meet iff the higher base lies less than the lower range's length above the lower base: a
// difference, so that no sum of an address and a length can wrap
bool meet(const Range &a, const Range &b)
{
    return a.base <= b.base ? b.base - a.base < a.bytes : a.base - b.base < b.bytes;
}

}  // namespace

void sa_peaks_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_peaks_check_call(int field, uint64_t in_addr, uint64_t out_addr, uint64_t count_addr, int rows, int k,
                        uint32_t threshold_bits, int lo, int hi, int min_sep, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_PEAKS_IN_MAG || field > SA_PEAKS_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (k < 1 || k > SA_PEAKS_K_MAX) return *why = "k must be 1..32", SA_EINVAL;
    if (threshold_bits > 0x7F800000u) return *why = "threshold must be +0.0 .. +inf: no NaN, no sign bit", SA_EINVAL;
    if (lo < 0 || lo >= hi || hi > SA_N) return *why = "the range must be 0 <= lo < hi <= 16384", SA_EINVAL;
    if (min_sep < 1 || min_sep > SA_N) return *why = "min_sep must be 1..16384", SA_EINVAL;
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0 || count_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 7) return *why = "`out` must be 8-byte aligned", SA_EINVAL;
    if (count_addr & 3) return *why = "`count` must be 4-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const Range r[3] = {{"in", in_addr, R * (SA_N * sizeof(float)) * (field ? 2u : 1u)},
                        {"out", out_addr, R * (uint64_t)k * sizeof(sa_peak)},
                        {"count", count_addr, R * sizeof(int32_t)}};
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (meet(r[a], r[b])) {
                snprintf(t_overlap, sizeof t_overlap, "`%s` (%llu bytes) and `%s` (%llu bytes) overlap", r[a].name,
                         (unsigned long long)r[a].bytes, r[b].name, (unsigned long long)r[b].bytes);
                return *why = t_overlap, SA_EINVAL;
            }
    return SA_OK;
}

extern "C" int sa_peaks_check(int field, uint64_t in_addr, uint64_t out_addr, uint64_t count_addr, int rows, int k,
                              uint32_t threshold_bits, int lo, int hi, int min_sep)
{
    const char *why;
    return sa_peaks_check_call(field, in_addr, out_addr, count_addr, rows, k, threshold_bits, lo, hi, min_sep, &why);
}

extern "C" const char *sa_peaks_last_error(void)
{
    return t_error;
}
