// sa_cfar_check.cpp -- the argument check of sa_cfar_f32 (include/specan_cfar.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_cfar_check.cpp).
#include "sa_cfar.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_overlap[160];

// [a, a + na) and [b, b + nb) meet iff the higher base lies less than the lower range's length above the lower base: a
// difference, so that no sum of an address and a length can wrap.
bool meet(uint64_t a, uint64_t na, uint64_t b, uint64_t nb)
{
    if (na == 0 || nb == 0) return false;
    return a <= b ? b - a < na : a - b < nb;
}

}  // namespace

void sa_cfar_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_cfar_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows, int log2_train, int guard, int mode, int what,
                       int lo, int hi, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_CFAR_IN_MAG || field > SA_CFAR_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (mode < SA_CFAR_MODE_CA || mode > SA_CFAR_MODE_SO) return *why = "mode must be 0, 1 or 2", SA_EINVAL;
    if (what < SA_CFAR_OUT_RATIO || what > SA_CFAR_OUT_FLOOR) return *why = "what must be 0 or 1", SA_EINVAL;
    if (log2_train < 0 || log2_train > SA_CFAR_LOG2_TRAIN_MAX) return *why = "log2_train must be 0..6", SA_EINVAL;
    if (guard < 0 || guard > SA_CFAR_GUARD_MAX) return *why = "guard must be 0..64", SA_EINVAL;
    if (lo < 0 || lo >= hi || hi > SA_N) return *why = "the range must be 0 <= lo < hi <= 16384", SA_EINVAL;
    if (hi - lo < 2 * guard + 2) return *why = "the range must hold 2 * guard + 2 bins or more", SA_EINVAL;
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 15) return *why = "`out` must be 16-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const uint64_t out_bytes = R * (SA_N * sizeof(float)), in_bytes = out_bytes * (field ? 2u : 1u);
    if (meet(out_addr, out_bytes, in_addr, in_bytes)) {
        snprintf(t_overlap, sizeof t_overlap, "`out` (%llu bytes) and `in` (%llu bytes) overlap", (unsigned long long)out_bytes,
                 (unsigned long long)in_bytes);
        return *why = t_overlap, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_cfar_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, int log2_train, int guard, int mode,
                             int what, int lo, int hi)
{
    const char *why;
    return sa_cfar_check_call(field, in_addr, out_addr, rows, log2_train, guard, mode, what, lo, hi, &why);
}

extern "C" const char *sa_cfar_last_error(void)
{
    return t_error;
}
