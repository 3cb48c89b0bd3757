// sa_fold_check.cpp -- the argument check of sa_fold_mag_f32 (include/specan_fold.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_fold_check.cpp).
#include "sa_fold.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_overlap[160];

}  // namespace

void sa_fold_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_fold_check_call(int log2a, int log2w, uint64_t in_addr, uint64_t out_addr, int batch, const char **why)
{
    *why = "";
    if (batch < 0) return *why = "negative batch", SA_ESHAPE;
    if (log2a < 0 || log2a > SA_FOLD_LOG2A_MAX) return *why = "log2a must be 0..7 (groups of A = 1..128 frames)", SA_EINVAL;
    if (log2w < 0 || log2w > SA_FOLD_LOG2W_MAX) return *why = "log2w must be 0..6 (buckets of W = 1..64 bins)", SA_EINVAL;
    if (log2a == 0 && log2w == 0) return *why = "log2a = log2w = 0 folds nothing", SA_EINVAL;
    if (batch == 0) return SA_OK;
    if (batch & ((1 << log2a) - 1)) return *why = "batch must be a multiple of the group size A", SA_ESHAPE;
    const uint64_t B = (uint64_t)batch, groups = B >> log2a;
    if (groups * kFoldBlocksPerGroup > 0x7FFFFFFFull) return *why = "batch too large for one launch (B / A >= 2^27)", SA_ESHAPE;
    if (in_addr == 0 || out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`mag` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 15) return *why = "`out` must be 16-byte aligned", SA_EINVAL;
    const uint64_t in_bytes = B * (SA_N * sizeof(float)), out_bytes = groups * (uint64_t)(SA_N >> log2w) * sizeof(sa_fold_point);
    // [in, in + in_bytes) and [out, out + out_bytes) meet iff the higher base lies less than the lower range's length above
    // the lower base: a difference, so that no sum of an address and a length can wrap
    if (in_addr <= out_addr ? out_addr - in_addr < in_bytes : in_addr - out_addr < out_bytes) {
        snprintf(t_overlap, sizeof t_overlap, "`mag` (%llu bytes read) and `out` (%llu bytes written) overlap",
                 (unsigned long long)in_bytes, (unsigned long long)out_bytes);
        return *why = t_overlap, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_fold_check(int log2a, int log2w, uint64_t in_addr, uint64_t out_addr, int batch)
{
    const char *why;
    return sa_fold_check_call(log2a, log2w, in_addr, out_addr, batch, &why);
}

extern "C" const char *sa_fold_last_error(void)
{
    return t_error;
}
