// sa_hold_check.cpp -- the argument check of sa_hold_f32 (include/specan_hold.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_hold_check.cpp).
#include "sa_hold.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_words[160];

}  // namespace

void sa_hold_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_hold_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows, int group, int q, const int32_t *ranks,
                       const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_HOLD_IN_MAG || field > SA_HOLD_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (group < 2 || group > SA_HOLD_GROUP_MAX) return *why = "group must be 2..128", SA_EINVAL;
    if (q < 1 || q > SA_HOLD_Q_MAX) return *why = "q must be 1..8", SA_EINVAL;
    if (ranks == nullptr) return *why = "NULL ranks", SA_EINVAL;
    for (int j = 0; j < q; ++j)
        if (ranks[j] < 0 || ranks[j] >= group) {
            snprintf(t_words, sizeof t_words, "ranks[%d] = %d is outside 0..%d", j, (int)ranks[j], group - 1);
            return *why = t_words, SA_EINVAL;
        }
    if (rows % group) {
        snprintf(t_words, sizeof t_words, "the rows (%d) must be a multiple of %d", rows, group);
        return *why = t_words, SA_ESHAPE;
    }
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 15) return *why = "`out` must be 16-byte aligned", SA_EINVAL;
    const uint64_t row = SA_N * sizeof(float);                     // rows < 2^31: the largest product is 2^31 2^17 = 2^48
    const uint64_t n_in = (uint64_t)rows * row * (field ? 2u : 1u), n_out = (uint64_t)(rows / group) * (uint64_t)q * row;
    // the two ranges meet iff the higher base lies less than the lower range's length above the lower base: a difference, so
    // that no sum of an address and a length can wrap
    if (in_addr <= out_addr ? out_addr - in_addr < n_in : in_addr - out_addr < n_out) {
        snprintf(t_words, sizeof t_words, "`in` (%llu bytes) and `out` (%llu bytes) overlap", (unsigned long long)n_in,
                 (unsigned long long)n_out);
        return *why = t_words, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_hold_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, int group, int q, const int32_t *ranks)
{
    const char *why;
    return sa_hold_check_call(field, in_addr, out_addr, rows, group, q, ranks, &why);
}

extern "C" const char *sa_hold_last_error(void)
{
    return t_error;
}
