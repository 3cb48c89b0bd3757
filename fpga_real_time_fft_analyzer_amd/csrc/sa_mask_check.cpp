// sa_mask_check.cpp -- the argument check of sa_mask_f32 (include/specan_mask.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_mask_check.cpp).
#include "sa_mask.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_words[160];

// the two ranges meet iff the higher base lies less than the lower range's length above the lower base: a difference, so
// that no sum of an address and a length can wrap.  An empty range meets nothing.
bool meet(uint64_t a, uint64_t na, uint64_t b, uint64_t nb)
{
    if (na == 0 || nb == 0) return false;
    return a <= b ? b - a < na : a - b < nb;
}

}  // namespace

void sa_mask_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_mask_check_call(uint64_t in_addr, int field, uint64_t upper_addr, uint64_t lower_addr, int lo, int hi, uint64_t rows_out_addr,
                       uint64_t summary_addr, int rows, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_MASK_IN_MAG || field > SA_MASK_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (lo < 0 || lo >= hi || hi > SA_N) {
        snprintf(t_words, sizeof t_words, "[%d, %d) is not 0 <= lo < hi <= 16384", lo, hi);
        return *why = t_words, SA_EINVAL;
    }
    if (upper_addr == 0 && lower_addr == 0) return *why = "NULL `upper` and `lower`: no limit at all", SA_EINVAL;
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || rows_out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (upper_addr & 15) return *why = "`upper` must be 16-byte aligned", SA_EINVAL;
    if (lower_addr & 15) return *why = "`lower` must be 16-byte aligned", SA_EINVAL;
    if (rows_out_addr & 7) return *why = "`rows_out` must be 8-byte aligned", SA_EINVAL;
    if (summary_addr & 3) return *why = "`summary` must be 4-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const char *name[5] = {"`in`", "`upper`", "`lower`", "`rows_out`", "`summary`"};
    const uint64_t addr[5] = {in_addr, upper_addr, lower_addr, rows_out_addr, summary_addr};
    const uint64_t size[5] = {R * (SA_N * sizeof(float)) * (field ? 2u : 1u), upper_addr ? SA_N * sizeof(float) : 0,
                              lower_addr ? SA_N * sizeof(float) : 0, R * sizeof(sa_mask_row), summary_addr ? 4 * sizeof(int32_t) : 0};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) {
            if (i == 1 && j == 2 && upper_addr == lower_addr) continue;      // one line as both limits: only read
            if (meet(addr[i], size[i], addr[j], size[j])) {
                snprintf(t_words, sizeof t_words, "%s and %s overlap (%llu and %llu bytes)", name[i], name[j], (unsigned long long)size[i],
                         (unsigned long long)size[j]);
                return *why = t_words, SA_EINVAL;
            }
        }
    return SA_OK;
}

extern "C" int sa_mask_check(uint64_t in_addr, int field, uint64_t upper_addr, uint64_t lower_addr, int lo, int hi,
                             uint64_t rows_out_addr, uint64_t summary_addr, int rows)
{
    const char *why;
    return sa_mask_check_call(in_addr, field, upper_addr, lower_addr, lo, hi, rows_out_addr, summary_addr, rows, &why);
}

extern "C" const char *sa_mask_last_error(void)
{
    return t_error;
}
