// sa_bands_check.cpp -- the argument check of sa_bands_f32 (include/specan_bands.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_bands_check.cpp).
#include "sa_bands.hpp"

#include <stdio.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_words[160];

constexpr double kFracMax = 1.0 - 1.0 / 4294967296.0;          // 1 - 2^-32, exact in a double

// the two ranges meet iff the higher base lies less than the lower range's length above the lower base: a difference, so
// that no sum of an address and a length can wrap.  An empty range meets nothing.
bool meet(uint64_t a, uint64_t na, uint64_t b, uint64_t nb)
{
    if (na == 0 || nb == 0) return false;
    return a <= b ? b - a < na : a - b < nb;
}

}  // namespace

void sa_bands_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_bands_check_call(int field, uint64_t in_addr, uint64_t power_addr, uint64_t cross_addr, int rows, int nb,
                        const sa_band *bands, int nq, const double *fracs, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_BANDS_IN_MAG || field > SA_BANDS_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (nb < 1 || nb > SA_BANDS_MAX) return *why = "nb must be 1..16", SA_EINVAL;
    if (bands == nullptr) return *why = "NULL bands", SA_EINVAL;
    for (int j = 0; j < nb; ++j)
        if (bands[j].lo < 0 || bands[j].lo >= bands[j].hi || bands[j].hi > SA_N) {
            snprintf(t_words, sizeof t_words, "bands[%d] = [%d, %d) is not 0 <= lo < hi <= 16384", j, (int)bands[j].lo, (int)bands[j].hi);
            return *why = t_words, SA_EINVAL;
        }
    if (nq < 0 || nq > SA_BANDS_Q_MAX) return *why = "nq must be 0..4", SA_EINVAL;
    if (nq > 0 && fracs == nullptr) return *why = "NULL fracs", SA_EINVAL;
    for (int q = 0; q < nq; ++q)
        if (!(fracs[q] >= 0.0 && fracs[q] <= kFracMax)) {         // a NaN fails both compares
            snprintf(t_words, sizeof t_words, "fracs[%d] = %.17g is outside 0 .. 1 - 2^-32", q, fracs[q]);
            return *why = t_words, SA_EINVAL;
        }
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || power_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (nq > 0 && cross_addr == 0) return *why = "NULL `cross` with nq > 0", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (power_addr & 7) return *why = "`power` must be 8-byte aligned", SA_EINVAL;
    if (nq > 0 && (cross_addr & 3)) return *why = "`cross` must be 4-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const uint64_t n_in = R * (SA_N * sizeof(float)) * (field ? 2u : 1u), n_power = R * (uint64_t)nb * sizeof(double);
    const uint64_t n_cross = R * (uint64_t)nb * (uint64_t)nq * sizeof(int32_t);      // 0 with nq 0: `cross` is not looked at
    const char *pair = meet(in_addr, n_in, power_addr, n_power) ? "`in` and `power`"
                       : meet(in_addr, n_in, cross_addr, n_cross) ? "`in` and `cross`"
                       : meet(power_addr, n_power, cross_addr, n_cross) ? "`power` and `cross`" : nullptr;
    if (pair) {
        snprintf(t_words, sizeof t_words, "%s overlap (%llu, %llu and %llu bytes)", pair, (unsigned long long)n_in,
                 (unsigned long long)n_power, (unsigned long long)n_cross);
        return *why = t_words, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_bands_check(int field, uint64_t in_addr, uint64_t power_addr, uint64_t cross_addr, int rows, int nb,
                              const sa_band *bands, int nq, const double *fracs)
{
    const char *why;
    return sa_bands_check_call(field, in_addr, power_addr, cross_addr, rows, nb, bands, nq, fracs, &why);
}

extern "C" const char *sa_bands_last_error(void)
{
    return t_error;
}
