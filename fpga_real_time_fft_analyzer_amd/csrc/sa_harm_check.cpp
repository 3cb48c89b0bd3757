// sa_harm_check.cpp -- the argument check of sa_harm_f32 (include/specan_harm.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_harm_check.cpp).
#include "sa_harm.hpp"

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

const char *words(const char *what, const sa_harm_cfg &c)
{
    snprintf(t_words, sizeof t_words, "%s (dc %d, top %d, lo %d, hi %d, fund %d, span %d, order %d)", what, (int)c.dc, (int)c.top,
             (int)c.lo, (int)c.hi, (int)c.fund, (int)c.span, (int)c.order);
    return t_words;
}

}  // namespace

void sa_harm_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_harm_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows, const sa_harm_cfg *cfg, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (field < SA_HARM_IN_MAG || field > SA_HARM_IN_POINT_POWER) return *why = "field must be 0, 1 or 2", SA_EINVAL;
    if (cfg == nullptr) return *why = "NULL cfg", SA_EINVAL;
    const sa_harm_cfg &c = *cfg;
    if (c.dc < 0 || c.dc >= c.top || c.top > SA_HARM_TOP_MAX) return *why = words("not 0 <= dc < top <= 8193", c), SA_EINVAL;
    if (c.lo < c.dc || c.lo >= c.hi || c.hi > c.top) return *why = words("not dc <= lo < hi <= top", c), SA_EINVAL;
    if (c.fund != -1 && (c.fund < c.dc || c.fund >= c.top)) return *why = words("fund is neither -1 nor in [dc, top)", c), SA_EINVAL;
    if (c.span < 0 || c.span > SA_HARM_SPAN_MAX) return *why = words("span must be 0..64", c), SA_EINVAL;
    if (c.order < 1 || c.order > SA_HARM_MAX) return *why = words("order must be 1..10", c), SA_EINVAL;
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 7) return *why = "`out` must be 8-byte aligned", SA_EINVAL;
    const uint64_t R = (uint64_t)rows;                             // below 2^31: the largest product is 2^31 2^17 = 2^48
    const uint64_t n_in = R * (SA_N * sizeof(float)) * (field ? 2u : 1u), n_out = R * sizeof(sa_harm_row);
    if (meet(in_addr, n_in, out_addr, n_out)) {
        snprintf(t_words, sizeof t_words, "`in` and `out` overlap (%llu and %llu bytes)", (unsigned long long)n_in,
                 (unsigned long long)n_out);
        return *why = t_words, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_harm_check(int field, uint64_t in_addr, uint64_t out_addr, int rows, const sa_harm_cfg *cfg)
{
    const char *why;
    return sa_harm_check_call(field, in_addr, out_addr, rows, cfg, &why);
}

extern "C" const char *sa_harm_last_error(void)
{
    return t_error;
}
