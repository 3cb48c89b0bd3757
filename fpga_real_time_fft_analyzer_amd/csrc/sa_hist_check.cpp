// sa_hist_check.cpp -- the argument check of sa_hist_f32 (include/specan_hist.h) and the calling thread's error text.
// Host only: no HIP runtime, no handle, no environment; every byte count is 64 bits wide and the addresses are compared as
// integers, never dereferenced -- so the unit also builds stand-alone (tests/cpp/test_sa_hist_check.cpp).
#include "sa_hist.hpp"

#include <stdio.h>
#include <string.h>

namespace {

thread_local char t_error[160] = "";
thread_local char t_words[160];

uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

}  // namespace

void sa_hist_set_error(const char *text)
{
    snprintf(t_error, sizeof t_error, "%s", text);
}

int sa_hist_check_call(uint64_t in_addr, uint64_t out_addr, int rows, int group, int log2w, int nlev, const float *edges, int lo,
                       int hi, const char **why)
{
    *why = "";
    if (rows < 0) return *why = "negative rows", SA_ESHAPE;
    if (group < 1 || group > kHistGroupMax) return *why = "group must be 1..16777216", SA_EINVAL;
    if (log2w < 0 || log2w > kHistLog2wMax) return *why = "log2w must be 0..6", SA_EINVAL;
    if (nlev < 2 || nlev > SA_HIST_LEVELS_MAX) return *why = "nlev must be 2..64", SA_EINVAL;
    const int wmask = (1 << log2w) - 1;
    if (lo < 0 || lo >= hi || hi > SA_N || (lo & wmask) || (hi & wmask))
        return *why = "the range must be 0 <= lo < hi <= 16384, both multiples of the bucket", SA_EINVAL;
    if (edges == nullptr) return *why = "NULL edges", SA_EINVAL;
    for (int j = 0; j < nlev - 1; ++j) {
        const uint32_t u = bits_of(edges[j]);
        if (u > 0x7F800000u) {
            snprintf(t_words, sizeof t_words, "edges[%d] (bits %#x) must be +0.0 .. +inf: no NaN, no sign bit", j, (unsigned)u);
            return *why = t_words, SA_EINVAL;
        }
        if (j > 0 && u < bits_of(edges[j - 1])) {
            snprintf(t_words, sizeof t_words, "edges[%d] is below edges[%d]", j, j - 1);
            return *why = t_words, SA_EINVAL;
        }
    }
    if (rows % group != 0) {
        snprintf(t_words, sizeof t_words, "rows (%d) must be a multiple of group (%d)", rows, group);
        return *why = t_words, SA_ESHAPE;
    }
    if (rows == 0) return SA_OK;
    if (in_addr == 0 || out_addr == 0) return *why = "NULL tensor", SA_EINVAL;
    if (in_addr & 15) return *why = "`in` must be 16-byte aligned", SA_EINVAL;
    if (out_addr & 3) return *why = "`out` must be 4-byte aligned", SA_EINVAL;
    // rows below 2^31: 2^48 bytes read at most; G C L 4 is at most 2^31 2^14 2^6 2^2 = 2^53
    const uint64_t n_in = (uint64_t)rows * (SA_N * sizeof(float));
    const uint64_t n_out = (uint64_t)(rows / group) * (uint64_t)((hi - lo) >> log2w) * (uint64_t)nlev * sizeof(uint32_t);
    // the two ranges meet iff the higher base lies less than the lower range's length above the lower base: a difference, so
    // that no sum of an address and a length can wrap
    if (in_addr <= out_addr ? out_addr - in_addr < n_in : in_addr - out_addr < n_out) {
        snprintf(t_words, sizeof t_words, "`in` (%llu bytes) and `out` (%llu bytes) overlap", (unsigned long long)n_in,
                 (unsigned long long)n_out);
        return *why = t_words, SA_EINVAL;
    }
    return SA_OK;
}

extern "C" int sa_hist_check(uint64_t in_addr, uint64_t out_addr, int rows, int group, int log2w, int nlev, const float *edges,
                             int lo, int hi)
{
    const char *why;
    return sa_hist_check_call(in_addr, out_addr, rows, group, log2w, nlev, edges, lo, hi, &why);
}

extern "C" const char *sa_hist_last_error(void)
{
    return t_error;
}
