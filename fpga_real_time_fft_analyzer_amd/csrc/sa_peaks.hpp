// sa_peaks.hpp -- what the two units of libspecan_peaks.so share (include/specan_peaks.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_peaks.h"

constexpr int kPeaksThreads = 256;                             // threads of a workgroup: one workgroup per row
constexpr int kPeaksBins = SA_N / kPeaksThreads;               // 64 bins per thread, in 16-byte units dealt round robin
static_assert(SA_N % (4 * kPeaksThreads) == 0 && SA_PEAKS_K_MAX <= kPeaksThreads, "whole units per thread; thread r holds record r");

// The refusals of include/specan_peaks.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers in, a code out.  Neither function is exported: the library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_peaks_check_call(int field, uint64_t in_addr, uint64_t out_addr,
                                                              uint64_t count_addr, int rows, int k, uint32_t threshold_bits,
                                                              int lo, int hi, int min_sep, const char **why);

// the calling thread's error text, read by sa_peaks_last_error()
__attribute__((visibility("hidden"))) void sa_peaks_set_error(const char *text);
