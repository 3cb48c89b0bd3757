// sa_mask.hpp -- what the two units of libspecan_mask.so share (include/specan_mask.h): the geometry of the launches and the
// argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_mask.h"

constexpr int kMaskThreads = 256;                              // threads of a workgroup: one workgroup per row
constexpr int kMaskRound = 4 * kMaskThreads;                   // bins of a workgroup in one round: four adjacent ones per thread
constexpr int kMaskRounds = SA_N / kMaskRound;                 // 16 rounds
constexpr int kMaskSumThreads = 1024;                          // the one workgroup of the summary launch
static_assert(kMaskRounds == 16 && kMaskRound == 1024, "a round is 1024 bins");
static_assert(sizeof(sa_mask_row) == 40, "a record is ten words");

// The refusals of include/specan_mask.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers in, a code out.  Neither function is exported: the library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_mask_check_call(uint64_t in_addr, int field, uint64_t upper_addr, uint64_t lower_addr,
                                                             int lo, int hi, uint64_t rows_out_addr, uint64_t summary_addr, int rows,
                                                             const char **why);

// the calling thread's error text, read by sa_mask_last_error()
__attribute__((visibility("hidden"))) void sa_mask_set_error(const char *text);
