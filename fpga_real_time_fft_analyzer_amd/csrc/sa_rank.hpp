// sa_rank.hpp -- what the two units of libspecan_rank.so share (include/specan_rank.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_rank.h"

constexpr int kRankThreads = 256;                              // threads of a workgroup: one workgroup per row
constexpr int kRankBins = SA_N / kRankThreads;                 // 64 bins per thread, in 16-byte units dealt round robin
constexpr int kRankKeyBits = 31;                               // a key is a float's bits without the sign: one round per bit
static_assert(SA_N % (4 * kRankThreads) == 0 && SA_RANK_Q_MAX <= 64, "whole units per thread; lane j holds rank j");

// The refusals of include/specan_rank.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers and the host array of ranks in, a code out.  Neither function is exported: the library's surface is
// the four names of the header.
__attribute__((visibility("hidden"))) int sa_rank_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows, int q,
                                                             const int32_t *ranks, int lo, int hi, const char **why);

// the calling thread's error text, read by sa_rank_last_error()
__attribute__((visibility("hidden"))) void sa_rank_set_error(const char *text);
