// sa_fold.hpp -- what the two units of libspecan_fold.so share (include/specan_fold.h): the geometry of the one launch, which
// the argument check has to know for its workgroup bound, and the check itself with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_fold.h"

constexpr int kFoldThreads = 256;                              // threads of a workgroup, each on four adjacent bins of one group
constexpr int kFoldLog2Quads = 12;                             // 16-byte quads of bins per frame: 4096
constexpr int kFoldBlocksPerGroup = (1 << kFoldLog2Quads) / kFoldThreads;      // 16: no partial workgroup at any batch
static_assert(SA_N == 4 << kFoldLog2Quads && (1 << kFoldLog2Quads) % kFoldThreads == 0, "whole workgroups per group of frames");

// The refusals of include/specan_fold.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers in, a code out.  Neither function is exported: the library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_fold_check_call(int log2a, int log2w, uint64_t in_addr, uint64_t out_addr,
                                                             int batch, const char **why);

// the calling thread's error text, read by sa_fold_last_error()
__attribute__((visibility("hidden"))) void sa_fold_set_error(const char *text);
