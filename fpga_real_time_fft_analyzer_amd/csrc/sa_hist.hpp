// sa_hist.hpp -- what the two units of libspecan_hist.so share (include/specan_hist.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_hist.h"

constexpr int kHistTile = 256;                                 // bins of a workgroup's tile: one 16-byte unit per lane of a wave
constexpr int kHistTiles = SA_N / kHistTile;                   // 64 tiles across a row
constexpr int kHistWavesMin = 4, kHistWavesMax = 16;           // waves of a workgroup: one per row of the group within these
// G x tiles owning workgroups below kHistOwnersFew: the rows of a group are cut into slices, aiming at kHistOwnersAim
// workgroups, no slice shorter than kHistSliceRowsMin rows; the slices merge with integer atomics into a zeroed output
constexpr int kHistOwnersFew = 256, kHistOwnersAim = 512, kHistSliceRowsMin = 32;
constexpr int kHistGroupMax = 1 << 24;
constexpr int kHistLog2wMax = 6;
static_assert(SA_N % kHistTile == 0 && kHistTile == 4 * 64 && (kHistTile >> kHistLog2wMax) >= 4, "a quad of bins per lane");
static_assert(SA_HIST_LEVELS_MAX == 64, "the edge tree has six levels");

// The refusals of include/specan_hist.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers and the host array of edges in, a code out.  Neither function is exported: the library's surface is
// the four names of the header.
__attribute__((visibility("hidden"))) int sa_hist_check_call(uint64_t in_addr, uint64_t out_addr, int rows, int group, int log2w,
                                                             int nlev, const float *edges, int lo, int hi, const char **why);

// the calling thread's error text, read by sa_hist_last_error()
__attribute__((visibility("hidden"))) void sa_hist_set_error(const char *text);
