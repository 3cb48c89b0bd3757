// sa_bands.hpp -- what the two units of libspecan_bands.so share (include/specan_bands.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_bands.h"

constexpr int kBandsThreads = 256;                             // threads of a workgroup: one workgroup per row
constexpr int kBandsRounds = SA_N / (4 * kBandsThreads);       // 16 rounds of four adjacent bins per thread
constexpr int kBandsTile = 256;                                // bins of a wave in one round: a node of tree level 8
constexpr int kBandsTiles = SA_N / kBandsTile;                 // 64 of them: one per lane of the wave that sums levels 8..13
static_assert(kBandsRounds == 16 && kBandsTiles == 64 && kBandsTile == 4 * 64, "a tile is a wave's quads of one round");
static_assert(sizeof(sa_band) == 8 && SA_BANDS_MAX * sizeof(sa_band) == 128 && SA_BANDS_Q_MAX * sizeof(double) == 32,
              "the bands and the fractions travel in the kernel's arguments");

// The refusals of include/specan_bands.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers and the host arrays of bands and fractions in, a code out.  Neither function is exported: the
// library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_bands_check_call(int field, uint64_t in_addr, uint64_t power_addr, uint64_t cross_addr,
                                                              int rows, int nb, const sa_band *bands, int nq, const double *fracs,
                                                              const char **why);

// the calling thread's error text, read by sa_bands_last_error()
__attribute__((visibility("hidden"))) void sa_bands_set_error(const char *text);
