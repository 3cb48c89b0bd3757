// sa_cfar.hpp -- what the two units of libspecan_cfar.so share (include/specan_cfar.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/specan_cfar.h"

constexpr int kCfarThreads = 256;                              // threads of a workgroup: one workgroup per row
constexpr int kCfarRounds = SA_N / (4 * kCfarThreads);         // 16 rounds of four adjacent bins per thread
constexpr int kCfarTile = 2048;                                // bins of a tile: two rounds
constexpr int kCfarTiles = SA_N / kCfarTile;                   // 8 tiles of a row, one after the other
constexpr int kCfarTrainMax = 1 << SA_CFAR_LOG2_TRAIN_MAX;     // 64
// the halo of a tile, fixed at its largest so that every index is known at compile time: bin i reads W[i - G - T], the
// cells i - G - T .. i - G - 1, and W[i + G + 1], the cells i + G + 1 .. i + G + T -- G + T cells on either side of the tile
constexpr int kCfarHalo = SA_CFAR_GUARD_MAX + kCfarTrainMax;                           // 128
constexpr int kCfarCells = kCfarHalo + kCfarTile + kCfarHalo;                          // 2304 cells of a tile's image in LDS
static_assert(kCfarRounds == 16 && kCfarTile == 2 * 4 * kCfarThreads, "a tile is two rounds");
static_assert(kCfarHalo % 4 == 0 && kCfarHalo <= 4 * kCfarThreads, "a halo is whole quads of one neighbouring round");

// The refusals of include/specan_cfar.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers in, a code out.  Neither function is exported: the library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_cfar_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows,
                                                             int log2_train, int guard, int mode, int what, int lo, int hi,
                                                             const char **why);

// the calling thread's error text, read by sa_cfar_last_error()
__attribute__((visibility("hidden"))) void sa_cfar_set_error(const char *text);
