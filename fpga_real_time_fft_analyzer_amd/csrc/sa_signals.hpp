// sa_signals.hpp -- what the two units of libspecan_signals.so share (include/specan_signals.h): the geometry of the one
// launch and the argument check with the text of its refusal.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/specan_signals.h"

constexpr int kSigThreads = 256;                               // threads of a workgroup: one workgroup per row
constexpr int kSigTile = 256;                                  // bins of a wave in one round: a node of tree level 8
constexpr int kSigTiles = SA_N / kSigTile;                     // 64: the tile nodes are the lanes of one wave
constexpr int kSigRounds = kSigTiles / 4;                      // 16 rounds of four adjacent bins per thread
constexpr int kSigWords = SA_N / 64;                           // the on-mask of a row: one word of 64 bins per thread
constexpr int kSigGapMax = SA_N - 1;
static_assert(kSigTiles == 64 && kSigRounds == 16 && kSigTile == 4 * 64, "a tile is a wave's quads of one round");
static_assert(kSigWords == kSigThreads, "a thread owns one word of the on-mask");
static_assert(6 * SA_SIGNALS_K_MAX <= kSigThreads, "a thread stores one word of one unused slot");
static_assert(sizeof(sa_signal) == 24 && offsetof(sa_signal, peak) == 8 && offsetof(sa_signal, peak_bin) == 12 &&
                  offsetof(sa_signal, power) == 16,
              "the record is four words and a double without a gap");

// The refusals of include/specan_signals.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers in, a code out.  Neither function is exported: the library's surface is the four names of the header.
__attribute__((visibility("hidden"))) int sa_signals_check_call(int field, uint64_t in_addr, uint64_t thr_addr,
                                                                uint32_t threshold_bits, uint64_t out_addr, uint64_t stats_addr,
                                                                int rows, int k, int lo, int hi, int gap, int min_width,
                                                                const char **why);

// the calling thread's error text, read by sa_signals_last_error()
__attribute__((visibility("hidden"))) void sa_signals_set_error(const char *text);
