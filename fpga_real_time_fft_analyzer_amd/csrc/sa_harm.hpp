// sa_harm.hpp -- what the two units of libspecan_harm.so share (include/specan_harm.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/specan_harm.h"

constexpr int kHarmThreads = 256;                              // threads of a workgroup: one workgroup per row
constexpr int kHarmTile = 256;                                 // bins of a wave in one round: a node of tree level 8
constexpr int kHarmTiles = (SA_HARM_TOP_MAX + kHarmTile - 1) / kHarmTile;       // 33: tile 32 is bin 8192 and nothing else
constexpr int kHarmRounds = (kHarmTiles + 3) / 4;              // 9 rounds of four adjacent bins per thread; the last is wave 0's alone
constexpr int kHarmSets = SA_HARM_MAX + 3;                     // the sums of a record: power[10], dist, nad, noise
static_assert(kHarmTiles == 33 && kHarmRounds == 9 && kHarmTile == 4 * 64, "a tile is a wave's quads of one round");
static_assert(2 * SA_HARM_SPAN_MAX + 1 <= kHarmTile, "a tone's band lies in at most two tiles");
static_assert(sizeof(sa_harm_cfg) == 28, "the parameters travel in the kernel's arguments");
static_assert(sizeof(sa_harm_row) == 168 && offsetof(sa_harm_row, dist) == 80 && offsetof(sa_harm_row, bin) == 104 &&
                  offsetof(sa_harm_row, fund) == 144 && offsetof(sa_harm_row, spur_bin) == 156,
              "the record is 13 doubles and 16 words without a gap");

// The refusals of include/specan_harm.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers and the host struct in, a code out.  Neither function is exported: the library's surface is the four
// names of the header.
__attribute__((visibility("hidden"))) int sa_harm_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows,
                                                             const sa_harm_cfg *cfg, const char **why);

// the calling thread's error text, read by sa_harm_last_error()
__attribute__((visibility("hidden"))) void sa_harm_set_error(const char *text);
