// sa_hold.hpp -- what the two units of libspecan_hold.so share (include/specan_hold.h): the geometry of the one launch and
// the argument check with the text of its refusal.
#pragma once

#include <stdint.h>

#include "../../include/specan_hold.h"

constexpr int kHoldThreads = 256;                              // threads of a workgroup
constexpr int kHoldClassMin = 8;                               // the register classes: AMAX = 8, 16, 32, 64, 128 keys per bin
constexpr int kHoldWideMax = 16;                               // classes up to here: a thread owns the bins of a 16-byte load

// the smallest class that holds a group of A frames
constexpr int hold_class(int group)
{
    int amax = kHoldClassMin;
    while (amax < group) amax *= 2;
    return amax;
}

// bins a thread owns, adjacent: the 4 floats or 2 records of one 16-byte load in the small classes, else one bin
constexpr int hold_bins(int amax, int field)
{
    return amax <= kHoldWideMax ? (field == 0 ? 4 : 2) : 1;
}

static_assert(hold_class(SA_HOLD_GROUP_MAX) == SA_HOLD_GROUP_MAX && SA_N % (4 * kHoldThreads) == 0, "whole workgroups per row");

// The refusals of include/specan_hold.h in their order; `why` (never null) is set to the words of a refusal, "" otherwise.
// Host only: integers and the host array of ranks in, a code out.  Neither function is exported: the library's surface is
// the four names of the header.
__attribute__((visibility("hidden"))) int sa_hold_check_call(int field, uint64_t in_addr, uint64_t out_addr, int rows, int group,
                                                             int q, const int32_t *ranks, const char **why);

// the calling thread's error text, read by sa_hold_last_error()
__attribute__((visibility("hidden"))) void sa_hold_set_error(const char *text);
