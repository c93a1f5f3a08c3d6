// limit_logic.h -- the eligibility rule of a maximum token length, shared by the pair-table insert
// (yabpe_kernels.h, gt_add_from) and by the host code that validates the option (yabpe.hip).
//
// A pair (left, right) may be merged only while len(left) + len(right) <= limit, lengths in bytes; limit 0 = no limit.
// The answer depends on the two tokens alone and a token's bytes never change, so it is the same for the whole life of
// a pair: a pair that fails it is never put into a pair table at all.
#pragma once
#include <stdint.h>

#include "tile_logic.h"

// smallest limit that means anything: two single bytes must be able to merge
#define YB_LIMIT_MIN 2u

YB_HD bool yb_limit_valid(long long limit) { return limit == 0 || (limit >= (long long)YB_LIMIT_MIN && limit <= 0xFFFFFFFFll); }
YB_HD bool yb_pair_fits(uint32_t len_left, uint32_t len_right, uint32_t limit) {
    return limit == 0u || (unsigned long long)len_left + len_right <= (unsigned long long)limit;
}
