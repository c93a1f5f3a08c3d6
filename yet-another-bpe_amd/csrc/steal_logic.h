// steal_logic.h -- the arithmetic of the sparse launch's second round (the k_scan_skip row): how the tiles
// behind the first round of chunks are cut into pieces, and the tagged counter the workgroups take those pieces from.
// Shared by k_scan_skip (yabpe_kernels.h), the host that sizes the launch (yabpe.hip) and the CPU model
// (tests/hostmodel/steal_model.cpp).
//
// The counter is ONE 64-bit word that is never cleared between launches: [launch tag : 40 | pieces handed out : 24].
// The host passes a tag that grows with every launch.  A claim is an add of 1; the value it returns names the piece if its
// tag is this launch's.  If the tag is older, the word still belongs to an earlier launch: the claimer raises it to
// (tag, 0) with a max -- which does nothing if somebody else has done so already -- and adds again.  The add that hit the
// old word only changed the old word's count, which nobody reads any more.
#pragma once
#include <stdint.h>

#include "tile_logic.h"

#define YB_STEAL_TAG_SHIFT 24
#define YB_STEAL_IDX_MASK ((1ull << YB_STEAL_TAG_SHIFT) - 1ull)
// (a launch adds at most pieces + 2 x workgroups: 2^21 chunks of 2,048 tiles in a stream of 2^32 tiles, 2,048 workgroups)

YB_HD unsigned long long yb_steal_arm(unsigned long long tag) { return tag << YB_STEAL_TAG_SHIFT; }
YB_HD bool yb_steal_current(unsigned long long word, unsigned long long tag) { return (word >> YB_STEAL_TAG_SHIFT) == tag; }
YB_HD uint32_t yb_steal_idx(unsigned long long word) { return (uint32_t)(word & YB_STEAL_IDX_MASK); }

// The claim itself, over anything that has add(v) and max(v) returning / applying to the counter word atomically.
template <class Ops>
YB_HD uint32_t yb_steal_claim(Ops &ops, unsigned long long tag) {
    unsigned long long old = ops.add(1ull);
    if (!yb_steal_current(old, tag)) {
        ops.max(yb_steal_arm(tag));
        old = ops.add(1ull);
    }
    return yb_steal_idx(old);
}

// Second round: the first `blocks` chunks of `chunk` tiles are dealt by workgroup index; the `rest` tiles behind them are cut
// into pieces of this many tiles (a multiple of 64, at most a chunk): one piece per workgroup if they were dealt evenly,
// so that nobody sweeps a second whole chunk while the others are done; not below 256 tiles, a piece costs a claim.
YB_HD uint32_t yb_piece_tiles(uint32_t rest, uint32_t blocks, uint32_t chunk) {
    if (blocks == 0u) blocks = 1u;
    unsigned long long p = ((unsigned long long)rest + blocks - 1u) / blocks;
    p = (p + 63ull) / 64ull * 64ull;
    if (p < 256ull) p = 256ull;
    if (p > (unsigned long long)chunk) p = chunk;
    return (uint32_t)p;
}
YB_HD uint32_t yb_piece_count(uint32_t rest, uint32_t piece) { return piece ? (uint32_t)(((unsigned long long)rest + piece - 1u) / piece) : 0u; }
