// load_logic.h -- placement arithmetic of the tile-centric loader (k_load_tiles in yabpe_kernels.h).
// Shared by the kernel and by the CPU model (tests/hostmodel/load_model.cpp).
//
// Word w of n_words has the bytes [off[w], off[w+1]) and the packed start pos(w) = off[w] - off_base + w: every earlier
// word contributed its bytes + 1 SEP.  pos is strictly increasing in w.  Tile t holds exactly the words whose packed
// start lies in [t * span, (t + 1) * span), each at slot pos(w) - t * span; a word that the stream does not keep (fewer
// than 2 bytes in the flat layout, or too long for a tile) still occupies its packed positions.
//
// A wave owns a run of consecutive tiles.  It finds the first word of the run with one K-ary search (K probes per step,
// one per lane) and walks forward from there: the first word of tile t + 1 is where tile t's walk ended.
#pragma once
#include <stdint.h>

#include "tile_logic.h"

#define YB_LOAD_RUN 16   /* consecutive tiles one wave loads */
#define YB_LOAD_STAGE 16 /* the byte window of a tile is fetched in aligned pieces of this many bytes */

YB_HD unsigned long long yb_load_pos(unsigned long long off_w, unsigned long long off_base, unsigned long long w) {
    return (off_w - off_base) + w;
}

// ---- K-ary search for the first word w in [lo, hi] with pos(w) >= target (hi: the answer if no word of [lo, hi) is).
// One step probes the words lo + k * stride, k < K, that lie below hi; `first` is the smallest k whose probe is >= target
// (K if none is, probes that were not made count as "none").  The step narrows [lo, hi]; the search is over when lo == hi.
YB_HD unsigned long long yb_kary_stride(unsigned long long lo, unsigned long long hi, uint32_t K) {
    const unsigned long long n = hi - lo;
    return n <= K ? 1ull : (n + K - 1ull) / K;
}
YB_HD void yb_kary_narrow(unsigned long long &lo, unsigned long long &hi, uint32_t K, uint32_t first) {
    const unsigned long long stride = yb_kary_stride(lo, hi, K);
    const unsigned long long n = hi - lo;
    const unsigned long long probes = (n + stride - 1ull) / stride;  // <= K
    if (first == 0u) {
        hi = lo;
    } else if ((unsigned long long)first >= probes) {  // every probe is below the target: the answer lies behind the last one
        lo = lo + (probes - 1ull) * stride + 1ull;
    } else {
        const unsigned long long h = lo + (unsigned long long)first * stride;
        lo = lo + ((unsigned long long)first - 1ull) * stride + 1ull;
        hi = h;
    }
}

// ---- what the loader does with one word
enum { YB_LOAD_SKIP = 0, YB_LOAD_COPY = 1, YB_LOAD_LONG = 2 };
struct YbLoadWord {
    int kind;          // SKIP: nothing stored; COPY: L tokens + SEP at `slot`; LONG: goes on the long-word list
    uint32_t slot;     // position in its tile
    uint32_t len_end;  // what the word raises its tile's length to (0: nothing)
    bool sep_only;     // LONG in the weighted layout: a SEP placeholder at `slot` keeps the word indices aligned
};
YB_HD YbLoadWord yb_load_word(unsigned long long pos, unsigned long long tile_start, unsigned long long L, bool weighted, uint32_t lmax) {
    YbLoadWord r;
    r.slot = (uint32_t)(pos - tile_start);
    r.sep_only = false;
    if (!weighted && L <= 1ull) {  // flat layout: a word of < 2 tokens can never form a pair
        r.kind = YB_LOAD_SKIP;
        r.len_end = 0u;
    } else if (L + 1ull > (unsigned long long)lmax) {
        r.kind = YB_LOAD_LONG;
        r.sep_only = weighted;
        r.len_end = weighted ? r.slot + 1u : 0u;
    } else {
        r.kind = YB_LOAD_COPY;
        r.len_end = r.slot + (uint32_t)L + 1u;
    }
    return r;
}

// ---- the byte window of a tile whose first word starts at address a0: the words that start in the tile begin less than
// `span` bytes behind a0 (their packed starts differ by less than span), and a kept word has at most lmax - 1 bytes, so
// [a0, a0 + span + lmax - 1) holds every byte the tile needs.  It is fetched in aligned pieces from `base` = a0 rounded
// down; a piece that sticks out of the corpus [lo, hi) is fetched byte by byte, so nothing outside it is read.
YB_HD unsigned long long yb_load_window_base(unsigned long long a0) { return a0 & ~(unsigned long long)(YB_LOAD_STAGE - 1); }
YB_HD uint32_t yb_load_window_pieces(uint32_t span, uint32_t lmax) {
    return (span + lmax - 1u + (YB_LOAD_STAGE - 1u) + (YB_LOAD_STAGE - 1u)) / YB_LOAD_STAGE;
}

// ---- gathering retile (k_retile_gather in yabpe_aux_kernels.h).  The kept elements of the old stream are numbered in stream
// order; base[t] is the number of the first one of old tile t (an exclusive scan of the tiles' kept counts, n_tiles + 1
// entries).  An element goes to the new tile (number of its word's first element) / span, at slot (its own number) -
// tile * span.  A workgroup owns `group` consecutive new tiles, the words that start in [k_lo, k_lo + group * span): it
// finds the first old tile that holds an element numbered >= k_lo (the first t with base[t + 1] > k_lo, by the K-ary search
// above) and walks the old tiles forward until one starts at or behind the end of its range.
struct YbGatherDest {
    bool mine;      // the element's word starts in this workgroup's range
    uint32_t tile;  // new tile, relative to the group's first
    uint32_t slot;
};
YB_HD YbGatherDest yb_gather_dest(unsigned long long g, unsigned long long gws, unsigned long long k_lo, uint32_t group, uint32_t span) {
    YbGatherDest d;
    d.mine = gws >= k_lo && gws < k_lo + (unsigned long long)group * span;
    d.tile = d.mine ? (uint32_t)(gws - k_lo) / span : 0u;
    d.slot = d.mine ? (uint32_t)(g - k_lo) - d.tile * span : 0u;
    return d;
}
