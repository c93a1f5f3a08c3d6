// tile_logic.h -- per-position rules of the merge-apply pass, shared by the HIP kernels
// (yabpe_kernels.hip) and by the CPU unit-test model (tests/hostmodel/tile_model.cpp).
//
// Token stream format (DESIGN.md "Data layout"): u16 ids; every word is followed by SEP; PAD fills
// tile lead/tail regions.  Ids are < PAD, so SEP/PAD never match a pair.
//
// The rules implement trainer.py:276-285 (greedy left-to-right, non-overlapping replacement) and the net
// effect of the incremental recount trainer.py:264-273 + :290-294 on the pair table, expressed per merge
// site so that all sites can be processed in parallel:
//   site p (tok[p]==a, tok[p+1]==b, selected by the greedy rule) rewrites (a,b) -> c and changes the
//   pair to its left and the pair to its right.  Where two sites touch (…a b a b…), the pair between
//   them is accounted for by the RIGHT site only, so nothing is counted twice.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YB_HD __host__ __device__ __forceinline__
#else
#define YB_HD inline
#endif

#define YB_SEP 0xFFFFu
#define YB_PAD 0xFFFEu
#define YB_MAX_TOKENS 0xFFFEu /* ids 0 .. 0xFFFD */

// key of the pair table: (left << 16) | right
YB_HD uint32_t yb_pairkey(uint32_t left, uint32_t right) { return (left << 16) | right; }
// the same pair as it appears in memory (little endian: first element in the low half)
YB_HD uint32_t yb_memkey(uint32_t left, uint32_t right) { return (right << 16) | left; }

// Width traits: the sentinels and the pair key of one id width.  ONE copy of the rules below serves both; YbW16 means what
// the YB_* macros above mean, YbW32 is the u32-id merge loop: ids 0 .. 2^24 - 3, a 48-bit pair key in a u64.
struct YbW16 {
    typedef uint32_t key_t;
    static constexpr uint32_t SEP = YB_SEP, PAD = YB_PAD, MAX_TOKENS = YB_MAX_TOKENS;
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu; // (left, right) = (SEP, SEP): no pair of ids
    static YB_HD key_t key(uint32_t left, uint32_t right) { return (left << 16) | right; }
    static YB_HD uint32_t left(key_t k) { return k >> 16; }
    static YB_HD uint32_t right(key_t k) { return k & 0xFFFFu; }
};
struct YbW32 {
    typedef unsigned long long key_t;
    static constexpr uint32_t SEP = 0xFFFFFFFFu, PAD = 0xFFFFFFFEu;
    static constexpr uint32_t MAX_TOKENS = 0xFFFFFEu; /* ids 0 .. 2^24 - 3: the decode table's bound */
    static constexpr unsigned long long EMPTY = ~0ull; // above every 48-bit key
    static YB_HD key_t key(uint32_t left, uint32_t right) { return ((unsigned long long)left << 24) | right; }
    static YB_HD uint32_t left(key_t k) { return (uint32_t)(k >> 24); }
    static YB_HD uint32_t right(key_t k) { return (uint32_t)(k & 0xFFFFFFull); }
};

// index hash of a 48-bit pair key: the u32 pair table, its LDS aggregator and the u32 replay table (replay_logic.h)
YB_HD uint32_t yb_hash48(unsigned long long k) {
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 32;
    return (uint32_t)k;
}

template <class W>
struct YbDeltasT {
    // fixed slots (no runtime-indexed arrays, so the device keeps them in registers):
    //   left:  lo -1, ln +1     right: ro -1, rn +1
    typename W::key_t lo, ln, ro, rn;
    bool left, right;
};
typedef YbDeltasT<YbW16> YbDeltas;

// Neighbour deltas of merge site p (the site's own (a,b) -1 is accounted separately).
//   T(q): token at position q of the tile (PAD outside), M(q): 1 if q is a merge site (0 outside).
template <class W, class TokF, class MrgF>
YB_HD void yb_site_deltas_w(int p, uint32_t a, uint32_t b, uint32_t c, TokF T, MrgF M, YbDeltasT<W> &d) {
    const uint32_t L = T(p - 1);
    d.left = L < W::PAD;
    if (M(p - 2)) { // left neighbour is the b of the site at p-2: old pair (b,a), new pair (c,c)
        d.lo = W::key(b, a);
        d.ln = W::key(c, c);
    } else {
        d.lo = W::key(L, a);
        d.ln = W::key(L, c);
    }
    const uint32_t R = T(p + 2);
    d.right = R < W::PAD && !M(p + 2); // if p+2 is a site, that site's left side covers this boundary
    d.ro = W::key(b, R);
    d.rn = W::key(c, R);
}
template <class TokF, class MrgF>
YB_HD void yb_site_deltas(int p, uint32_t a, uint32_t b, uint32_t c, TokF T, MrgF M, YbDeltas &d) {
    yb_site_deltas_w<YbW16>(p, a, b, c, T, M, d);
}

// What position p of the old tile contributes to the rewritten tile.
// Returns 1 and sets `out` when the element is kept.
// drop_dead (flat layout only): words that are reduced to a single token can never produce a pair again
// (trainer.py:231 iterates range(len(word)-1)), so the token and its SEP are removed from the stream; empty
// words (SEP after SEP/PAD/tile start) likewise.
template <class W, class TokF, class MrgF>
YB_HD int yb_keep_w(int p, uint32_t c, bool drop_dead, TokF T, MrgF M, uint32_t &out) {
    uint32_t v = T(p);
    if (v == W::PAD) return 0;
    if (M(p - 1)) return 0; // consumed as the b of the site at p-1
    if (v < W::PAD) {
        out = M(p) ? c : v;
        if (!drop_dead) return 1;
        bool prev_boundary = M(p - 2) ? false : (T(p - 1) >= W::PAD);
        int nx = M(p) ? p + 2 : p + 1;
        bool next_sep = !M(nx) && T(nx) == W::SEP;
        return !(prev_boundary && next_sep);
    }
    // v == SEP
    out = W::SEP;
    if (!drop_dead) return 1;
    if (M(p - 2)) { // word ends with the c written at p-2
        bool pb = M(p - 4) ? false : (T(p - 3) >= W::PAD);
        return !pb;
    }
    uint32_t u = T(p - 1);
    if (u >= W::PAD) return 0; // empty word
    bool pb = M(p - 3) ? false : (T(p - 2) >= W::PAD);
    return !pb;
}
template <class TokF, class MrgF>
YB_HD int yb_keep(int p, uint32_t c, bool drop_dead, TokF T, MrgF M, uint32_t &out) {
    return yb_keep_w<YbW16>(p, c, drop_dead, T, M, out);
}

// Greedy left-to-right site rule (trainer.py:276-285) for one position: p is a site iff (T(p), T(p+1)) == (a, b) and, for
// a == b, p lies an even distance from the start of its maximal run of a (run_start: first position of that run).
YB_HD bool yb_is_site(uint32_t x, uint32_t y, uint32_t a, uint32_t b, int p, int run_start) {
    return x == a && y == b && (a != b || ((p - run_start) & 1) == 0);
}

// Site-driven form of the same rewrite, used by k_apply (work proportional to the number of sites):
// the only elements that leave a tile are the b of every site, PAD, and -- in the flat layout -- the two
// remaining slots (c, SEP) of a word that was exactly (a b): it is now a single token and can never produce
// a pair again.  This equals yb_keep() on a stream that holds no single-token / empty words, which the flat
// loader guarantees (it never emits them) and this rule preserves.
template <class W, class TokF>
YB_HD bool yb_site_word_dies_w(int p, TokF T) {
    return T(p - 1) >= W::PAD && T(p + 2) == W::SEP;
}
template <class TokF>
YB_HD bool yb_site_word_dies(int p, TokF T) {
    return yb_site_word_dies_w<YbW16>(p, T);
}
