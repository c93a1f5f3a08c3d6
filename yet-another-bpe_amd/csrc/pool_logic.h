// pool_logic.h -- the rules of the persistent word pool (yabpe_pool_add), shared by the HIP kernels
// (yabpe_pool_kernels.h) and by the CPU unit-test model (tests/hostmodel/pool_model.cpp).
//
//   state     pool word p = arena[off[p], off[p + 1]) with count[p] (u64) and hash[p] (the MASKED hash of its bytes); an
//             open-addressing array of u32 pool indices (PL_EMPTY: free), a power of two in size, at most half full.
//   hash      k_word_hash's 64-bit hash of the bytes (pl_word_hash below is the same function for the host model), cut to
//             its low `bits` bits (option "pool_hash_bits"): placement and the hash pre-check both use the cut value, so a
//             test can force collisions (bits = 4) or one single probe chain (bits = 0).
//   probing   linear from pl_home; a slot matches when hash, length and then bytes are equal (pl_match); the first free
//             slot ends the chain -- nothing is ever removed.
//   growth    capacities double until they hold what is asked (pl_grow); the slots grow when the words would fill more
//             than half of them (pl_slots_full).  The per-word arrays hold as many words as half the slots.
#pragma once
#include <stdint.h>

#include "tile_logic.h" // YB_HD

constexpr uint32_t PL_EMPTY = 0xFFFFFFFFu;                      // free slot; also "not in the pool" as a probe's result
constexpr unsigned long long PL_MAX_WORDS = 0xFFFFFFFEull;      // unique words a pool holds, and words one call brings, at most
constexpr unsigned long long PL_MAX_WORD_BYTES = 0xFFFFFFFFull; // bytes of one word at most
constexpr uint32_t PL_WAVE_BYTES = 64;                          // longer words are compared and copied by a whole wave

// what a probe says about a call-unique word
constexpr uint32_t PL_NEW = 0xFFFFFFFFu;   // not in the pool: to be appended
constexpr uint32_t PL_DROP = 0xFFFFFFFEu;  // zero length: dropped (reference trainer.py:170, 211)

YB_HD unsigned long long pl_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// (k_word_hash of yabpe_aux_kernels.h, which the call-local pooling computes for every word)
YB_HD unsigned long long pl_word_hash(const uint8_t *p, unsigned long long L) {
    unsigned long long h = 0xcbf29ce484222325ull ^ L;
    for (unsigned long long i = 0; i < L; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return pl_mix(h);
}

YB_HD unsigned long long pl_mask_hash(unsigned long long h, uint32_t bits) {
    return bits >= 64 ? h : bits == 0 ? 0ull : h & ((1ull << bits) - 1ull);
}
YB_HD unsigned long long pl_home(unsigned long long masked_hash, unsigned long long cap) { return masked_hash & (cap - 1ull); }
YB_HD unsigned long long pl_next(unsigned long long slot, unsigned long long cap) { return (slot + 1ull) & (cap - 1ull); }

// the cheap part of the match: stored masked hash and length against the word's
YB_HD bool pl_match_head(unsigned long long s_hash, unsigned long long s_len, unsigned long long w_hash, unsigned long long w_len) {
    return s_hash == w_hash && s_len == w_len;
}
YB_HD bool pl_match(unsigned long long s_hash, unsigned long long s_len, const uint8_t *s_bytes, unsigned long long w_hash,
                    unsigned long long w_len, const uint8_t *w_bytes) {
    if (!pl_match_head(s_hash, s_len, w_hash, w_len)) return false;
    for (unsigned long long i = 0; i < w_len; ++i)
        if (s_bytes[i] != w_bytes[i]) return false;
    return true;
}

// capacities: the smallest cap * 2^k >= need (cap >= 1)
YB_HD unsigned long long pl_grow(unsigned long long cap, unsigned long long need) {
    while (cap < need) cap <<= 1;
    return cap;
}
YB_HD unsigned long long pl_pow2(unsigned long long v) { return pl_grow(2ull, v); } // a slot count from an option: >= 2, a power of two
YB_HD bool pl_slots_full(unsigned long long n_words, unsigned long long slot_cap) { return n_words * 2ull > slot_cap; }
YB_HD unsigned long long pl_slots_for(unsigned long long slot_cap, unsigned long long n_words) { return pl_grow(slot_cap, n_words * 2ull); }
YB_HD unsigned long long pl_words_for(unsigned long long slot_cap) { return slot_cap / 2ull; } // entries of count / hash (off: one more)
