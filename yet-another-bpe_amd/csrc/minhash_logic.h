// minhash_logic.h -- the near-duplicate rule (BBPETokenizer.minhash_tokens, yet_another_bpe/tokenizer.py), host- and
// device-callable: yabpe_minhash_kernels.h and the CPU model of tests/hostmodel/minhash_model.cpp call the same functions.
//
// With mix and rnd(seed, stream, i) of yet_another_bpe/synth.py (enc_mix / enc_rnd of encode_logic.h), G the golden-ratio
// constant of rnd, all arithmetic u64 with wraparound:
//   shingles   a document of L ids with ngram = n has L - n + 1 shingles, one per window of n consecutive ids (L >= n), one
//              shingle of all its L ids (0 < L < n), none (L = 0).
//   hash       of a shingle of m ids: s = rnd(0, 0x68, m); for every id in order s = mix(s + G * (id + 1)); h = s >> 32.
//   functions  a_k = rnd(seed, 0x70, k) | 1, b_k = rnd(seed, 0x71, k); p_k(h) = (a_k * h + b_k) >> 32 (multiply-shift).
//   signature  sig[d][k] = min over the shingles of d of p_k(h); 0xFFFFFFFF in every slot of a document without shingles.
//   band key   with r = num_perm / bands: key[d][t] = fold of s = rnd(0, 0x6b, t), then s = mix(s + G * (v + 1)) for the r
//              values v = sig[d][t * r .. t * r + r - 1] in order.  Two documents are candidates iff they share key[.][t] for a t.
#pragma once
#include <stdint.h>

#include "encode_logic.h"

constexpr unsigned long long MH_STREAM_SHINGLE = 0x68, MH_STREAM_A = 0x70, MH_STREAM_B = 0x71, MH_STREAM_BAND = 0x6b;
constexpr uint32_t MH_MAX_NGRAM = 32, MH_MAX_PERM = 1024;
constexpr uint32_t MH_EMPTY = 0xFFFFFFFFu;                  // every slot of a document without shingles
constexpr uint32_t MH_TILE = 1024;                          // shingle positions of one piece (one workgroup of k_minhash)
constexpr unsigned long long MH_MAX_SLOTS = 1ull << 36;     // n_docs * num_perm, and ids, one call addresses at most

struct MinhashRule {
    unsigned long long seed;
    uint32_t num_perm, ngram, bands;  // bands 0: no keys
};

// the rule's argument checks (yabpe_minhash and the model refuse the same things)
YB_HD bool mh_rule_valid(const MinhashRule &R) {
    return R.num_perm >= 1 && R.num_perm <= MH_MAX_PERM && R.ngram >= 1 && R.ngram <= MH_MAX_NGRAM &&
           (R.bands == 0 || (R.bands <= R.num_perm && R.num_perm % R.bands == 0));
}

YB_HD unsigned long long mh_shingles(unsigned long long L, uint32_t n) { return L >= n ? L - n + 1 : (L ? 1ull : 0ull); }
YB_HD uint32_t mh_shingle_ids(unsigned long long L, uint32_t n) { return L >= n ? n : (uint32_t)L; }  // m: the ids of one shingle
YB_HD unsigned long long mh_pieces(unsigned long long shingles) { return (shingles + MH_TILE - 1) / MH_TILE; }

// the shingle hash in two halves: the start for shingles of m ids, then one step per id
YB_HD unsigned long long mh_hash_init(uint32_t m) { return enc_rnd(0, MH_STREAM_SHINGLE, m); }
YB_HD unsigned long long mh_hash_step(unsigned long long s, uint32_t id) { return enc_mix(s + ENC_RND_G * ((unsigned long long)id + 1)); }
YB_HD uint32_t mh_hash_final(unsigned long long s) { return (uint32_t)(s >> 32); }

YB_HD unsigned long long mh_param_a(unsigned long long seed, uint32_t k) { return enc_rnd(seed, MH_STREAM_A, k) | 1ull; }
YB_HD unsigned long long mh_param_b(unsigned long long seed, uint32_t k) { return enc_rnd(seed, MH_STREAM_B, k); }
YB_HD uint32_t mh_perm(unsigned long long a, unsigned long long b, uint32_t h) { return (uint32_t)((a * h + b) >> 32); }

// key[d][band] from the r signature values of the band
YB_HD unsigned long long mh_band_key(const uint32_t *sig, uint32_t band, uint32_t r) {
    unsigned long long s = enc_rnd(0, MH_STREAM_BAND, band);
    for (uint32_t j = 0; j < r; ++j) s = mh_hash_step(s, sig[j]);
    return s;
}

// The document of piece p: the last d in [0, n_docs - 1] with piece_off[d] <= p (a document without pieces shares its start
// with its successor and is never the answer while a later one starts there too).
YB_HD uint32_t mh_doc_of(const unsigned long long *piece_off, unsigned long long p, uint32_t n_docs) {
    uint32_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (piece_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
