// CPU model of the MinHash passes: the rule of yet-another-bpe_amd/csrc/minhash_logic.h (the functions the kernels of
// yabpe_minhash_kernels.h call), run sequentially in the kernels' shape -- shingle and piece counts per document, their
// exclusive scan, rows preset unless the document is exactly one piece, then piece by piece: the document found by search in
// the scanned starts, the ids staged with their halo, the hashes padded to a multiple of four with position 0's, four waves
// taking every fourth quad for passes of 128 functions, the waves' minima combined, stored (one piece) or min-ed into the
// row (several) -- and the band keys once every row is complete.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/minhash_logic.h"

// ids[n_ids], doc_off[n_docs] starts -> sig[n_docs * num_perm], n_shingles[n_docs], keys[n_docs * bands] (bands > 0).
// Returns the number of pieces; -1 for arguments yabpe_minhash refuses; -2 if a search or a staging step left its document.
extern "C" long long minhash_model_run(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint64_t seed, uint32_t num_perm,
                                       uint32_t ngram, uint32_t bands, uint32_t *sig, uint64_t *n_shingles, uint64_t *keys) {
    constexpr uint32_t waves = 4, chunk = 128;  // MH_WAVES, MH_CHUNK of yabpe_minhash_kernels.h
    const MinhashRule R{seed, num_perm, ngram, bands};
    if (!mh_rule_valid(R) || !doc_off || !n_docs || doc_off[0] != 0) return -1;
    for (uint32_t d = 1; d < n_docs; ++d)
        if (doc_off[d] < doc_off[d - 1] || doc_off[d] > n_ids) return -1;
    auto doc_len = [&](uint32_t d) { return (d + 1 < n_docs ? doc_off[d + 1] : n_ids) - doc_off[d]; };
    std::vector<unsigned long long> piece_off(n_docs + 1, 0);
    for (uint32_t d = 0; d < n_docs; ++d) {  // k_minhash_plan, the scan, k_minhash_fill
        n_shingles[d] = mh_shingles(doc_len(d), ngram);
        const unsigned long long np = mh_pieces(n_shingles[d]);
        piece_off[d + 1] = piece_off[d] + np;
        if (np != 1) std::fill(sig + (size_t)d * num_perm, sig + (size_t)(d + 1) * num_perm, MH_EMPTY);
    }
    std::vector<uint32_t> s_ids(MH_TILE + MH_MAX_NGRAM - 1), s_h(MH_TILE), s_min((size_t)waves * chunk);
    for (unsigned long long p = 0; p < piece_off[n_docs]; ++p) {  // a workgroup of k_minhash
        const uint32_t d = mh_doc_of(piece_off.data(), p, n_docs);
        if (piece_off[d] > p || piece_off[d + 1] <= p) return -2;
        const unsigned long long L = doc_len(d), S = mh_shingles(L, ngram), s0 = (p - piece_off[d]) * MH_TILE;
        const uint32_t m = mh_shingle_ids(L, ngram), cnt = S - s0 < MH_TILE ? (uint32_t)(S - s0) : MH_TILE;
        if (s0 >= S || s0 + cnt + m - 1 > L) return -2;
        for (uint32_t i = 0; i < cnt + m - 1; ++i) s_ids[i] = ids[doc_off[d] + s0 + i];
        const uint32_t padded = (cnt + 3u) & ~3u;
        for (uint32_t i = 0; i < padded; ++i) {
            const uint32_t pos = i < cnt ? i : 0u;
            unsigned long long s = mh_hash_init(m);
            for (uint32_t j = 0; j < m; ++j) s = mh_hash_step(s, s_ids[pos + j]);
            s_h[i] = mh_hash_final(s);
        }
        for (uint32_t k0 = 0; k0 < num_perm; k0 += chunk) {  // a pass
            for (uint32_t w = 0; w < waves; ++w)
                for (uint32_t t = 0; t < chunk; ++t) {  // a lane's function
                    const uint32_t k = k0 + t;
                    const unsigned long long a = k < num_perm ? mh_param_a(seed, k) : 0ull, b = k < num_perm ? mh_param_b(seed, k) : ~0ull;
                    uint32_t mn = MH_EMPTY;
                    for (uint32_t q = w; q < padded / 4; q += waves)
                        for (uint32_t e = 0; e < 4; ++e) mn = std::min(mn, mh_perm(a, b, s_h[4 * q + e]));
                    s_min[(size_t)w * chunk + t] = mn;
                }
            for (uint32_t t = 0; t < chunk && k0 + t < num_perm; ++t) {
                uint32_t v = s_min[t];
                for (uint32_t w = 1; w < waves; ++w) v = std::min(v, s_min[(size_t)w * chunk + t]);
                uint32_t &slot = sig[(size_t)d * num_perm + k0 + t];
                slot = S <= MH_TILE ? v : std::min(slot, v);
            }
        }
    }
    const uint32_t r = bands ? num_perm / bands : 0;
    for (uint64_t i = 0; i < (uint64_t)n_docs * bands; ++i)  // k_minhash_keys
        keys[i] = mh_band_key(sig + (i / bands) * num_perm + (i % bands) * r, (uint32_t)(i % bands), r);
    return (long long)piece_off[n_docs];
}
