// CPU model of the resumed load's segmentation: the id-pair table and the word walks of
// yet-another-bpe_amd/csrc/replay_logic.h (the functions the HIP kernels call), run over a batch of words.
// Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/replay_logic.h"

// Words w = bytes[off[w], off[w + 1]).  form 0: the sequential (heap) walk for every word; form 1: the lane form for words
// of at most RP_SHORT bytes, the sequential walk for the others (what the kernel does).  Tokens of word w are written to
// out_tok[off[w] - off[0] ...], their number to out_cnt[w].  Returns 0.
extern "C" int replay_model(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges, const uint8_t *bytes,
                            const uint64_t *off, uint64_t n_words, int form, uint16_t *out_tok, uint32_t *out_cnt) {
    RpTableHost m;
    rp_build_table(left, right, merged, n_merges, &m);
    const RpTable t = m.table();
    std::vector<uint32_t> tok, nxt, prv;
    std::vector<unsigned long long> heap;
    for (uint64_t w = 0; w < n_words; ++w) {
        const uint64_t s = off[w];
        const uint32_t L = (uint32_t)(off[w + 1] - s);
        uint16_t *dst = out_tok + (s - off[0]);
        if (form == 1 && L <= RP_SHORT) {
            out_cnt[w] = rp_walk_lanes(bytes + s, L, t, dst);
            continue;
        }
        tok.resize(L + 1);
        nxt.resize(L + 1);
        prv.resize(L + 1);
        heap.resize(3 * (size_t)L + 1);
        const uint32_t cnt = rp_walk_heap(bytes + s, L, t, tok.data(), nxt.data(), prv.data(), heap.data());
        for (uint32_t k = 0; k < cnt; ++k) dst[k] = (uint16_t)tok[k];
        out_cnt[w] = cnt;
    }
    return 0;
}

// One lookup: the smallest rank >= tmin of (a, b).  Returns 1 and the rank / merged id, or 0.
extern "C" int replay_model_lookup(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges, uint32_t a, uint32_t b,
                                   uint32_t tmin, uint32_t *rank, uint32_t *res) {
    RpTableHost m;
    rp_build_table(left, right, merged, n_merges, &m);
    return rp_lookup(m.table(), a, b, tmin, rank, res) ? 1 : 0;
}

// The table at 64-bit keys (the u32 resumed load's): built by the same rp_build_table, read by rp32_lookup.  n_q lookups of
// one table: found[q] = 1 with rank[q] / res[q], or 0.  displaced: keys of the index that do not sit at their hash's slot;
// wrapped: those of them whose probe sequence went past the end of the index.  Returns 0.
extern "C" int replay_model_lookup32(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges, const uint32_t *a,
                                     const uint32_t *b, const uint32_t *tmin, uint32_t n_q, uint8_t *found, uint32_t *rank, uint32_t *res,
                                     uint32_t *displaced, uint32_t *wrapped) {
    Rp32TableHost m;
    rp_build_table(left, right, merged, n_merges, &m);
    const Rp32Table t{m.table(), m.n_merges()};
    for (uint32_t q = 0; q < n_q; ++q) found[q] = rp32_lookup(t, a[q], b[q], tmin[q], &rank[q], &res[q]) ? 1 : 0;
    *displaced = *wrapped = 0;
    for (uint32_t s = 0; s <= t.mask; ++s) {
        if (m.idx_key[s] == YbW32::EMPTY) continue;
        const uint32_t home = yb_hash48(m.idx_key[s]) & t.mask;
        *displaced += home != s;
        *wrapped += home > s;
    }
    return 0;
}
