// CPU model of the masking pass: the rule of yet-another-bpe_amd/csrc/mask_logic.h (the functions k_mask calls), run sequentially in
// the kernel's shape -- blocks of `block` ids, the documents of a block's first and last id found in the whole table and every
// id's document searched between those two, the four counters summed per wave of 64 ids, then per block, then added to the
// call's.  Test infrastructure only.  With -DMASK_MODEL_MAIN: a stand-alone program that runs the model on document lengths
// that take every path and compares it with a direct walk over the documents (the program a sanitizer build runs).
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/mask_logic.h"

// ids[n_ids], doc_off[n_docs] (NULL with n_docs <= 1: one document), words[n_ids] or NULL -> out_ids, out_labels, counters[4]
// (protected, masked, random, kept).  Returns 0; -1 for arguments yabpe_mask refuses; -2 if a search left its document.
extern "C" int mask_model_run(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *words, uint64_t seed,
                              uint64_t first_doc, uint64_t select, uint64_t mask, uint64_t random, uint32_t mask_id, uint32_t n_random,
                              uint32_t ignore, uint32_t flags, uint32_t block, uint32_t *out_ids, uint32_t *out_labels, uint64_t *counters) {
    const MaskRule R{select, mask, random, mask_id, n_random};
    const bool whole_word = (flags & 1u) != 0;
    if (!mask_rule_valid(R) || (flags & ~1u) || (whole_word && !words) || (!doc_off && n_docs > 1) || block == 0 || block % 64) return -1;
    std::vector<unsigned long long> docs(1, 0);
    if (doc_off) docs.assign(doc_off, doc_off + n_docs);
    if (docs.empty() || docs[0] != 0) return -1;
    for (size_t d = 1; d < docs.size(); ++d)
        if (docs[d] < docs[d - 1] || docs[d] > n_ids) return -1;
    const uint32_t nd = (uint32_t)docs.size();
    for (uint32_t k = 0; k < MASK_KINDS; ++k) counters[k] = 0;
    for (unsigned long long i0 = 0; i0 < n_ids; i0 += block) {  // a workgroup
        const unsigned long long il = i0 + block - 1 < n_ids ? i0 + block - 1 : n_ids - 1;
        const uint32_t d_lo = mask_doc_of(docs.data(), i0, 0, nd - 1), d_hi = mask_doc_of(docs.data(), il, 0, nd - 1);
        unsigned long long blk[MASK_KINDS] = {0, 0, 0, 0};
        for (unsigned long long w0 = i0; w0 < i0 + block; w0 += 64) {  // a wave (whole waves run: lanes past the end count nothing)
            uint32_t wave[MASK_KINDS] = {0, 0, 0, 0};
            for (unsigned long long i = w0; i < w0 + 64 && i < n_ids; ++i) {
                const uint32_t d = mask_doc_of(docs.data(), i, d_lo, d_hi);
                if (docs[d] > i || (d + 1 < nd ? docs[d + 1] : n_ids) <= i) return -2;
                const uint32_t kind = mask_token(seed, first_doc, d, i - docs[d], words ? words[i] : 0u, whole_word, R, ignore, ids[i], &out_ids[i],
                                                 &out_labels[i]);
                if (kind < MASK_KINDS) ++wave[kind];
            }
            for (uint32_t k = 0; k < MASK_KINDS; ++k) blk[k] += wave[k];
        }
        for (uint32_t k = 0; k < MASK_KINDS; ++k) counters[k] += blk[k];
    }
    return 0;
}

#ifdef MASK_MODEL_MAIN
#include <cstdio>

namespace {
// the same result document by document, no blocks and no searches
bool agrees(const std::vector<uint32_t> &lens, bool with_doc_off, bool with_words, uint32_t flags, uint64_t seed) {
    std::vector<uint64_t> off;
    uint64_t n = 0;
    for (uint32_t l : lens) {
        off.push_back(n);
        n += l;
    }
    std::vector<uint32_t> ids(n + 1), words(n + 1), got_ids(n + 1), got_lab(n + 1);
    for (uint64_t i = 0; i < n; ++i) {
        ids[i] = (uint32_t)(enc_mix(i + seed) % 1000);
        words[i] = (uint32_t)(i / 3) | (enc_mix(i ^ 0x55) % 16 == 0 ? MASK_WORD_SPECIAL : 0u);
    }
    uint64_t cnt[MASK_KINDS];
    const uint64_t Ts = (1ull << 32) / 2, Tm = (1ull << 32) / 10 * 8, Tr = (1ull << 32) / 10;
    const int rc = mask_model_run(ids.data(), n, with_doc_off ? off.data() : nullptr, (uint32_t)lens.size(), with_words ? words.data() : nullptr, seed,
                                  1ull << 40, Ts, Tm, Tr, 5000, 777, 0xFFFFFF9Cu, flags, MASK_BLOCK, got_ids.data(), got_lab.data(), cnt);
    if (rc != 0) return false;
    const MaskRule R{Ts, Tm, Tr, 5000, 777};
    uint64_t exp_cnt[MASK_KINDS] = {0, 0, 0, 0};
    uint64_t i = 0;
    for (size_t d = 0; d < lens.size(); ++d)
        for (uint32_t j = 0; j < lens[d]; ++j, ++i) {
            uint32_t nid, lab;
            const uint32_t kind = mask_token(seed, 1ull << 40, (uint32_t)d, j, with_words ? words[i] : 0u, (flags & 1u) != 0, R, 0xFFFFFF9Cu, ids[i], &nid, &lab);
            if (kind < MASK_KINDS) ++exp_cnt[kind];
            if (nid != got_ids[i] || lab != got_lab[i]) return false;
        }
    for (uint32_t k = 0; k < MASK_KINDS; ++k)
        if (cnt[k] != exp_cnt[k]) return false;
    return true;
}
}  // namespace

int main() {
    const std::vector<std::vector<uint32_t>> sets = {
        {0, 0, 5, 0, 0, 7, 300, 0, 3, 0, 0}, std::vector<uint32_t>(600, 1), {3, 3, 700, 3, 3}, {0, 0, 0}, {0}, {256, 256, 1}, {1000}};
    int bad = 0, runs = 0;
    for (const auto &lens : sets)
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (int with_words = (int)flags; with_words < 2; ++with_words) {
                bad += !agrees(lens, true, with_words != 0, flags, 7 + runs);
                ++runs;
            }
    for (uint32_t n : {0u, 77u, 515u}) {  // n_docs = 1 with doc_off = NULL
        bad += !agrees({n}, false, true, 1, 3);
        ++runs;
    }
    printf("mask_model: %d runs, %d differ\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
