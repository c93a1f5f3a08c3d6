// CPU model of the span-corruption passes: the rule of yet-another-bpe_amd/csrc/span_logic.h (the functions the kernels of
// yabpe_span_kernels.h call), run sequentially in the kernels' shape -- blocks of `block` ids, the documents of a block's first
// and last id found in the whole table and every id's document searched between those two; the flags pass with the
// predecessor's answer taken from the block (the block's first id computes it); exclusive scans; the place pass; the offsets;
// the write pass.  Test infrastructure only.  With -DSPAN_MODEL_MAIN: a stand-alone program that runs the model on document
// lengths that take every path and compares it with a direct walk over the documents (the program a sanitizer build runs).
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/span_logic.h"

namespace {
void scan(const std::vector<uint8_t> &in, std::vector<unsigned long long> &out) {
    out.assign(in.size() + 1, 0);
    for (size_t i = 0; i < in.size(); ++i) out[i + 1] = out[i] + in[i];
}
}  // namespace

// ids[n_ids], doc_off[n_docs] (NULL with n_docs <= 1: one document), words[n_ids] or NULL, len[max_len - 1], sentinels[n_sentinels]
// -> out_in (room for n_ids), out_in_off[n_docs + 1], out_tgt (room for 2 n_ids + n_docs), out_tgt_off[n_docs + 1], counters[5]
// (protected, noise, cut, runs over the cap, runs).  Returns 0; -1 for arguments yabpe_span_corrupt refuses; -2 if a search left
// its document; -3 if a store would leave its array.
extern "C" int span_model_run(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *words, uint64_t seed,
                              uint64_t first_doc, uint64_t open, const uint64_t *len, uint32_t max_len, const uint32_t *sentinels, uint32_t n_sentinels,
                              uint64_t max_doc_ids, uint32_t flags, uint32_t block, uint32_t *out_in, uint64_t *out_in_off, uint32_t *out_tgt,
                              uint64_t *out_tgt_off, uint64_t *counters) {
    unsigned long long h_len[SPAN_MAX_LEN] = {0};
    if (max_len >= 1 && max_len <= SPAN_MAX_LEN)
        for (uint32_t k = 0; k + 1 < max_len; ++k) h_len[k] = len[k];
    if (!span_rule_valid(open, h_len, max_len)) return -1;
    const bool whole_word = (flags & 1u) != 0, final_sentinel = (flags & 2u) != 0;
    if ((flags & ~3u) || n_sentinels < (final_sentinel ? 2u : 1u) || !sentinels || (whole_word && !words) || (!doc_off && n_docs > 1) || block == 0 ||
        block % 64)
        return -1;
    std::vector<unsigned long long> docs(1, 0);
    if (doc_off) docs.assign(doc_off, doc_off + n_docs);
    if (docs.empty() || docs[0] != 0) return -1;
    for (size_t d = 1; d < docs.size(); ++d)
        if (docs[d] < docs[d - 1] || docs[d] > n_ids) return -1;
    const uint32_t nd = (uint32_t)docs.size();
    const SpanRule R{open, h_len, max_len};
    const unsigned long long K = n_sentinels - (final_sentinel ? 1u : 0u);
    for (int k = 0; k < 5; ++k) counters[k] = 0;
    std::vector<uint8_t> f(n_ids), start(n_ids), c_in(n_ids), c_tgt(n_ids), s_noise(block);
    std::vector<unsigned long long> run, in_pos, tgt_pos;
    auto doc_end = [&](uint32_t d) { return d + 1 < nd ? docs[d + 1] : (unsigned long long)n_ids; };
    auto block_docs = [&](unsigned long long i0, uint32_t *lo, uint32_t *hi) {
        const unsigned long long il = i0 + block - 1 < n_ids ? i0 + block - 1 : n_ids - 1;
        *lo = mask_doc_of(docs.data(), i0, 0, nd - 1);
        *hi = mask_doc_of(docs.data(), il, 0, nd - 1);
    };
    // ---- flags
    for (unsigned long long i0 = 0; i0 < n_ids; i0 += block) {
        uint32_t d_lo, d_hi;
        block_docs(i0, &d_lo, &d_hi);
        for (unsigned long long i = i0; i < i0 + block && i < n_ids; ++i) {  // every thread's own answer, then the barrier
            const uint32_t d = mask_doc_of(docs.data(), i, d_lo, d_hi);
            if (docs[d] > i || doc_end(d) <= i) return -2;
            s_noise[i - i0] = span_token_noise(span_doc_key(seed, first_doc, d), i - docs[d], words ? words[i] : 0u, whole_word, R);
        }
        for (unsigned long long i = i0; i < i0 + block && i < n_ids; ++i) {
            const uint32_t d = mask_doc_of(docs.data(), i, d_lo, d_hi), w = words ? words[i] : 0u;
            const unsigned long long j = i - docs[d], kd = span_doc_key(seed, first_doc, d);
            const bool kept = span_kept(j, max_doc_ids), noise = s_noise[i - i0] != 0;
            bool prev = false;
            if (j > 0 && kept && noise) prev = i > i0 ? s_noise[i - 1 - i0] != 0 : span_token_noise(kd, j - 1, words ? words[i - 1] : 0u, whole_word, R);
            f[i] = span_flags(kept, noise, j, prev);
            start[i] = (f[i] & SPAN_F_START) ? 1 : 0;
            counters[0] += (w & MASK_WORD_SPECIAL) ? 1 : 0;
            counters[1] += kept && noise;
            counters[2] += !kept;
        }
    }
    // ---- run numbers, the cap, slots
    scan(start, run);
    for (unsigned long long i0 = 0; i0 < n_ids; i0 += block) {
        uint32_t d_lo, d_hi;
        block_docs(i0, &d_lo, &d_hi);
        for (unsigned long long i = i0; i < i0 + block && i < n_ids; ++i) {
            const uint32_t d = mask_doc_of(docs.data(), i, d_lo, d_hi);
            const unsigned long long first = docs[d], j = i - first;
            unsigned long long k = 0;
            if (f[i] & SPAN_F_NOISE) k = run[i] + ((f[i] & SPAN_F_START) ? 1 : 0) - 1 - run[first];
            const bool is_last = final_sentinel && (i + 1 == doc_end(d) || (max_doc_ids && j + 1 == max_doc_ids));
            bool over;
            f[i] = span_place(f[i], k, K, is_last, &c_in[i], &c_tgt[i], &over);
            counters[3] += over;
        }
    }
    counters[4] = run[n_ids];
    // ---- positions, offsets
    scan(c_in, in_pos);
    scan(c_tgt, tgt_pos);
    for (uint32_t d = 0; d <= nd; ++d) {
        const unsigned long long p = d < nd ? docs[d] : (unsigned long long)n_ids;
        out_in_off[d] = in_pos[p];
        out_tgt_off[d] = tgt_pos[p];
    }
    if (in_pos[n_ids] > n_ids || tgt_pos[n_ids] > 2 * n_ids + nd) return -3;
    // ---- write
    for (unsigned long long i0 = 0; i0 < n_ids; i0 += block) {
        uint32_t d_lo, d_hi;
        block_docs(i0, &d_lo, &d_hi);
        for (unsigned long long i = i0; i < i0 + block && i < n_ids; ++i) {
            if (!(f[i] & SPAN_F_KEPT)) continue;
            unsigned long long k = 0, n_runs = 0;
            if (f[i] & (SPAN_F_START | SPAN_F_LAST)) {
                const unsigned long long base = run[docs[mask_doc_of(docs.data(), i, d_lo, d_hi)]];
                k = run[i] - base;
                n_runs = run[i + 1] - base;
            }
            if (in_pos[i] + c_in[i] > in_pos[n_ids] || tgt_pos[i] + c_tgt[i] > tgt_pos[n_ids]) return -3;
            if (((f[i] & SPAN_F_START) && k >= n_sentinels) || ((f[i] & SPAN_F_LAST) && (n_runs < K ? n_runs : K) >= n_sentinels)) return -3;
            span_write(f[i], ids[i], in_pos[i], tgt_pos[i], k, n_runs, K, sentinels, out_in, out_tgt);
        }
    }
    return 0;
}

#ifdef SPAN_MODEL_MAIN
#include <cstdio>

namespace {
// the same result document by document: noise by the rule's definition (opens and lengths per unit), no blocks, no scans
bool agrees(const std::vector<uint32_t> &lens, bool with_doc_off, bool with_words, uint32_t flags, uint64_t seed, uint32_t max_len, uint64_t open,
            uint32_t n_sent, uint64_t cut) {
    std::vector<uint64_t> off;
    uint64_t n = 0;
    for (uint32_t l : lens) {
        off.push_back(n);
        n += l;
    }
    const uint32_t nd = (uint32_t)lens.size();
    std::vector<uint32_t> ids(n + 1), words(n + 1), got_in(n + 1), got_tgt(2 * n + nd + 1), sent(n_sent);
    for (uint32_t k = 0; k < n_sent; ++k) sent[k] = 9000 + k;
    for (uint64_t i = 0; i < n; ++i) {
        ids[i] = (uint32_t)(enc_mix(i + seed) % 1000);
        words[i] = (uint32_t)(i / 3) | (enc_mix(i ^ 0x55) % 16 == 0 ? MASK_WORD_SPECIAL : 0u);
    }
    uint64_t len[SPAN_MAX_LEN] = {0};
    for (uint32_t k = 0; k + 1 < max_len; ++k) len[k] = (1ull << 32) / (k + 2);
    std::vector<uint64_t> in_off(nd + 1), tgt_off(nd + 1);
    uint64_t cnt[5];
    const int rc = span_model_run(ids.data(), n, with_doc_off ? off.data() : nullptr, nd, with_words ? words.data() : nullptr, seed, 1ull << 40, open, len,
                                  max_len, sent.data(), n_sent, cut, flags, SPAN_BLOCK, got_in.data(), in_off.data(), got_tgt.data(), tgt_off.data(), cnt);
    if (rc != 0) return false;
    const bool whole_word = flags & 1u, final_sentinel = (flags & 2u) != 0;
    const uint64_t K = n_sent - (final_sentinel ? 1 : 0);
    std::vector<uint32_t> exp_in, exp_tgt;
    uint64_t i = 0;
    for (uint32_t d = 0; d < nd; ++d) {
        if (in_off[d] != exp_in.size() || tgt_off[d] != exp_tgt.size()) return false;
        const unsigned long long kd = span_doc_key(seed, 1ull << 40, d);
        uint64_t n_runs = 0, kept = 0;
        bool in_run = false;
        for (uint32_t j = 0; j < lens[d]; ++j, ++i) {
            if (cut && j >= cut) continue;
            ++kept;
            const uint32_t w = with_words ? words[i] : 0u;
            const uint64_t v = whole_word ? (w & 0x7FFFFFFFu) : j;
            bool noise = false;
            for (uint64_t u = v >= max_len - 1 ? v - (max_len - 1) : 0; u <= v && !(w & MASK_WORD_SPECIAL); ++u) {
                const unsigned long long r = enc_rnd(kd, SPAN_STREAM_DRAW, u);
                if ((r >> 32) >= open) continue;
                uint64_t l = 1;
                for (uint32_t k = 0; k + 1 < max_len; ++k) l += (r & 0xFFFFFFFFull) < len[k];
                noise = noise || u + l > v;
            }
            if (!noise) {
                in_run = false;
                exp_in.push_back(ids[i]);
                continue;
            }
            if (!in_run) {
                in_run = true;
                if (++n_runs <= K) {
                    exp_in.push_back(sent[n_runs - 1]);
                    exp_tgt.push_back(sent[n_runs - 1]);
                }
            }
            (n_runs <= K ? exp_tgt : exp_in).push_back(ids[i]);
        }
        if (final_sentinel && kept) exp_tgt.push_back(sent[n_runs < K ? n_runs : K]);
    }
    if (in_off[nd] != exp_in.size() || tgt_off[nd] != exp_tgt.size()) return false;
    for (size_t k = 0; k < exp_in.size(); ++k)
        if (exp_in[k] != got_in[k]) return false;
    for (size_t k = 0; k < exp_tgt.size(); ++k)
        if (exp_tgt[k] != got_tgt[k]) return false;
    return true;
}
}  // namespace

int main() {
    const std::vector<std::vector<uint32_t>> sets = {
        {0, 0, 5, 0, 0, 7, 300, 0, 3, 0, 0}, std::vector<uint32_t>(600, 1), {3, 3, 700, 3, 3}, {0, 0, 0}, {0}, {256, 256, 1}, {1000}};
    int bad = 0, runs = 0;
    for (const auto &lens : sets)
        for (uint32_t flags = 0; flags < 4; ++flags)
            for (int with_words = (int)(flags & 1u); with_words < 2; ++with_words)
                for (uint32_t max_len : {1u, 5u, 32u})
                    for (uint64_t cut : {0ull, 2ull, 260ull}) {
                        bad += !agrees(lens, true, with_words != 0, flags, 7 + runs, max_len, (1ull << 32) / 5, 2 + runs % 40, cut);
                        ++runs;
                    }
    for (uint32_t n : {0u, 77u, 515u})  // n_docs = 1 with doc_off = NULL
        for (uint64_t open : {0ull, 1ull << 30, 1ull << 32}) {
            bad += !agrees({n}, false, true, 3, 3, 10, open, 3, 0);
            ++runs;
        }
    printf("span_model: %d runs, %d differ\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
