// CPU model of the fill-in-the-middle passes: the rule of yet-another-bpe_amd/csrc/fim_logic.h (the functions the kernels of
// yabpe_fim_kernels.h call), run sequentially in the kernels' shape -- the plan per document and one scan of the lengths; the
// write per output slot in blocks of `block` slots, the documents of a block's first and last slot found in the whole offsets
// and every slot's document searched between those two; for the cuts a lead-byte count per `granule` bytes, its scan, and per
// document two table reads, the draws and the selects.  Block and granule are arguments: small ones put a seam everywhere.
// Test infrastructure only.  With -DFIM_MODEL_MAIN: a stand-alone program that runs the model on documents that take every
// path and compares it with a direct walk over the documents (the program a sanitizer build runs).
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/fim_logic.h"

// ids[n_ids], doc_off[n_docs] (NULL with n_docs <= 1: one document), cuts[n_docs] with FIM_PIECES (else NULL), sent = (pre,
// suf, mid, eot) -> out_ids / out_labels (room for n_ids + 4 per output document), out_off[n_out_docs + 1], out_info[4 per
// output document], counters[6] (documents out, PSM, SPM, truncated documents, ids dropped, output slots).  Returns 0; -1 for
// arguments yabpe_fim refuses as invalid, -4 for those past its capacity; -2 if a search left its document; -3 if a store or
// a load would leave its array.
extern "C" int fim_model_run(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *cuts, uint64_t seed,
                             uint64_t first_doc, uint64_t fim, uint64_t spm, const uint32_t *sent, uint32_t ignore, uint64_t max_len, uint32_t flags,
                             uint32_t block, uint32_t *out_ids, uint32_t *out_labels, uint64_t *out_off, uint32_t *out_info, uint64_t *counters) {
    if (!fim_rule_valid(fim, spm, max_len, flags) || block == 0) return -1;
    if (!doc_off && n_docs > 1) return -1;
    std::vector<unsigned long long> docs(1, 0);
    if (doc_off) docs.assign(doc_off, doc_off + n_docs);
    if (docs.empty() || docs[0] != 0) return -1;
    for (size_t d = 1; d < docs.size(); ++d)
        if (docs[d] < docs[d - 1] || docs[d] > n_ids) return -1;
    const bool pieces = (flags & FIM_PIECES) != 0;
    const uint32_t n_in = (uint32_t)docs.size();
    if (pieces && (n_in % 3 != 0 || !cuts)) return -1;
    if (!pieces && cuts) return -1;
    const uint32_t stride = pieces ? 3u : 1u, nd = n_in / stride;
    auto in_start = [&](unsigned long long k) { return k < n_in ? docs[k] : (unsigned long long)n_ids; };
    for (uint32_t d = 0; d < nd; ++d)
        if (in_start((unsigned long long)(d + 1) * stride) - in_start((unsigned long long)d * stride) > FIM_MAX_DOC) return -4;
    if (n_ids > (1ull << 36) || n_ids + fim_extra(flags) * nd > (1ull << 36)) return -4;
    const FimRule R{fim, spm, sent[0], sent[1], sent[2], sent[3], ignore, max_len, flags};
    // ---- plan: one thread per document, then the scan
    std::vector<FimDoc> plan(nd);
    std::vector<unsigned long long> len(nd), off(nd + 1, 0);
    for (int k = 0; k < 6; ++k) counters[k] = 0;
    for (uint32_t d = 0; d < nd; ++d) {
        const unsigned long long k0 = (unsigned long long)d * stride, first = in_start(k0), n = in_start(k0 + stride) - first;
        uint32_t mode;
        unsigned long long a, b;
        if (pieces) {
            mode = cuts[3 * d] == FIM_PSM ? FIM_PSM : cuts[3 * d] == FIM_SPM ? FIM_SPM : FIM_NONE;
            a = in_start(k0 + 1) - first;
            b = in_start(k0 + 2) - first;
        } else {
            const unsigned long long kd = fim_doc_key(seed, first_doc, d);
            mode = fim_mode(kd, fim, spm);
            fim_draw_cuts(kd, mode, n, &a, &b);
        }
        unsigned long long dropped;
        plan[d] = fim_plan(mode, n, a, b, R, &len[d], &dropped);
        counters[1] += mode == FIM_PSM;
        counters[2] += mode == FIM_SPM;
        counters[3] += dropped != 0;
        counters[4] += dropped;
    }
    for (uint32_t d = 0; d < nd; ++d) off[d + 1] = off[d] + len[d];
    const unsigned long long n_out = off[nd];
    counters[0] = nd;
    counters[5] = n_out;
    if (n_out > n_ids + fim_extra(flags) * nd) return -3;
    for (uint32_t d = 0; d <= nd; ++d) out_off[d] = off[d];
    for (uint32_t d = 0; d < nd; ++d) {
        out_info[4 * d] = plan[d].mode;
        out_info[4 * d + 1] = plan[d].p;
        out_info[4 * d + 2] = plan[d].m;
        out_info[4 * d + 3] = plan[d].s;
    }
    // ---- write: one thread per output slot, a block per `block` slots
    for (unsigned long long i0 = 0; i0 < n_out; i0 += block) {
        const unsigned long long il = i0 + block - 1 < n_out ? i0 + block - 1 : n_out - 1;
        const uint32_t d_lo = mask_doc_of(off.data(), i0, 0, nd - 1), d_hi = mask_doc_of(off.data(), il, 0, nd - 1);
        for (unsigned long long i = i0; i <= il; ++i) {
            const uint32_t d = mask_doc_of(off.data(), i, d_lo, d_hi);
            if (off[d] > i || off[d + 1] <= i) return -2;
            const unsigned long long first = docs[(size_t)d * stride], k = i - off[d];
            unsigned long long src;
            if (fim_slot(plan[d], k, R, &src) <= FIM_SLOT_SUFFIX && first + src >= in_start((unsigned long long)(d + 1) * stride)) return -3;
            fim_write_slot(plan[d], k, ids, first, R, &out_ids[i], &out_labels[i]);
        }
    }
    return 0;
}

// text[n_bytes], doc_off[n_docs] (NULL with n_docs <= 1) -> piece_off[3 n_docs], cuts[3 n_docs].  Returns 0; -1 for arguments
// yabpe_fim_cuts refuses; -3 if a select left its document.
extern "C" int fim_model_cuts(const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint64_t seed, uint64_t first_doc,
                              uint64_t fim, uint64_t spm, uint64_t max_len, uint32_t flags, uint32_t granule, uint64_t *piece_off, uint64_t *cuts) {
    if (!fim_rule_valid(fim, spm, max_len, flags) || granule == 0) return -1;
    if (!doc_off && n_docs > 1) return -1;
    std::vector<unsigned long long> docs(1, 0);
    if (doc_off) docs.assign(doc_off, doc_off + n_docs);
    if (docs.empty() || docs[0] != 0) return -1;
    for (size_t d = 1; d < docs.size(); ++d)
        if (docs[d] < docs[d - 1] || docs[d] > n_bytes) return -1;
    // ---- the lead-byte count of every granule and its scan
    const unsigned long long n_gran = (n_bytes + granule - 1) / granule;
    std::vector<unsigned long long> table(n_gran + 1, 0);
    for (unsigned long long g = 0; g < n_gran; ++g) {
        unsigned long long cnt = 0;
        for (unsigned long long c = g * granule; c < (g + 1) * granule && c < n_bytes; ++c) cnt += enc_is_lead(text[c]) ? 1u : 0u;
        table[g + 1] = table[g] + cnt;
    }
    // ---- one thread per document
    for (size_t d = 0; d < docs.size(); ++d) {
        const unsigned long long start = docs[d], end = d + 1 < docs.size() ? docs[d + 1] : (unsigned long long)n_bytes;
        unsigned long long c3[3], p3[3];
        fim_doc_cuts(text, table.data(), granule, start, end, fim_lead(text, table.data(), granule, start), fim_lead(text, table.data(), granule, end),
                     fim_doc_key(seed, first_doc, d), fim, spm, c3, p3);
        if (p3[1] < start || p3[2] < p3[1] || p3[2] > end) return -3;
        for (int k = 0; k < 3; ++k) {
            cuts[3 * d + k] = c3[k];
            piece_off[3 * d + k] = p3[k];
        }
    }
    return 0;
}

#ifdef FIM_MODEL_MAIN
#include <stdio.h>

#include <string>

namespace {
const uint32_t SENT[4] = {9001, 9002, 9003, 9004};

// the model against a walk over the documents that builds every sequence piece by piece
bool agrees(const std::vector<uint32_t> &lens, bool with_off, uint64_t seed, uint64_t fim, uint64_t spm, uint64_t max_len, uint32_t flags, uint32_t block) {
    std::vector<uint32_t> ids;
    std::vector<uint64_t> starts;
    for (uint32_t n : lens) {
        starts.push_back(ids.size());
        for (uint32_t j = 0; j < n; ++j) ids.push_back((uint32_t)(enc_rnd(seed, 1, ids.size()) % 1000));
    }
    const uint32_t nd = (uint32_t)lens.size();
    std::vector<uint32_t> got(ids.size() + 4 * nd + 1), lab(got.size()), info(4 * nd + 1);
    std::vector<uint64_t> off(nd + 2);
    uint64_t cnt[6];
    if (fim_model_run(ids.data(), ids.size(), with_off ? starts.data() : nullptr, nd, nullptr, seed, 1ull << 40, fim, spm, SENT, 0xFFFFFF9Cu, max_len, flags,
                      block, got.data(), lab.data(), off.data(), info.data(), cnt) != 0)
        return false;
    const bool eot = (flags & FIM_EOT) != 0, loss_middle = (flags & FIM_LOSS_MIDDLE) != 0;
    std::vector<uint32_t> exp, exp_lab;
    auto put = [&](uint32_t v, bool labelled) {
        exp.push_back(v);
        exp_lab.push_back(labelled ? v : 0xFFFFFF9Cu);
    };
    for (uint32_t d = 0; d < nd; ++d) {
        if (off[d] != exp.size()) return false;
        const unsigned long long kd = fim_doc_key(seed, 1ull << 40, d), r = enc_rnd(kd, FIM_STREAM_MODE, 0), n = lens[d];
        const uint32_t *doc = ids.data() + starts[d];
        if ((r >> 32) >= fim) {
            for (unsigned long long j = 0; j < n && (!max_len || j < max_len); ++j) put(doc[j], true);
            continue;
        }
        const bool is_spm = (r & 0xFFFFFFFFull) < spm;
        const unsigned long long x = enc_rnd(kd, FIM_STREAM_CUT, 0) % (n + 1), y = enc_rnd(kd, FIM_STREAM_CUT, 1) % (n + 1);
        unsigned long long a = x < y ? x : y, b = x < y ? y : x, p0 = 0, m_end = b, s_end = n;
        if (max_len) {
            unsigned long long e = n > max_len - 3 - eot ? n - (max_len - 3 - eot) : 0;
            while (e && s_end > b) --s_end, --e;
            while (e && p0 < a) ++p0, --e;
            while (e && m_end > a) --m_end, --e;
        }
        put(SENT[0], !loss_middle);
        if (!is_spm)
            for (unsigned long long j = p0; j < a; ++j) put(doc[j], !loss_middle);
        put(SENT[1], !loss_middle);
        for (unsigned long long j = b; j < s_end; ++j) put(doc[j], !loss_middle);
        put(SENT[2], !loss_middle);
        if (is_spm)
            for (unsigned long long j = p0; j < a; ++j) put(doc[j], !loss_middle);
        for (unsigned long long j = a; j < m_end; ++j) put(doc[j], true);
        if (eot) put(SENT[3], true);
        if (info[4 * d] != (is_spm ? 2u : 1u) || info[4 * d + 1] != a - p0 || info[4 * d + 2] != m_end - a || info[4 * d + 3] != s_end - b) return false;
    }
    if (off[nd] != exp.size() || cnt[5] != exp.size()) return false;
    for (size_t k = 0; k < exp.size(); ++k)
        if (exp[k] != got[k] || exp_lab[k] != lab[k]) return false;
    return true;
}

// the cuts against a walk over the code points of every document
bool cuts_agree(const std::vector<std::string> &texts, uint64_t seed, uint32_t granule) {
    std::string buf;
    std::vector<uint64_t> starts;
    for (const auto &t : texts) {
        starts.push_back(buf.size());
        buf += t;
    }
    const uint32_t nd = (uint32_t)texts.size();
    std::vector<uint64_t> po(3 * nd), cu(3 * nd);
    if (fim_model_cuts((const uint8_t *)buf.data(), buf.size(), starts.data(), nd, seed, 5, 1ull << 32, 1ull << 31, 0, 0, granule, po.data(), cu.data()) != 0)
        return false;
    for (uint32_t d = 0; d < nd; ++d) {
        std::vector<uint64_t> at;  // the byte of every code point, and the end
        for (size_t k = 0; k < texts[d].size(); ++k)
            if (enc_is_lead((uint8_t)texts[d][k])) at.push_back(starts[d] + k);
        const uint64_t n = at.size();
        at.push_back(starts[d] + texts[d].size());
        const unsigned long long kd = fim_doc_key(seed, 5, d);
        const uint64_t x = enc_rnd(kd, FIM_STREAM_CUT, 0) % (n + 1), y = enc_rnd(kd, FIM_STREAM_CUT, 1) % (n + 1), a = x < y ? x : y, b = x < y ? y : x;
        if (cu[3 * d + 1] != a || cu[3 * d + 2] != b || po[3 * d] != starts[d] || po[3 * d + 1] != at[a] || po[3 * d + 2] != at[b]) return false;
    }
    return true;
}
}  // namespace

int main() {
    const std::vector<std::vector<uint32_t>> sets = {{0, 1, 2, 3, 255, 256, 257, 1000}, std::vector<uint32_t>(300, 1), {0, 0, 0, 5, 300, 0, 0, 7, 0, 0}, {0}, {3, 0}};
    int bad = 0, runs = 0;
    for (const auto &lens : sets)
        for (uint32_t flags = 0; flags < 4; ++flags)
            for (uint64_t max_len : {0ull, 5ull, 6ull, 8ull, 300ull})
                for (uint64_t fim : {0ull, 1ull << 31, 1ull << 32})
                    for (uint32_t block : {256u, 64u, 1u}) {
                        bad += !agrees(lens, true, 11 + runs, fim, (runs % 3) * (1ull << 31), max_len, flags, block);
                        ++runs;
                    }
    for (uint32_t n : {0u, 77u, 515u}) {  // n_docs = 1 with doc_off = NULL
        bad += !agrees({n}, false, 3 + n, 1ull << 32, 1ull << 31, 0, 1, 256);
        ++runs;
    }
    const std::vector<std::string> texts = {"plain ascii", "", "a\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80 mixed \xc3\xa9\xc3\xa9 text", std::string(62, 'a') + "\xf0\x9f\x98\x80" + "bbb",
                                            "", "\xf0\x9f\x98\x80\xf0\x9f\x98\x80\xf0\x9f\x98\x80\xf0\x9f\x98\x80", "x", ""};
    for (uint32_t granule : {64u, 4u, 1u})
        for (uint64_t seed = 0; seed < 40; ++seed) {
            bad += !cuts_agree(texts, seed, granule);
            ++runs;
        }
    printf("fim_model: %d runs, %d differ\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
