// CPU model of the device encoder with spans (yabpe_encode_spans): the split and merges as tests/hostmodel/encode_model.cpp
// runs them, plus the span rules of yet-another-bpe_amd/csrc/encode_logic.h that the HIP kernels call -- the token starts
// of enc_merge_heap, and the char unit through the lead-byte prefix per granule (enc_lead_chunk / enc_lead).  Test
// infrastructure only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/encode_logic.h"
#include "../../yet-another-bpe_amd/csrc/unicode_classes.inc"

static std::vector<uint8_t> g_cls;

static void build_table() {
    if (!g_cls.empty()) return;
    g_cls.assign(0x110000, PT_O);
    for (unsigned r = 0; r < YB_UNICODE_CLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_CLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_CLASS_NRUNS ? YB_UNICODE_CLASS_RUNS[r + 1][0] : 0x110000;
        memset(g_cls.data() + lo, (int)YB_UNICODE_CLASS_RUNS[r][1], hi - lo);
    }
}

// Returns 0 (ids in out_ids[0..*out_n), (start, end) pairs relative to each id's document in out_spans[0..2 * *out_n),
// per-document offsets in out_doc_off[0..n_docs]), the model builder's error code, or -8 when cap is too small.
// chars != 0: code points instead of bytes.  *err_pos = first malformed UTF-8 byte or -1.
extern "C" int spans_model(const uint8_t *text_in, uint64_t n, const uint64_t *doc_off, uint32_t n_docs, const uint8_t *vocab_bytes,
                           const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab, const uint8_t *merge_bytes,
                           const uint64_t *merge_off, uint32_t n_merges, const uint8_t *sp_bytes, const uint32_t *sp_off, uint32_t n_sp,
                           uint32_t unk_id, int chars, uint32_t *out_ids, uint64_t *out_spans, uint64_t cap, uint64_t *out_n,
                           uint64_t *out_doc_off, int64_t *err_pos) {
    build_table();
    EncModelHost m;
    const int rc = enc_build_model(vocab_bytes, vocab_off, vocab_ids, n_vocab, merge_bytes, merge_off, n_merges, sp_bytes, sp_off, n_sp,
                                   unk_id, &m);
    if (rc) return rc;
    const EncTable t = m.table();
    std::vector<EncChunk> aligned(n / 16 + 1); // enc_lead reads the text in aligned 16-byte chunks
    uint8_t *text = (uint8_t *)aligned.data();
    memcpy(text, text_in, n);
    std::vector<uint8_t> meta(n + 1, 0), sflag(n + 1, 0);
    for (uint32_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) meta[doc_off[d]] |= PT_CHUNK0;
    if (n_sp) {
        uint32_t max_len = 0;
        for (uint32_t s = 0; s < n_sp; ++s) max_len = sp_off[s + 1] - sp_off[s] > max_len ? sp_off[s + 1] - sp_off[s] : max_len;
        const PtView v{text, meta.data(), n, 0};
        const PtSpecials sp{sp_bytes, sp_off, n_sp, max_len};
        auto occ = [&](uint64_t q) -> uint32_t { return pt_special_at(v, sp, q); };
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t o = occ(i);
            if (o && enc_special_is_head(v, sp, occ, i)) enc_special_walk(v, sp, occ, sflag.data(), i, o);
        }
        for (uint64_t i = 0; i < n; ++i)
            if (enc_segment_start(sflag.data(), i)) meta[i] |= PT_CHUNK0;
    }
    *err_pos = -1;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t end = n;
        for (uint64_t k = i + 1; k < i + 4 && k < n; ++k)
            if (meta[k] & PT_CHUNK0) {
                end = k;
                break;
            }
        bool bad = false;
        const PtView v0{text, meta.data(), n, 0};
        const uint8_t c = pt_classify(v0, i, end, g_cls.data(), &bad);
        meta[i] = (uint8_t)((meta[i] & PT_CHUNK0) | c);
        if (bad && *err_pos < 0) *err_pos = (int64_t)i;
    }
    if (*err_pos >= 0) return 0;
    const PtView v{text, meta.data(), n, 0};
    std::vector<uint64_t> starts;
    for (uint64_t i = 0; i < n; ++i)
        if (pt_is_start(v, i, -1) && sflag[i] != ENC_INSIDE) starts.push_back(i);
    starts.push_back(n);
    // the lead-byte prefix: one count per granule, then its exclusive scan
    const uint64_t n_gran = (n + ENC_GRANULE - 1) / ENC_GRANULE;
    std::vector<unsigned long long> table(n_gran + 1, 0);
    for (uint64_t g = 0; g < n_gran; ++g) {
        uint32_t cnt = 0;
        for (uint64_t c = g * ENC_GRANULE; c < (g + 1) * ENC_GRANULE && c < n; c += 16) cnt += enc_lead_chunk(text, n, c, n - c < 16 ? (uint32_t)(n - c) : 16u);
        table[g + 1] = table[g] + cnt;
    }
    auto lead = [&](unsigned long long p) { return enc_lead(text, n, table.data(), p); };
    std::vector<uint32_t> tok, nxt, prv, one(1, 0);
    std::vector<unsigned long long> heap;
    uint64_t k = 0;
    uint32_t d = 0; // documents whose start is at or before the pre-token at hand: it belongs to document d - 1
    for (size_t w = 0; w + 1 < starts.size(); ++w) {
        const uint64_t s = starts[w], L = starts[w + 1] - s;
        while (d < n_docs && doc_off[d] <= s) out_doc_off[d++] = k;
        const uint64_t ds = doc_off[d - 1];
        uint32_t cnt = 0;
        const uint32_t *ids = nullptr, *pos = nullptr;
        if (sflag[s] != 0) {
            const uint32_t idx = sflag[s] - 1u;
            cnt = m.sp_has[idx] ? 1u : 0u;
            ids = &m.sp_id[idx];
            pos = one.data();
        } else {
            tok.resize(L);
            nxt.resize(L);
            prv.resize(L);
            heap.resize(3 * L);
            cnt = enc_merge_heap(text + s, (uint32_t)L, t, tok.data(), nxt.data(), prv.data(), heap.data());
            for (uint32_t j = 0; j < cnt; ++j) tok[j] = m.out_id[tok[j]];
            ids = tok.data();
            pos = nxt.data();
        }
        if (k + cnt > cap) return -8;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t a = s + enc_heap_start(pos, j), e = s + enc_token_end(pos, cnt, (uint32_t)L, j);
            out_ids[k] = ids[j];
            out_spans[2 * k] = chars ? enc_char_start(lead, a) - lead(ds) : a - ds;
            out_spans[2 * k + 1] = chars ? enc_char_end(lead, e) - lead(ds) : e - ds;
            ++k;
        }
    }
    while (d <= n_docs) out_doc_off[d++] = k;
    *out_n = k;
    return 0;
}
