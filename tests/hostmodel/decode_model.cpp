// CPU model of the device decoder: the id table and the per-byte UTF-8 roles of yet-another-bpe_amd/csrc/decode_logic.h (the
// functions the HIP kernels call), run sequentially over a batch of documents.  Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/decode_logic.h"

// Returns 0 (text in out[0..*out_n), per-document offsets in out_doc_off[0..n_docs]), the table builder's error code, or -8
// when cap is too small.  counts = (ids skipped as unknown, U+FFFD written, documents repaired).
extern "C" int decode_model(const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab,
                            const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint8_t *out, uint64_t cap,
                            uint64_t *out_n, uint64_t *out_doc_off, uint64_t *counts) {
    DecTableHost t;
    const int rc = dec_build_table(vocab_off, vocab_ids, n_vocab, &t);
    if (rc) return rc;
    const uint64_t n_tab = t.ent.size() / 2;
    counts[0] = counts[1] = counts[2] = 0;
    std::vector<uint8_t> doc;
    uint64_t o = 0;
    for (uint32_t d = 0; d < n_docs; ++d) {
        const uint64_t a = doc_off[d], b = d + 1 < n_docs ? doc_off[d + 1] : n_ids;
        doc.clear();
        for (uint64_t i = a; i < b; ++i) {
            if (ids[i] >= n_tab || t.ent[2ull * ids[i]] == DEC_UNKNOWN) {
                ++counts[0];
                continue;
            }
            const uint32_t off = t.ent[2ull * ids[i]], len = t.ent[2ull * ids[i] + 1];
            doc.insert(doc.end(), vocab_bytes + off, vocab_bytes + off + len);
        }
        out_doc_off[d] = o;
        const DecView v{doc.data(), 0};
        bool bad = false;
        for (uint64_t p = 0; p < doc.size(); ++p) {
            const uint32_t ol = dec_out_len(v, p, 0, doc.size());
            if (o + ol > cap) return -8;
            dec_emit(doc[p], ol, out + o);
            o += ol;
            counts[1] += ol == 3 ? 1 : 0;
            bad |= ol != 1;
        }
        counts[2] += bad ? 1 : 0;
    }
    out_doc_off[n_docs] = o;
    *out_n = o;
    return 0;
}
