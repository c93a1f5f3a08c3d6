// CPU model of the fixed-shape batch layouts: the index rules of yet-another-bpe_amd/csrc/layout_logic.h (the functions the HIP
// kernels call), run sequentially in the kernels' shape -- flat output index, 4 slots per step, a window of stream offsets per
// piece seen through an origin.  Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/layout_logic.h"

namespace {
uint32_t value(const uint32_t *ids, unsigned long long slot, uint32_t pad, uint32_t bos, uint32_t eos) {
    return slot == LAY_SLOT_PAD ? pad : slot == LAY_SLOT_BOS ? bos : slot == LAY_SLOT_EOS ? eos : ids[slot];
}
} // namespace

// Document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids).  row_len 0: the longest sequence.  Returns 0 and
// *out_row_len, out_rows[n_docs * *out_row_len], out_len[n_docs]; -8 when cap (slots of out_rows) is too small.
extern "C" int layout_model_pad(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint32_t row_len, uint32_t pad,
                                uint32_t bos, uint32_t eos, uint32_t flags, uint32_t *out_rows, uint64_t cap, uint32_t *out_len,
                                uint32_t *out_row_len) {
    auto end = [&](uint32_t d) { return d + 1 < n_docs ? doc_off[d + 1] : n_ids; };
    if (!row_len)
        for (uint32_t d = 0; d < n_docs; ++d) {
            const unsigned long long seq = end(d) - doc_off[d] + lay_n_added(flags);
            row_len = seq > row_len ? (uint32_t)seq : row_len;
        }
    *out_row_len = row_len;
    if ((uint64_t)row_len * n_docs > cap) return -8;
    for (uint32_t d = 0; d < n_docs; ++d) {
        const unsigned long long a = doc_off[d], n = end(d) - a;
        out_len[d] = (uint32_t)lay_kept(n, row_len, flags);
        for (uint32_t col = 0; col < row_len; ++col)
            out_rows[(uint64_t)d * row_len + col] = value(ids, lay_pad_slot(a, n, row_len, flags, col), pad, bos, eos);
    }
    return 0;
}

// piece: output slots per "workgroup" (a multiple of 4); stage: offsets a window may hold before the search goes to the whole
// array.  Returns 0 and *out_n_rows, three arrays of *out_n_rows * row_len; -8 when cap is too small.
extern "C" int layout_model_pack(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint32_t row_len, uint32_t pad,
                                 uint32_t bos, uint32_t eos, uint32_t flags, uint32_t piece, uint32_t stage, uint32_t *out_ids,
                                 uint32_t *out_doc, uint32_t *out_pos, uint64_t cap, uint64_t *out_n_rows) {
    const uint32_t added = lay_n_added(flags);
    std::vector<unsigned long long> soff(n_docs + 1ull);
    for (uint32_t d = 0; d < n_docs; ++d) soff[d] = doc_off[d] + (unsigned long long)added * d;
    const unsigned long long total = soff[n_docs] = n_ids + (unsigned long long)added * n_docs;
    const unsigned long long n_rows = lay_pack_rows(total, row_len, flags), n_slots = n_rows * row_len;
    *out_n_rows = n_rows;
    if (n_slots > cap) return -8;
    std::vector<unsigned long long> window;
    for (unsigned long long g0 = 0; g0 < n_slots; g0 += piece) {
        const unsigned long long g1 = g0 + piece < n_slots ? g0 + piece : n_slots, e = g1 < total ? g1 : total;
        uint32_t d0 = 0, d1 = 0, org = 0;
        const unsigned long long *w = soff.data();
        if (g0 < e) {
            d0 = lay_find_doc(soff.data(), 0, 0, n_docs - 1, g0);
            d1 = lay_find_doc(soff.data(), 0, d0, n_docs - 1, e - 1);
            if (d1 - d0 + 2 <= stage) {
                window.assign(soff.begin() + d0, soff.begin() + d1 + 2);
                w = window.data();
                org = d0;
            }
        }
        for (unsigned long long g = g0; g < g1; g += 4) {
            uint32_t d = d0;
            unsigned long long sd = 0, next = 0;
            for (int k = 0; k < 4; ++k) {
                const unsigned long long gg = g + k;
                if (gg >= g1) break;
                if (gg >= total) {
                    out_ids[gg] = pad;
                    out_doc[gg] = LAY_NO_DOC;
                    out_pos[gg] = 0;
                    continue;
                }
                if (gg >= next) {
                    d = lay_find_doc(w, org, next ? d + 1 : d0, d1, gg);
                    sd = w[d - org];
                    next = w[d + 1 - org];
                }
                unsigned long long pos;
                out_ids[gg] = value(ids, lay_pack_slot(gg, d, sd, next, flags, &pos), pad, bos, eos);
                out_doc[gg] = d;
                out_pos[gg] = (uint32_t)pos;
            }
        }
    }
    return 0;
}
