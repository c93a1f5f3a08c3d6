// CPU model of the windows layout (yabpe_layout_windows): the rules yet-another-bpe_amd/csrc/layout_logic.h adds for it (the
// functions the HIP kernels call), run sequentially in the kernels' shape -- row counts, their exclusive scan, one record per
// output row found by the search in the scan, then the flat output index in pieces, 4 slots per step, walking on across a row
// end with one record read per row touched; the spans in a pass of their own, a wave's 256 slots interleaved over its lanes.
// Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/layout_logic.h"

// Document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids).  spans: NULL or n_ids (start, end) pairs.  piece:
// output slots per "workgroup" (a multiple of 4).  Returns 0 and *out_n_rows, out_rows[*out_n_rows * row_len], the three
// per-row arrays and, with spans, out_spans[*out_n_rows * row_len * 2]; -8 when cap_rows (rows the outputs hold) is too small.
// counters: [0] the longest document [1] documents of more than one row [2] slots kept.
extern "C" int windows_model(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *spans,
                             uint32_t row_len, uint32_t stride, uint32_t pad, uint32_t bos, uint32_t eos, uint32_t flags, uint32_t piece,
                             uint32_t *out_rows, uint32_t *out_doc, uint32_t *out_start, uint32_t *out_len, uint64_t *out_spans,
                             uint64_t cap_rows, uint64_t *out_n_rows, uint64_t *counters) {
    const uint32_t added = lay_n_added(flags), C = row_len - added, step = C - stride;
    auto end = [&](uint32_t d) { return d + 1 < n_docs ? doc_off[d + 1] : n_ids; };
    // count + scan
    std::vector<unsigned long long> row_off(n_docs + 1ull, 0);
    counters[0] = counters[1] = counters[2] = 0;
    for (uint32_t d = 0; d < n_docs; ++d) {
        const unsigned long long n = end(d) - doc_off[d], rows = lay_win_rows(n, C, step);
        row_off[d + 1] = row_off[d] + rows;
        counters[0] = n > counters[0] ? n : counters[0];
        counters[1] += rows > 1;
        counters[2] += rows * added + (rows - 1) * C + lay_win_content(n, rows - 1, C, step);
    }
    const unsigned long long n_rows = row_off[n_docs], n_slots = n_rows * row_len;
    *out_n_rows = n_rows;
    if (n_rows > cap_rows) return -8;
    // rows
    struct Rec { unsigned long long first, content; };
    std::vector<Rec> rec(n_rows);
    for (unsigned long long r = 0; r < n_rows; ++r) {
        const uint32_t d = lay_find_doc(row_off.data(), 0, 0, n_docs - 1, r);
        const unsigned long long k = r - row_off[d], content = lay_win_content(end(d) - doc_off[d], k, C, step);
        out_doc[r] = d;
        out_start[r] = (uint32_t)(k * step);
        out_len[r] = (uint32_t)content + added;
        rec[r] = {doc_off[d] + k * step, content};
        // (the record names the slots lay_win_slot names from the document itself)
        for (uint32_t col = 0; col < row_len; ++col)
            if (lay_win_row_slot(rec[r].first, content, row_len, flags, col) != lay_win_slot(doc_off[d], end(d) - doc_off[d], k, row_len, stride, flags, col))
                return -1;
    }
    // write
    for (unsigned long long f0 = 0; f0 < n_slots; f0 += piece)
        for (unsigned long long f = f0; f < f0 + piece && f < n_slots; f += 4) {
            unsigned long long row = f / row_len;
            uint32_t col = (uint32_t)(f % row_len);
            Rec rc = rec[row];
            for (int k = 0; k < 4; ++k) {
                if (f + k >= n_slots) break;
                const unsigned long long slot = lay_win_row_slot(rc.first, rc.content, row_len, flags, col);
                out_rows[f + k] = slot == LAY_SLOT_PAD ? pad : slot == LAY_SLOT_BOS ? bos : slot == LAY_SLOT_EOS ? eos : ids[slot];
                if (++col == row_len && row + 1 < n_rows) {
                    col = 0;
                    rc = rec[++row];
                }
            }
        }
    // spans: a pass of its own over the 256 slots of a "wave" and step -- lane l takes the slots l, 64 + l, 128 + l, 192 + l
    if (spans)
        for (unsigned long long fw = 0; fw < n_slots; fw += 256)
            for (int k = 0; k < 4; ++k)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const unsigned long long g = fw + 64 * k + lane;
                    if (g >= n_slots) continue;
                    const Rec rc = rec[g / row_len];
                    const unsigned long long slot = lay_win_row_slot(rc.first, rc.content, row_len, flags, (uint32_t)(g % row_len));
                    out_spans[2 * g] = slot < LAY_SLOT_EOS ? spans[2 * slot] : 0;
                    out_spans[2 * g + 1] = slot < LAY_SLOT_EOS ? spans[2 * slot + 1] : 0;
                }
    return 0;
}
