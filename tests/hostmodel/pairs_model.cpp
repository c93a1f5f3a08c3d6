// CPU model of the pairs layout (yabpe_layout_pairs): Rule 4 of yet-another-bpe_amd/csrc/layout_logic.h (the functions the HIP
// kernels call), run sequentially in the kernels' shape -- the counters and, in windows mode, the row counts and their exclusive
// scan; one record per output row, found in windows mode by the search in the scan; then the flat output index in pieces, 4
// slots per step, walking on across a row end with one record read per row touched; the spans in a pass of their own, a wave's
// 256 slots interleaved over its lanes.  Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/layout_logic.h"

// what the two sides keep in one of the truncation modes (Rule 4's closed forms)
extern "C" void pairs_keep(uint64_t la, uint64_t lb, uint64_t C, uint32_t mode, uint64_t *ka, uint64_t *kb) {
    unsigned long long a, b;
    lay_pair_keep(la, lb, C, mode, &a, &b);
    *ka = a;
    *kb = b;
}

// Document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids); documents 2p and 2p + 1 are pair p.  spans: NULL or
// n_ids (start, end) pairs.  piece: output slots per "workgroup" (a multiple of 4).  Returns 0 and *out_n_rows, out_rows and
// out_types[*out_n_rows * row_len], the four per-row arrays and, with spans, out_spans[*out_n_rows * row_len * 2]; -8 when
// cap_rows (rows the outputs hold) is too small.  counters: [0] the longest document [1] pairs that lost an id or took several
// rows [2] ids dropped [3] slots kept.
extern "C" int pairs_model(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *spans, uint32_t row_len,
                           uint32_t mode, uint32_t stride, uint32_t sep, uint32_t n_sep, uint32_t pad, uint32_t bos, uint32_t eos, uint32_t flags,
                           uint32_t piece, uint32_t *out_rows, uint8_t *out_types, uint32_t *out_pair, uint32_t *out_start, uint32_t *out_first,
                           uint32_t *out_second, uint64_t *out_spans, uint64_t cap_rows, uint64_t *out_n_rows, uint64_t *counters) {
    const uint32_t added = lay_n_added(flags) + n_sep, C = row_len - added, n_pairs = n_docs / 2;
    const bool windows = mode == LAY_PAIRS_WINDOWS;
    auto end = [&](uint32_t d) { return d + 1 < n_docs ? doc_off[d + 1] : n_ids; };
    // count (+ scan in windows mode; else row p = pair p)
    std::vector<unsigned long long> row_off(n_pairs + 1ull, 0);
    counters[0] = counters[1] = counters[2] = counters[3] = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        const unsigned long long la = doc_off[2 * p + 1] - doc_off[2 * p], lb = end(2 * p + 1) - doc_off[2 * p + 1];
        const unsigned long long longer = la > lb ? la : lb;
        counters[0] = longer > counters[0] ? longer : counters[0];
        const unsigned long long rows = lay_pair_rows(la, lb, C, mode, stride);
        row_off[p + 1] = row_off[p] + rows;
        if (windows) {
            const unsigned long long ka = lay_pair_first(la, C, stride), Cb = C - ka, step = Cb - stride;
            counters[1] += rows > 1 || ka < la;
            counters[3] += rows * (added + ka) + (rows - 1) * Cb + lay_win_content(lb, rows - 1, Cb, step);
        } else {
            unsigned long long ka, kb;
            lay_pair_keep(la, lb, C, mode, &ka, &kb);
            counters[1] += ka + kb < la + lb;
            counters[2] += la + lb - ka - kb;
            counters[3] += added + ka + kb;
        }
    }
    const unsigned long long n_rows = row_off[n_pairs], n_slots = n_rows * row_len;
    *out_n_rows = n_rows;
    if (n_rows > cap_rows) return -8;
    // rows
    struct Rec { unsigned long long a0, b0; uint32_t ka, kb; };
    std::vector<Rec> rec(n_rows);
    for (unsigned long long r = 0; r < n_rows; ++r) {
        unsigned long long p = r, k = 0;
        if (windows) {
            p = lay_find_doc(row_off.data(), 0, 0, n_pairs - 1, r);
            k = r - row_off[p];
        }
        const unsigned long long a = doc_off[2 * p], b = doc_off[2 * p + 1], e = end((uint32_t)(2 * p + 1));
        unsigned long long ka, s, kb;
        lay_pair_row(b - a, e - b, k, C, mode, stride, &ka, &s, &kb);
        if (ka + kb > C || ka > b - a || s + kb > e - b) return -1; // a row that does not fit, or ids that are not the side's
        out_pair[r] = (uint32_t)p;
        out_start[r] = (uint32_t)s;
        out_first[r] = (uint32_t)ka;
        out_second[r] = (uint32_t)kb;
        rec[r] = {a, b + s, (uint32_t)ka, (uint32_t)kb};
    }
    // write
    for (unsigned long long f0 = 0; f0 < n_slots; f0 += piece)
        for (unsigned long long f = f0; f < f0 + piece && f < n_slots; f += 4) {
            unsigned long long row = f / row_len;
            uint32_t col = (uint32_t)(f % row_len);
            Rec rc = rec[row];
            for (int k = 0; k < 4; ++k) {
                if (f + k >= n_slots) break;
                uint32_t type;
                const unsigned long long slot = lay_pair_slot(rc.a0, rc.ka, rc.b0, rc.kb, n_sep, row_len, flags, col, &type);
                out_rows[f + k] = slot == LAY_SLOT_PAD ? pad : slot == LAY_SLOT_BOS ? bos : slot == LAY_SLOT_EOS ? eos : slot == LAY_SLOT_SEP ? sep : ids[slot];
                out_types[f + k] = (uint8_t)type;
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
                    uint32_t type;
                    const unsigned long long slot = lay_pair_slot(rc.a0, rc.ka, rc.b0, rc.kb, n_sep, row_len, flags, (uint32_t)(g % row_len), &type);
                    out_spans[2 * g] = slot < LAY_SLOT_SEP ? spans[2 * slot] : 0;
                    out_spans[2 * g + 1] = slot < LAY_SLOT_SEP ? spans[2 * slot + 1] : 0;
                }
    return 0;
}
