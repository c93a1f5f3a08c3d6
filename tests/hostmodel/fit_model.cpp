// CPU model of the whole-document packing: the rules of yet-another-bpe_amd/csrc/fit_logic.h (the functions the host driver and
// the HIP kernels call), run sequentially in the kernels' shape -- keys and histogram per document, radix passes whose ranks are
// (steps before) + (waves before) + (lanes below), the plan, and a write over the flat output index with 4 slots per step and a
// window of the plan per piece seen through its origins.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/fit_logic.h"

namespace {
uint32_t value(const uint32_t *ids, unsigned long long slot, uint32_t pad, uint32_t bos, uint32_t eos) {
    return slot == LAY_SLOT_PAD ? pad : slot == LAY_SLOT_BOS ? bos : slot == LAY_SLOT_EOS ? eos : ids[slot];
}

// one radix pass in the scatter kernel's shape: tiles of `tile` keys in steps of `block` keys, a wave = 64 consecutive keys
void radix_pass(const std::vector<uint32_t> &kin, const std::vector<uint32_t> &vin, uint32_t pass, uint32_t block, uint32_t tile,
                std::vector<uint32_t> *kout, std::vector<uint32_t> *vout) {
    const size_t n = kin.size(), n_tiles = (n + tile - 1) / tile;
    std::vector<unsigned long long> counts(256 * n_tiles, 0), offs(256 * n_tiles, 0);
    for (size_t i = 0; i < n; ++i) ++counts[fit_digit(kin[i], pass) * n_tiles + i / tile];
    for (size_t k = 1; k < counts.size(); ++k) offs[k] = offs[k - 1] + counts[k - 1];
    kout->assign(n, 0);
    vout->assign(n, 0);
    for (size_t t = 0; t < n_tiles; ++t) {
        unsigned long long base[256];
        for (uint32_t g = 0; g < 256; ++g) base[g] = offs[g * n_tiles + t];
        for (size_t s0 = t * tile; s0 < std::min(n, (t + 1) * (size_t)tile); s0 += block) {       // a step
            unsigned long long step[256] = {0};
            for (size_t w0 = s0; w0 < std::min(n, s0 + block); w0 += 64) {                          // a wave of it
                uint32_t wave[256] = {0};
                for (size_t i = w0; i < std::min(n, w0 + 64); ++i) {                                // its lanes, the lowest first
                    const uint32_t g = fit_digit(kin[i], pass);
                    const unsigned long long o = base[g] + step[g] + wave[g]++;
                    (*kout)[o] = kin[i];
                    (*vout)[o] = vin[i];
                }
                for (uint32_t g = 0; g < 256; ++g) step[g] += wave[g];
            }
            for (uint32_t g = 0; g < 256; ++g) base[g] += step[g];
        }
    }
}
} // namespace

// hist[0 .. C] -> the flat plan: first[n_shapes + 1], place[n_shapes + 1], pl[4 * n_places] = (col, len, rank, per_row) per place.
// Returns 0, or -8 when a capacity (entries of first / place, places of pl) is too small.
extern "C" int fit_model_plan(const uint32_t *hist, uint32_t C, uint64_t *first, uint32_t *place, uint32_t *pl, uint32_t cap_shapes,
                              uint32_t cap_places, uint32_t *n_shapes, uint32_t *n_places, uint64_t *n_rows, uint64_t *steps) {
    FitPlan P;
    fit_plan(hist, C, &P);
    *n_shapes = P.n_shapes();
    *n_places = (uint32_t)P.pl.size();
    *n_rows = P.n_rows;
    *steps = P.steps;
    if (P.first.size() > cap_shapes || P.pl.size() > cap_places) return -8;
    for (size_t s = 0; s < P.first.size(); ++s) {
        first[s] = P.first[s];
        place[s] = P.place[s];
    }
    for (size_t p = 0; p < P.pl.size(); ++p) {
        pl[4 * p] = P.pl[p].col;
        pl[4 * p + 1] = P.pl[p].len;
        pl[4 * p + 2] = P.pl[p].rank;
        pl[4 * p + 3] = P.pl[p].per_row;
    }
    return 0;
}

// Document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids).  block, tile: the sort's step and tile (keys);
// piece: output slots per "workgroup" (a multiple of 4); stage_shapes, stage_places: what a window may hold before the searches
// go to the whole plan.  Returns 0 and *out_n_rows, three arrays of *out_n_rows * C, out_used[*out_n_rows], out_sorted[n_docs]
// (the documents stably by n_d); -8 when cap (slots) or cap_rows is too small.
extern "C" int fit_model_rows(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint32_t C, uint32_t pad, uint32_t bos,
                              uint32_t eos, uint32_t flags, uint32_t block, uint32_t tile, uint32_t piece, uint32_t stage_shapes,
                              uint32_t stage_places, uint32_t *out_ids, uint32_t *out_doc, uint32_t *out_pos, uint32_t *out_used, uint64_t cap,
                              uint64_t cap_rows, uint32_t *out_sorted, uint64_t *out_n_rows) {
    auto doc_end = [&](uint32_t d) { return d + 1 < n_docs ? doc_off[d + 1] : n_ids; };
    // lengths
    std::vector<uint32_t> key(n_docs), val(n_docs), hist((size_t)C + 1, 0);
    uint32_t max_key = 0;
    for (uint32_t d = 0; d < n_docs; ++d) {
        key[d] = (uint32_t)lay_kept(doc_end(d) - doc_off[d], C, flags);
        val[d] = d;
        ++hist[key[d]];
        max_key = std::max(max_key, key[d]);
    }
    *out_n_rows = 0;
    if (!max_key) return 0;
    // sort
    for (uint32_t pass = 0; pass < fit_sort_passes(max_key); ++pass) {
        std::vector<uint32_t> k2, v2;
        radix_pass(key, val, pass, block, tile, &k2, &v2);
        key.swap(k2);
        val.swap(v2);
    }
    for (uint32_t d = 0; d < n_docs; ++d) out_sorted[d] = val[d];
    // plan
    FitPlan P;
    fit_plan(hist.data(), C, &P);
    const unsigned long long n_rows = P.n_rows, n_slots = n_rows * C;
    *out_n_rows = n_rows;
    if (n_slots > cap || n_rows > cap_rows) return -8;
    // write
    std::vector<unsigned long long> w_first;
    std::vector<uint32_t> w_place;
    std::vector<FitPlace> w_pl;
    for (unsigned long long g0 = 0; g0 < n_slots; g0 += piece) {
        const unsigned long long g1 = g0 + piece < n_slots ? g0 + piece : n_slots;
        const uint32_t s0 = lay_find_doc(P.first.data(), 0, 0, P.n_shapes() - 1, g0 / C);
        const uint32_t s1 = lay_find_doc(P.first.data(), 0, s0, P.n_shapes() - 1, (g1 - 1) / C);
        const uint32_t p0 = P.place[s0], p1 = P.place[s1 + 1];
        FitView V{P.first.data(), P.place.data(), P.pl.data(), 0, 0};
        if (s1 - s0 + 1 <= stage_shapes && p1 - p0 <= stage_places) {
            w_first.assign(P.first.begin() + s0, P.first.begin() + s1 + 2);
            w_place.assign(P.place.begin() + s0, P.place.begin() + s1 + 2);
            w_pl.assign(P.pl.begin() + p0, P.pl.begin() + p1);
            V = FitView{w_first.data(), w_place.data(), w_pl.data(), s0, p0};
        }
        for (unsigned long long g = g0; g < g1; g += 4) { // one lane, one step
            unsigned long long row = g / C, a = 0, n = 0;
            uint32_t col = (uint32_t)(g % C), shape = s0, end = 0, d = LAY_NO_DOC, c0 = 0, len = 0;
            for (int k = 0; k < 4 && g + k < g1; ++k) {
                if (col >= end) {
                    uint32_t used;
                    const uint32_t p = fit_slot(V, shape, s1, row, col, C, &shape, &end, &used);
                    if (col == 0) out_used[row] += used + 1; // (+ 1: a row written twice, or never, shows)
                    d = LAY_NO_DOC;
                    if (p != FIT_PAD) {
                        const FitPlace q = V.pl[p - V.p_org];
                        d = val[q.rank + (row - V.first[shape - V.s_org]) * q.per_row];
                        a = doc_off[d];
                        n = doc_end(d) - a;
                        c0 = q.col;
                        len = q.len;
                    }
                }
                out_ids[g + k] = d == LAY_NO_DOC ? pad : value(ids, lay_pad_slot(a, n, len, flags, col - c0), pad, bos, eos);
                out_doc[g + k] = d;
                out_pos[g + k] = d == LAY_NO_DOC ? 0u : col - c0;
                if (++col == C) {
                    col = 0;
                    end = 0;
                    ++row;
                }
            }
        }
    }
    for (unsigned long long r = 0; r < n_rows; ++r) out_used[r] -= 1;
    return 0;
}
