// fit_logic.h -- the rules of BBPETokenizer.encode_batch_fit (yet_another_bpe/tokenizer.py): whole documents packed into rows by
// best-fit decreasing.  Shared by the host driver (yabpe_layout_fit in yabpe.hip), the HIP kernels (yabpe_fit_kernels.h) and the
// CPU unit-test model (tests/hostmodel/fit_model.cpp).
//
//   n_d       the length of seq(d) = [bos] + the document's ids + [eos] after the cut to the row length C (Rule 1 of
//             layout_logic.h: the content loses ids from its end, BOS and EOS survive).  A document with n_d == 0 is in no row.
//   plan      Rows with the same remaining room are interchangeable, so best-fit decreasing runs on the histogram H[k] = documents
//             with n_d == k instead of on the documents.  The state maps a shape -- the sequence lengths of a row in placement
//             order, non-increasing -- to the number of rows that have it; room(s) = C - sum(s).  For k = C .. 1 with n = H[k]:
//             among the shapes with a row left and room >= k the one with the smallest room, of several the lexicographically
//             greatest, takes t = room / k sequences a row: min(rows, n / t) rows whole, then one row the rest; with no such shape
//             n / t' rows of (k,) * t' open (t' = C / k) and one row of the rest.  Every k is appended to a shape at most once, so
//             a shape is a list of runs (k, t) with k strictly descending, and the tuple order of two shapes is the
//             lexicographic order of their runs.  Rule 5 (fit_plan).
//   rows      The shapes in descending tuple order, the rows of a shape consecutive.  A row holds its sequences end to end from
//             column 0 in shape order, then padding.
//   dealing   For every k the documents with n_d == k, in ascending d, take the places of length k in row order, within a row
//             left to right.  With the documents sorted stably by n_d (sorted_doc; the documents with n_d == 0 lead it) the
//             place j of the row first + i of a shape is the document sorted_doc[rank + i * per_row]: rank = the documents shorter
//             than k + the places of length k in the rows before `first` + the places of length k left of j in the row,
//             per_row = the places of length k a row of the shape has.
//             Rule 6 (fit_find_place / fit_slot): which place, if any, slot (row, col) lies in.
//   sort      LSD radix passes of 8 bits over the keys n_d (fit_digit); a pass whose digit is 0 in every key is skipped
//             (fit_sort_passes).
#pragma once
#include <stdint.h>

#include "layout_logic.h"

#include <functional>
#include <map>
#include <utility>
#include <vector>

constexpr uint32_t LAY_FIT_FLAGS = LAY_BOS | LAY_EOS;
constexpr uint32_t FIT_MAX_ROW = (1u << 24) - 1;    // the longest row: a sort key has at most three digits
constexpr uint32_t FIT_PAD = 0xFFFFFFFFu;           // `place` of a slot behind the last sequence of its row

// One sequence of the rows of one shape (16 bytes: one load).
struct alignas(16) FitPlace {
    uint32_t col, len;      // its first column, its length k
    uint32_t rank, per_row; // the row first + i of the shape holds the document sorted_doc[rank + i * per_row] here
};

YB_HD uint32_t fit_digit(uint32_t key, uint32_t pass) { return (key >> (8u * pass)) & 0xFFu; }

// radix passes the keys 0 .. max_key need (max_key >= 1)
YB_HD uint32_t fit_sort_passes(uint32_t max_key) { return max_key < (1u << 8) ? 1u : max_key < (1u << 16) ? 2u : max_key < (1u << 24) ? 3u : 4u; }

// Rule 6.  The last place p in [lo, hi] with pl[p - org].col <= col (pl[lo - org].col <= col is the caller's promise: the
// first place of a shape starts at column 0).  org: the place pl[0] is (an LDS window).
YB_HD uint32_t fit_find_place(const FitPlace *pl, uint32_t org, uint32_t lo, uint32_t hi, uint32_t col) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (pl[mid - org].col <= col)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The plan as a slot sees it: the shapes [s_org, ...) and the places [p_org, ...) of the whole plan or of a window of it.
struct FitView {
    const unsigned long long *first;    // first[s - s_org]: the first row of shape s; the entry behind the last shape: n_rows
    const uint32_t *place;              // place[s - s_org]: the first place of shape s; the entry behind the last shape: n_places
    const FitPlace *pl;                 // pl[p - p_org]
    uint32_t s_org, p_org;
};

// Slot (row, col), the row being one of the shapes [s_lo, s_hi]: *shape = the row's shape; returns the place the slot lies in
// or FIT_PAD; *end = the first column behind the slots of this row that resolve as this one does (the end of the place, or C);
// *used = the filled slots of the row.
YB_HD uint32_t fit_slot(const FitView &V, uint32_t s_lo, uint32_t s_hi, unsigned long long row, uint32_t col, uint32_t C, uint32_t *shape,
                        uint32_t *end, uint32_t *used) {
    const uint32_t s = lay_find_doc(V.first, V.s_org, s_lo, s_hi, row);
    const uint32_t p0 = V.place[s - V.s_org], p1 = V.place[s + 1 - V.s_org];
    const FitPlace last = V.pl[p1 - 1 - V.p_org];
    *shape = s;
    *used = last.col + last.len;
    if (col >= *used) {
        *end = C;
        return FIT_PAD;
    }
    const uint32_t p = fit_find_place(V.pl, V.p_org, p0, p1 - 1, col);
    const FitPlace q = V.pl[p - V.p_org];
    *end = q.col + q.len;
    return p;
}

// Rule 5 (host).  hist[k] for k in [0, C] (hist[0], the documents in no row, only moves the ranks) -> the flat plan.
struct FitPlan {
    std::vector<unsigned long long> first;  // n_shapes + 1: the first row of every shape, then n_rows
    std::vector<uint32_t> place;            // n_shapes + 1: the first place of every shape, then n_places
    std::vector<FitPlace> pl;               // the places, shape by shape, left to right
    unsigned long long n_rows = 0, steps = 0;
    uint32_t n_shapes() const { return (uint32_t)place.size() - 1; }
};

inline void fit_plan(const uint32_t *hist, uint32_t C, FitPlan *out) {
    using Shape = std::vector<std::pair<uint32_t, uint32_t>>;  // runs (k, t), k strictly descending
    // candidates by (room ascending, shape descending): rows of room 0 are never asked for, and wait in `done`
    std::map<uint32_t, std::map<Shape, unsigned long long, std::greater<Shape>>> open;
    std::map<Shape, unsigned long long, std::greater<Shape>> done;
    auto add = [&](const Shape &s, uint32_t room, unsigned long long m) {
        if (!m) return;
        if (room)
            open[room][s] += m;
        else
            done[s] += m;
    };
    unsigned long long steps = 0;
    for (uint32_t k = C; k >= 1; --k) {
        unsigned long long n = hist[k];
        while (n) {
            ++steps;
            auto it = open.lower_bound(k);
            if (it == open.end()) {
                const unsigned long long t = C / k;
                add(Shape(1, {k, (uint32_t)t}), (uint32_t)(C - t * k), n / t);
                if (n % t) add(Shape(1, {k, (uint32_t)(n % t)}), (uint32_t)(C - (n % t) * k), 1);
                break;
            }
            const uint32_t room = it->first;
            auto sit = it->second.begin();  // the greatest shape of this room
            const Shape s = sit->first;
            const unsigned long long m = sit->second, t = room / k, whole = m < n / t ? m : n / t;
            n -= whole * t;
            const unsigned long long part = whole < m && n ? 1 : 0;  // one more row takes the rest
            if (whole + part == m)
                it->second.erase(sit);
            else
                sit->second = m - whole - part;
            if (it->second.empty()) open.erase(it);
            Shape s2 = s;
            s2.push_back({k, (uint32_t)t});
            add(s2, (uint32_t)(room - t * k), whole);
            if (part) {
                s2.back().second = (uint32_t)n;
                add(s2, (uint32_t)(room - n * k), 1);
                n = 0;
            }
        }
    }
    for (auto &by_room : open)
        for (auto &e : by_room.second) done[e.first] += e.second;
    // flat arrays: the shapes in descending order; rank of a place = documents shorter than k + places of length k before it
    std::vector<unsigned long long> before((size_t)C + 2, 0);  // before[k]: documents with n_d < k, then the places of length k dealt
    for (uint32_t k = 1; k <= C + 1; ++k) before[k] = before[k - 1] + hist[k - 1];
    out->first.clear();
    out->place.clear();
    out->pl.clear();
    unsigned long long row = 0;
    for (auto &e : done) {
        out->first.push_back(row);
        out->place.push_back((uint32_t)out->pl.size());
        uint32_t col = 0;
        for (auto &run : e.first) {
            for (uint32_t j = 0; j < run.second; ++j, col += run.first)
                out->pl.push_back(FitPlace{col, run.first, (uint32_t)(before[run.first] + j), run.second});
            before[run.first] += e.second * run.second;
        }
        row += e.second;
    }
    out->first.push_back(row);
    out->place.push_back((uint32_t)out->pl.size());
    out->n_rows = row;
    out->steps = steps;
}
