// yabpe_fit_kernels.h -- whole documents packed into rows by best-fit decreasing (rules and plan: fit_logic.h; contract:
// BBPETokenizer.encode_batch_fit, yet_another_bpe/tokenizer.py).
//
// Passes (host orchestration: yabpe_layout_fit in yabpe.hip; between sort and write the host turns the histogram into the plan):
//   lengths   k_fit_lengths: one thread per document: its key n_d (the length of its sequence after the cut), the histogram of
//             the keys (integer atomics; a row of at most FIT_HIST_LDS - 1 slots: in LDS first, one global atomic per length a
//             workgroup saw) and the call's counters (lay_commit).
//   sort      the documents stably by key, LSD radix passes of 8 bits: k_fit_sort_count (digit counts per tile, digit-major),
//             exclusive_scan, k_fit_sort_scatter.  A tile is FIT_SORT_TILE keys in FIT_SORT_ITEMS steps of one key a thread; the
//             rank of a key among the equal digits of its tile is (the count of the steps before) + (the count of the waves
//             before in this step) + (the lanes below with the same digit: 8 ballots).  No atomic decides an order: the
//             counts of k_fit_sort_count are sums.
//   write     k_fit_write: k_lay_pack_write's shape.  A workgroup owns LAY_PIECE consecutive output slots, a thread 4 slots per
//             step and three 16-byte stores.  The shapes and places of the piece's rows are staged in LDS (19 KiB: as many
//             workgroups a CU as its 32 waves allow); a piece whose rows have more than FIT_STAGE_SHAPES shapes or
//             FIT_STAGE_PLACES places (rows of many tiny documents) searches the plan in global memory.  The thread that owns
//             column 0 of a row stores its `used`.
// No workgroup waits for another; every loop runs over a constant number of steps or a search in an array whose length is given.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_logic.h"
#include "yabpe_layout_kernels.h" // LayConst, lay_commit, lay_value, lay_store4, lay_row_col, LAY_PIECE

namespace yb {

constexpr int FIT_HIST_LDS = 4096;                 // histogram entries a workgroup keeps in LDS (16 KiB)
constexpr int FIT_SORT_ITEMS = 8;                  // keys per thread and radix pass
constexpr int FIT_SORT_TILE = BLOCK * FIT_SORT_ITEMS;
constexpr int FIT_STAGE_SHAPES = 256;              // shapes (2 KiB + 1 KiB) and ...
constexpr int FIT_STAGE_PLACES = 1024;             // ... places (16 KiB) the write stages in LDS
static_assert(BLOCK == 256, "a thread per radix digit");

struct FitLenParams {
    const unsigned long long *doc;  // n_docs document starts (ids), ascending, doc[0] = 0
    uint32_t n_docs;
    unsigned long long n_ids;
    uint32_t C, flags;              // C >= max(1, n_added)
    uint32_t *key;                  // out: n_d per document
    uint32_t *hist;                 // out (zeroed): C + 1 counts
    unsigned long long *counters;   // [0] longest sequence [1] truncated documents [2] ids dropped [3] slots kept
};

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void k_fit_lengths(FitLenParams P) {
    __shared__ uint32_t s_hist[LDS ? FIT_HIST_LDS : 1];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i <= P.C; i += BLOCK) s_hist[i] = 0;
        __syncthreads();
    }
    const unsigned long long d = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long v[4] = {0, 0, 0, 0}; // max, truncated, dropped, kept
    if (d < P.n_docs) {
        const unsigned long long a = P.doc[d], b = d + 1 < P.n_docs ? P.doc[d + 1] : P.n_ids;
        const unsigned long long seq = b - a + lay_n_added(P.flags), kept = lay_kept(b - a, P.C, P.flags);
        P.key[d] = (uint32_t)kept;
        atomicAdd(LDS ? &s_hist[kept] : &P.hist[kept], 1u);
        v[0] = seq;
        v[1] = seq > kept ? 1u : 0u;
        v[2] = seq - kept;
        v[3] = kept;
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i <= P.C; i += BLOCK)
            if (s_hist[i]) atomicAdd(&P.hist[i], s_hist[i]);
    }
    lay_commit<true>(v, P.counters);
}

// counts[g * n_tiles + tile] = the keys of the tile whose digit is g
__global__ __launch_bounds__(BLOCK) void k_fit_sort_count(const uint32_t *key, uint32_t n, uint32_t pass, uint32_t *counts, uint32_t n_tiles) {
    __shared__ uint32_t s_cnt[BLOCK];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * FIT_SORT_TILE + threadIdx.x;
#pragma unroll
    for (int s = 0; s < FIT_SORT_ITEMS; ++s) {
        const unsigned long long i = base + (unsigned long long)s * BLOCK;
        if (i < n) atomicAdd(&s_cnt[fit_digit(key[i], pass)], 1u);
    }
    __syncthreads();
    counts[(unsigned long long)threadIdx.x * n_tiles + blockIdx.x] = s_cnt[threadIdx.x];
}

struct FitScatterParams {
    const uint32_t *key_in;
    const uint32_t *val_in;             // NULL: the identity (the first pass)
    uint32_t n, pass;
    const unsigned long long *offs;     // the exclusive scan of k_fit_sort_count's counts
    uint32_t n_tiles;
    uint32_t *key_out, *val_out;
};

__global__ __launch_bounds__(BLOCK) void k_fit_sort_scatter(FitScatterParams P) {
    __shared__ uint32_t s_wave[WPB][BLOCK];     // this step: the keys of every digit in every wave
    __shared__ unsigned long long s_base[BLOCK]; // where the next key of every digit goes
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    s_base[threadIdx.x] = P.offs[(unsigned long long)threadIdx.x * P.n_tiles + blockIdx.x];
    for (int w = 0; w < WPB; ++w) s_wave[w][threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * FIT_SORT_TILE + threadIdx.x;
    for (int s = 0; s < FIT_SORT_ITEMS; ++s) {
        const unsigned long long i = base + (unsigned long long)s * BLOCK;
        const bool valid = i < P.n;
        const uint32_t key = valid ? P.key_in[i] : 0u, g = fit_digit(key, P.pass);
        unsigned long long same = __ballot(valid); // the lanes of this wave with the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (g >> b) & 1u;
            const unsigned long long has = __ballot(valid && bit);
            same &= bit ? has : ~has;
        }
        const uint32_t below = __popcll(same & ((1ull << lane) - 1));
        if (valid && below == 0) s_wave[wib][g] = __popcll(same);
        __syncthreads();
        if (valid) {
            unsigned long long o = s_base[g] + below;
            for (uint32_t w = 0; w < wib; ++w) o += s_wave[w][g];
            P.key_out[o] = key;
            P.val_out[o] = P.val_in ? P.val_in[i] : (uint32_t)i;
        }
        __syncthreads();
        unsigned long long step = 0;
        for (int w = 0; w < WPB; ++w) {
            step += s_wave[w][threadIdx.x];
            s_wave[w][threadIdx.x] = 0;
        }
        s_base[threadIdx.x] += step;
        __syncthreads();
    }
}

struct FitWriteParams {
    const uint32_t *ids;
    const unsigned long long *doc;      // n_docs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    const uint32_t *sorted_doc;         // the documents stably by n_d
    const unsigned long long *first;    // the plan (fit_logic.h): n_shapes + 1 first rows,
    const uint32_t *place;              // n_shapes + 1 first places,
    const FitPlace *pl;                 // the places
    uint32_t n_shapes;
    unsigned long long n_slots;         // n_rows * C >= 1
    uint32_t C, flags;
    LayConst K;
    uint32_t *out_ids, *out_doc, *out_pos, *out_used;
};

// The slots of one lane: V = the plan, or the window of it that holds the shapes [s0, s1] of the piece's rows.
__device__ __forceinline__ void fit_lane(const FitWriteParams &P, const FitView &V, uint32_t s0, uint32_t s1, unsigned long long g0,
                                         unsigned long long g1) {
    const bool narrow = P.n_slots <= 0xFFFFFFFFull; // (uniform: the 32-bit division then)
#pragma unroll
    for (int s = 0; s < LAY_VPT; ++s) {
        const unsigned long long g = g0 + ((unsigned long long)s * BLOCK + threadIdx.x) * 4;
        if (g >= g1) break;
        unsigned long long row;
        uint32_t col;
        lay_row_col(g, P.C, narrow, &row, &col);
        uint32_t vi[4] = {0, 0, 0, 0}, vd[4] = {0, 0, 0, 0}, vp[4] = {0, 0, 0, 0};
        uint32_t shape = s0, end = 0;               // col >= end: the slot is not resolved yet
        uint32_t d = LAY_NO_DOC, c0 = 0, len = 0;   // the place the slots lie in: its document, first column and length
        unsigned long long a = 0, n = 0;            // that document's first id and ids
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (g + k >= g1) break; // (the last vector of the output: slots that do not exist)
            if (col >= end) {       // the thread's first slot, or the place, the pad tail or the row ended
                uint32_t used;
                const uint32_t p = fit_slot(V, shape, s1, row, col, P.C, &shape, &end, &used);
                if (col == 0) P.out_used[row] = used;
                d = LAY_NO_DOC;
                if (p != FIT_PAD) {
                    const FitPlace q = V.pl[p - V.p_org];
                    d = P.sorted_doc[q.rank + (row - V.first[shape - V.s_org]) * q.per_row];
                    a = P.doc[d];
                    n = (d + 1 < P.n_docs ? P.doc[d + 1] : P.n_ids) - a;
                    c0 = q.col;
                    len = q.len;
                }
            }
            vi[k] = P.K.pad_id;
            vd[k] = d;
            if (d != LAY_NO_DOC) { // a row of len slots that the document's sequence fills (Rule 1)
                vi[k] = lay_value(P.ids, lay_pad_slot(a, n, len, P.flags, col - c0), P.K);
                vp[k] = col - c0;
            }
            if (++col == P.C) { // the next slot opens the next row
                col = 0;
                end = 0;
                ++row;
            }
        }
        lay_store4(P.out_ids, g, P.n_slots, vi);
        lay_store4(P.out_doc, g, P.n_slots, vd);
        lay_store4(P.out_pos, g, P.n_slots, vp);
    }
}

__global__ __launch_bounds__(BLOCK) void k_fit_write(FitWriteParams P) {
    __shared__ unsigned long long s_first[FIT_STAGE_SHAPES + 1];
    __shared__ uint32_t s_place[FIT_STAGE_SHAPES + 1];
    __shared__ FitPlace s_pl[FIT_STAGE_PLACES];
    __shared__ uint32_t s_s[2];
    const unsigned long long g0 = (unsigned long long)blockIdx.x * LAY_PIECE;
    const unsigned long long g1 = g0 + LAY_PIECE < P.n_slots ? g0 + LAY_PIECE : P.n_slots;
    if (threadIdx.x == 0) { // the shapes of the piece's first and last row
        s_s[0] = lay_find_doc(P.first, 0, 0, P.n_shapes - 1, g0 / P.C);
        s_s[1] = lay_find_doc(P.first, 0, s_s[0], P.n_shapes - 1, (g1 - 1) / P.C);
    }
    __syncthreads();
    const uint32_t s0 = s_s[0], s1 = s_s[1], p0 = P.place[s0], p1 = P.place[s1 + 1];
    if (s1 - s0 + 1 <= (uint32_t)FIT_STAGE_SHAPES && p1 - p0 <= (uint32_t)FIT_STAGE_PLACES) { // (uniform)
        for (uint32_t i = threadIdx.x; i < s1 - s0 + 2; i += BLOCK) {
            s_first[i] = P.first[s0 + i];
            s_place[i] = P.place[s0 + i];
        }
        for (uint32_t i = threadIdx.x; i < p1 - p0; i += BLOCK) s_pl[i] = P.pl[p0 + i];
        __syncthreads();
        fit_lane(P, FitView{s_first, s_place, s_pl, s0, p0}, s0, s1, g0, g1);
    } else {
        fit_lane(P, FitView{P.first, P.place, P.pl, 0, 0}, s0, s1, g0, g1);
    }
}

} // namespace yb
