// yabpe_fitlab_kernels.h -- labelled sequences packed whole into rows: ids, labels, sequence, position, and the seams (rules:
// fit_logic.h, Rules 5 to 8; contract: BBPETokenizer.fit_labelled, yet_another_bpe/tokenizer.py).
//
// The lengths, the radix sort and the plan are yabpe_layout_fit's as they are (k_fit_lengths, fit_sort, fit_plan).  What is new is
// the write: k_fit_write resolves, for every thread and step, slot -> place -> sorted_doc -> the document's start -> its ids,
// three dependent global loads.  Two channels would double that chain, so here it is paid once per SEQUENCE:
//   places   k_fitl_places: one thread per placed sequence (record t of Rule 7).  It finds its shape by a search in the record
//            bases, reads its place and resolves sorted_doc[rank + i * per_row] and that sequence's start.  It writes the public
//            record (seq, col, len), the private resolved record (source start, first output slot) with its (len, seq), and per
//            row: row_first by the thread of the row's first place, used by the thread of its last place, labelled = 0.
//   write    k_fitl_write: a workgroup owns FITL_TILE consecutive output slots, a lane FITL_SLOTS consecutive ones.  One lookup
//            (row_first of the tile's first row, then a search by output slot among that row's records) finds the first record
//            that can reach into the tile.  The records that cover the tile are staged into LDS FITL_STAGE at a time, starts
//            relative to the tile (a tile of one-id sequences holds more records than one stage: rounds).  A lane finds the
//            record of its first slot by a search in LDS and walks on for the other three; whether a slot is a pad, the last slot
//            of its sequence (shifted form) or a masked first slot is decided in registers.  Ids and labels are loaded with one
//            16-byte load each where the four slots are one aligned source run, else with 4-byte loads that the wave's
//            neighbours share lines with; the label run starts one entry later in the shifted form.  Five 16-byte stores.  The
//            slots whose label is not `ignore` are counted per wave by ballots and added with one atomic per wave and row present
//            in it.
// No workgroup waits for another; every loop runs over a search in an array whose length is given, over the stages of one tile
// or over the rows one wave touches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_logic.h"

namespace yb {

struct FitlParams {
    const uint32_t *ids, *labels;        // the ragged sequences, 16-byte aligned
    const unsigned long long *seq_off;   // n_seqs starts, ascending, seq_off[0] = 0
    uint32_t n_seqs;
    unsigned long long n_ids;
    const uint32_t *sorted_seq;          // the sequences stably by n_s
    const unsigned long long *first;     // the plan (fit_logic.h): n_shapes + 1 first rows,
    const uint32_t *place;               // n_shapes + 1 first places,
    const FitPlace *pl;                  // the places,
    const uint32_t *base;                // n_shapes + 1 first records (Rule 7)
    uint32_t n_shapes, n_placed;
    unsigned long long n_rows, n_slots;  // n_slots = n_rows * C
    uint32_t C, flags, pad_id, ignore;
    FitlRec *rec;                        // [n_placed] resolved records
    uint2 *rec2;                         // [n_placed] (len, seq)
    uint32_t *placed;                    // out [n_placed][3]: (seq, col, len)
    uint32_t *row_first;                 // out [n_rows + 1]
    uint32_t *used, *labelled;           // out [n_rows] each
    uint32_t *out_ids, *out_labels, *out_seq, *out_pos;  // out [n_slots] each
};

__global__ __launch_bounds__(FITL_BLOCK) void k_fitl_places(FitlParams P) {
    const unsigned long long t64 = (unsigned long long)blockIdx.x * FITL_BLOCK + threadIdx.x;
    if (t64 == 0) P.row_first[P.n_rows] = P.n_placed;
    if (t64 >= P.n_placed) return;
    const uint32_t t = (uint32_t)t64;
    uint32_t i, j;
    const uint32_t s = fitl_find_record(P.base, P.place, P.n_shapes, t, &i, &j);
    const uint32_t p0 = P.place[s], p1 = P.place[s + 1];
    const FitPlace q = P.pl[p0 + j];
    const unsigned long long row = P.first[s] + i;
    const uint32_t seq = P.sorted_seq[q.rank + (unsigned long long)i * q.per_row];
    P.rec[t] = FitlRec{P.seq_off[seq], row * P.C + q.col};
    P.rec2[t] = make_uint2(q.len, seq);
    P.placed[3ull * t] = seq;
    P.placed[3ull * t + 1] = q.col;
    P.placed[3ull * t + 2] = q.len;
    if (j == 0) {
        P.row_first[row] = t;
        P.labelled[row] = 0;
    }
    if (p0 + j + 1 == p1) P.used[row] = q.col + q.len;
}

__device__ __forceinline__ uint32_t fitl_rel(unsigned long long o, unsigned long long tile0) {  // where o lies in the tile, clamped
    return o <= tile0 ? 0u : (o - tile0 < FITL_TILE ? (uint32_t)(o - tile0) : FITL_TILE);
}

__global__ __launch_bounds__(FITL_BLOCK) void k_fitl_write(FitlParams P) {
    __shared__ uint32_t s_start[FITL_STAGE + 1];  // of each staged record the slot of the tile it starts in; [FITL_STAGE]: where the next stage starts
    __shared__ uint32_t s_skip[FITL_STAGE];       // the ids of the record that lie before the tile
    __shared__ unsigned long long s_src[FITL_STAGE];
    __shared__ uint2 s_rec2[FITL_STAGE];
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x;
    const unsigned long long tile0 = (unsigned long long)blockIdx.x * FITL_TILE;  // (tile0 < n_slots: the grid)
    const uint32_t tile_n = P.n_slots - tile0 < FITL_TILE ? (uint32_t)(P.n_slots - tile0) : FITL_TILE;
    const unsigned long long row0 = tile0 / P.C;
    const uint32_t col0 = (uint32_t)(tile0 - row0 * P.C);
    if (tid == 0) {  // the last record of the tile's first row that starts at or before the tile (the row's first one does)
        uint32_t lo = P.row_first[row0], hi = P.row_first[row0 + 1] - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (P.rec[mid].at <= tile0) lo = mid; else hi = mid - 1;
        }
        s_first = lo;
    }
    __syncthreads();
    const uint32_t r_first = s_first, i0 = tid * FITL_SLOTS;
    uint32_t id[FITL_SLOTS], lab[FITL_SLOTS], seq[FITL_SLOTS], pos[FITL_SLOTS];
    unsigned long long g[FITL_SLOTS] = {0, 0, 0, 0};  // of a filled slot: where its id lies in ids
    uint32_t filled = 0, loads = 0;                   // a bit per slot: it holds an id; its label is an entry of labels
#pragma unroll
    for (uint32_t s = 0; s < FITL_SLOTS; ++s) id[s] = P.pad_id, lab[s] = P.ignore, seq[s] = FIT_PAD, pos[s] = 0;
    for (unsigned long long rb = r_first;; rb += FITL_STAGE) {
        {   // a stage: records [rb, rb + FITL_STAGE); past the last record everything starts at n_slots
            const unsigned long long r = rb + tid;
            FitlRec a{0, P.n_slots};
            if (r < P.n_placed) {
                a = P.rec[r];
                s_rec2[tid] = P.rec2[r];
            }
            s_start[tid] = fitl_rel(a.at, tile0);
            s_skip[tid] = a.at < tile0 ? (uint32_t)(tile0 - a.at) : 0u;
            s_src[tid] = a.src;
            if (tid == 0) s_start[FITL_STAGE] = fitl_rel(rb + FITL_STAGE < P.n_placed ? P.rec[rb + FITL_STAGE].at : P.n_slots, tile0);
        }
        __syncthreads();
        const uint32_t from = s_start[0], to = s_start[FITL_STAGE];  // the slots this stage covers (pads behind its records included)
        uint32_t j = 0;
        bool have = false;
#pragma unroll
        for (uint32_t s = 0; s < FITL_SLOTS; ++s) {
            const uint32_t i = i0 + s;
            if (i < from || i >= to) continue;
            if (!have || s_start[j + 1] <= i) {  // the last staged record that starts at or before slot i
                uint32_t lo = have ? j + 1 : 0, hi = FITL_STAGE - 1;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo + 1) / 2;
                    if (s_start[mid] <= i) lo = mid; else hi = mid - 1;
                }
                j = lo;
                have = true;
            }
            const uint2 b = s_rec2[j];                       // (len, seq)
            const uint32_t p = i - s_start[j] + s_skip[j];  // the position inside the sequence, or past it: a pad
            if (p >= b.x) continue;
            uint32_t l;
            seq[s] = b.y;
            pos[s] = p;
            g[s] = s_src[j] + p;
            filled |= 1u << s;
            if (fitl_label(P.flags, p, b.x, &l)) loads |= 1u << s;
        }
        if (to >= tile_n) break;  // (the same for every thread)
        __syncthreads();
    }
    const uint32_t shift = (P.flags & FITL_SHIFTED) ? 1u : 0u;
    const bool run = g[1] == g[0] + 1 && g[2] == g[0] + 2 && g[3] == g[0] + 3;  // (read only with all four slots filled)
    if (filled == 0xFu && run && (g[0] & 3) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.ids + g[0]);
        id[0] = v.x, id[1] = v.y, id[2] = v.z, id[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t s = 0; s < FITL_SLOTS; ++s)
            if (filled >> s & 1u) id[s] = P.ids[g[s]];
    }
    if (loads == 0xFu && run && ((g[0] + shift) & 3) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.labels + g[0] + shift);
        lab[0] = v.x, lab[1] = v.y, lab[2] = v.z, lab[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t s = 0; s < FITL_SLOTS; ++s)
            if (loads >> s & 1u) lab[s] = P.labels[g[s] + shift];
    }
    if (i0 + FITL_SLOTS <= tile_n) {
        *reinterpret_cast<uint4 *>(P.out_ids + tile0 + i0) = make_uint4(id[0], id[1], id[2], id[3]);
        *reinterpret_cast<uint4 *>(P.out_labels + tile0 + i0) = make_uint4(lab[0], lab[1], lab[2], lab[3]);
        *reinterpret_cast<uint4 *>(P.out_seq + tile0 + i0) = make_uint4(seq[0], seq[1], seq[2], seq[3]);
        *reinterpret_cast<uint4 *>(P.out_pos + tile0 + i0) = make_uint4(pos[0], pos[1], pos[2], pos[3]);
    } else {
#pragma unroll
        for (uint32_t s = 0; s < FITL_SLOTS; ++s)
            if (i0 + s < tile_n) {
                P.out_ids[tile0 + i0 + s] = id[s];
                P.out_labels[tile0 + i0 + s] = lab[s];
                P.out_seq[tile0 + i0 + s] = seq[s];
                P.out_pos[tile0 + i0 + s] = pos[s];
            }
    }
    // the labelled slots per row: the wave takes one row with such slots left at a time
    uint32_t open = 0, rrow[FITL_SLOTS];  // the slot's row, counted from the tile's first one
#pragma unroll
    for (uint32_t s = 0; s < FITL_SLOTS; ++s) {
        rrow[s] = (uint32_t)(((unsigned long long)col0 + i0 + s) / P.C);
        if ((loads >> s & 1u) && lab[s] != P.ignore) open |= 1u << s;
    }
    const uint32_t lane = tid & 63u;
    for (;;) {
        const unsigned long long any = __ballot(open != 0);
        if (!any) break;
        const int leader = __ffsll((long long)any) - 1;
        const uint32_t mine = (open & 1u) ? rrow[0] : (open & 2u) ? rrow[1] : (open & 4u) ? rrow[2] : rrow[3];
        const uint32_t r = __shfl(mine, leader);
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t s = 0; s < FITL_SLOTS; ++s)
            if ((open >> s & 1u) && rrow[s] == r) {
                ++cnt;
                open &= ~(1u << s);
            }
        const uint32_t total = __popcll(__ballot(cnt & 1u)) + 2 * __popcll(__ballot(cnt & 2u)) + 4 * __popcll(__ballot(cnt & 4u));
        if ((int)lane == leader) atomicAdd(&P.labelled[row0 + r], total);
    }
}

}  // namespace yb
