// yabpe_span_kernels.h -- span corruption (T5 / UL2 style denoising) of ragged ids: inputs with one sentinel per removed run,
// targets that list the sentinels with the ids they stand for (rule in span_logic.h; contract: BBPETokenizer.corrupt_spans,
// yet_another_bpe/tokenizer.py).
//
// Every pass takes one thread per id and a workgroup per SPAN_BLOCK consecutive ids, and finds documents as k_mask does: two
// threads search the whole table for the documents of the workgroup's first and last id, every thread between those two.
// Passes (host orchestration: yabpe_span_corrupt in yabpe.hip):
//   flags     k_span_flags: per id a byte -- kept (before the cut), noise, run start -- and the run-start bit again as a byte
//             of its own for the scan.  A thread evaluates at most Lmax draws, nearest opener first, and leaves at the first
//             that reaches its unit; its predecessor's answer comes through LDS (the workgroup's first thread computes it).
//             Token mode stages no draws in LDS: the draws are a few multiplies each and no memory, and what a halo would
//             save is at most the Lmax - 1 draws of ids that no opener covers (not measured against this form).
//   run index exclusive_scan of the run-start bytes; k_span_place: a run's number is the scan's value at its id minus the value
//             at its document's first id.  Runs past the sentinel cap lose their bits; per id the slots it takes in the inputs
//             and the targets, the final sentinel charged to the document's last kept id.
//   positions exclusive_scan of both slot counts; k_span_offsets gathers in_off / tgt_off at the document starts.
//   write     k_span_write: every id stores itself and / or its sentinel.  The compaction is monotone: consecutive lanes
//             store to ascending, nearly consecutive slots.
// Counters (protected, noise, cut in the flags pass; runs past the cap in the place pass) as k_mask's: per wave by ballots,
// per workgroup through LDS, one atomic per counter and workgroup into one of MASK_SHARDS copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "span_logic.h"
#include "yabpe_mask_kernels.h"  // MASK_SHARDS, MASK_SHARD_STRIDE

namespace yb {

enum SpanCounter : uint32_t { SPAN_C_PROTECTED = 0, SPAN_C_NOISE = 1, SPAN_C_CUT = 2, SPAN_C_OVER = 3, SPAN_COUNTERS = 4 };

struct SpanParams {
    const uint32_t *ids;
    unsigned long long n_ids;
    const unsigned long long *doc_off;  // n_docs document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_docs;
    const uint32_t *words;              // per id: piece index | MASK_WORD_SPECIAL, or nullptr (nothing is protected)
    unsigned long long seed, first_doc;
    SpanRule rule;                      // (rule.len: device memory)
    unsigned long long max_doc_ids;     // 0: no cut
    const uint32_t *sentinels;          // device copy of the table
    unsigned long long K;               // runs of a document that get a sentinel
    uint32_t whole_word, final_sentinel;
    uint8_t *flags, *start;             // [n_ids] each
    unsigned long long *run;            // [n_ids + 1]: exclusive scan of start
    uint8_t *c_in, *c_tgt;              // [n_ids] each
    unsigned long long *in_pos, *tgt_pos;  // [n_ids + 1] each: exclusive scans of c_in / c_tgt
    unsigned long long *in_off, *tgt_off;  // [n_docs + 1] each
    uint32_t *out_in, *out_tgt;
    unsigned long long *counters;       // [MASK_SHARDS][MASK_SHARD_STRIDE], of each copy [SPAN_COUNTERS]
};

// the documents of the workgroup's first and last id -> s_doc[0..1] (ends with a barrier)
__device__ __forceinline__ void span_block_docs(const SpanParams &P, unsigned long long i0, uint32_t *s_doc) {
    if (threadIdx.x < 2) {
        const unsigned long long il = i0 + SPAN_BLOCK - 1 < P.n_ids ? i0 + SPAN_BLOCK - 1 : P.n_ids - 1;
        s_doc[threadIdx.x] = mask_doc_of(P.doc_off, threadIdx.x ? il : i0, 0, P.n_docs - 1);
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned long long span_doc_end(const SpanParams &P, uint32_t d) { return d + 1 < P.n_docs ? P.doc_off[d + 1] : P.n_ids; }

// counter `which` += the threads of the workgroup with hit set (every thread of the workgroup calls this; s_cnt: one word a wave)
__device__ __forceinline__ void span_count(const SpanParams &P, uint32_t which, bool hit, uint32_t *s_cnt) {
    constexpr int WAVES = SPAN_BLOCK / 64;
    const uint32_t n = (uint32_t)__popcll(__ballot(hit));
    __syncthreads();  // (the last call's readers are done with s_cnt)
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sum += s_cnt[w];
        if (sum) atomicAdd(&P.counters[(blockIdx.x % MASK_SHARDS) * MASK_SHARD_STRIDE + which], (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(SPAN_BLOCK) void k_span_flags(SpanParams P) {
    __shared__ uint32_t s_doc[2];
    __shared__ uint32_t s_cnt[SPAN_BLOCK / 64];
    __shared__ uint8_t s_noise[SPAN_BLOCK];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * SPAN_BLOCK, i = i0 + threadIdx.x;  // (i0 < n_ids: the grid)
    span_block_docs(P, i0, s_doc);
    const bool live = i < P.n_ids, whole_word = P.whole_word != 0;
    bool noise = false, kept = false, special = false;
    unsigned long long j = 0, kd = 0;
    if (live) {
        const uint32_t d = mask_doc_of(P.doc_off, i, s_doc[0], s_doc[1]);
        const uint32_t w = P.words ? P.words[i] : 0u;
        j = i - P.doc_off[d];
        kd = span_doc_key(P.seed, P.first_doc, d);
        special = (w & MASK_WORD_SPECIAL) != 0;
        kept = span_kept(j, P.max_doc_ids);
        noise = span_token_noise(kd, j, w, whole_word, P.rule);
    }
    s_noise[threadIdx.x] = noise ? 1 : 0;
    __syncthreads();
    if (live) {
        bool prev = false;
        if (j > 0 && kept && noise)  // (j > 0: id i - 1 is of the same document)
            prev = threadIdx.x ? s_noise[threadIdx.x - 1] != 0 : span_token_noise(kd, j - 1, P.words ? P.words[i - 1] : 0u, whole_word, P.rule);
        const uint8_t f = span_flags(kept, noise, j, prev);
        P.flags[i] = f;
        P.start[i] = (f & SPAN_F_START) ? 1 : 0;
    }
    span_count(P, SPAN_C_PROTECTED, live && special, s_cnt);
    span_count(P, SPAN_C_NOISE, live && kept && noise, s_cnt);
    span_count(P, SPAN_C_CUT, live && !kept, s_cnt);
}

__global__ __launch_bounds__(SPAN_BLOCK) void k_span_place(SpanParams P) {
    __shared__ uint32_t s_doc[2];
    __shared__ uint32_t s_cnt[SPAN_BLOCK / 64];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * SPAN_BLOCK, i = i0 + threadIdx.x;
    span_block_docs(P, i0, s_doc);
    bool over = false;
    if (i < P.n_ids) {
        const uint32_t d = mask_doc_of(P.doc_off, i, s_doc[0], s_doc[1]);
        const unsigned long long first = P.doc_off[d], j = i - first;
        const uint8_t f = P.flags[i];
        unsigned long long k = 0;
        if (f & SPAN_F_NOISE) k = P.run[i] + ((f & SPAN_F_START) ? 1 : 0) - 1 - P.run[first];  // (a noise id lies in a run: the sum is >= 1)
        const bool is_last = P.final_sentinel && (i + 1 == span_doc_end(P, d) || (P.max_doc_ids && j + 1 == P.max_doc_ids));
        uint8_t c_in, c_tgt;
        P.flags[i] = span_place(f, k, P.K, is_last, &c_in, &c_tgt, &over);
        P.c_in[i] = c_in;
        P.c_tgt[i] = c_tgt;
    }
    span_count(P, SPAN_C_OVER, over, s_cnt);
}

// in_off / tgt_off: the positions at the document starts, and the totals at [n_docs]
__global__ __launch_bounds__(SPAN_BLOCK) void k_span_offsets(SpanParams P) {
    const unsigned long long d = (unsigned long long)blockIdx.x * SPAN_BLOCK + threadIdx.x;
    if (d > P.n_docs) return;
    const unsigned long long p = d < P.n_docs ? P.doc_off[d] : P.n_ids;
    P.in_off[d] = P.in_pos[p];
    P.tgt_off[d] = P.tgt_pos[p];
}

__global__ __launch_bounds__(SPAN_BLOCK) void k_span_write(SpanParams P) {
    __shared__ uint32_t s_doc[2];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * SPAN_BLOCK, i = i0 + threadIdx.x;
    span_block_docs(P, i0, s_doc);
    if (i >= P.n_ids) return;
    const uint8_t f = P.flags[i];
    if (!(f & SPAN_F_KEPT)) return;
    unsigned long long k = 0, n_runs = 0;
    if (f & (SPAN_F_START | SPAN_F_LAST)) {  // (only these read their document's first id)
        const unsigned long long base = P.run[P.doc_off[mask_doc_of(P.doc_off, i, s_doc[0], s_doc[1])]];
        k = P.run[i] - base;          // START: the runs of the document before this one
        n_runs = P.run[i + 1] - base; // LAST: i is the last kept id, no run starts after it
    }
    span_write(f, P.ids[i], P.in_pos[i], P.tgt_pos[i], k, n_runs, P.K, P.sentinels, P.out_in, P.out_tgt);
}

}  // namespace yb
