// yabpe_mask_kernels.h -- masked-language-model inputs and labels from ragged ids (rule in mask_logic.h; contract:
// BBPETokenizer.mask_tokens, yet_another_bpe/tokenizer.py).
//
// One pass (host orchestration: yabpe_mask in yabpe.hip):
//   k_mask    one thread per id, a workgroup per MASK_BLOCK consecutive ids.  Two threads find the documents of the workgroup's
//             first and last id in the whole table; every thread then searches between those two (nearly always the same
//             document: no search; hundreds of one-token documents in a workgroup: at most eight steps).  The thread draws
//             from (seed, first_doc + d, unit or index) alone and stores its input id and its label: no thread waits for
//             another, and nothing is counted per id in memory.  The four counters (protected, masked, random, kept) are
//             summed per wave by ballots, per workgroup through LDS, and committed with one atomic per counter and workgroup
//             -- into one of MASK_SHARDS copies of the counters, 128 bytes apart, which the host sums: a quarter of a million
//             workgroups adding to ONE word are served one after the other, and that queue, not memory, bounded the pass
//             (DESIGN.md (u)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mask_logic.h"

namespace yb {

constexpr uint32_t MASK_SHARDS = 64;        // copies of the counters (workgroup b adds to copy b % MASK_SHARDS)
constexpr uint32_t MASK_SHARD_STRIDE = 16;  // u64 between two copies: a 128-byte line each

struct MaskParams {
    const uint32_t *ids;
    unsigned long long n_ids;
    const unsigned long long *doc_off;  // n_docs document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_docs;
    const uint32_t *words;              // per id: piece index | MASK_WORD_SPECIAL, or nullptr (nothing is protected)
    unsigned long long seed, first_doc;
    MaskRule rule;
    uint32_t ignore, whole_word;
    uint32_t *out_ids, *out_labels;
    unsigned long long *counters;       // [MASK_SHARDS][MASK_SHARD_STRIDE], of each copy [MASK_KINDS]: protected, masked, random, kept
};

__global__ __launch_bounds__(MASK_BLOCK) void k_mask(MaskParams P) {
    constexpr int WAVES = MASK_BLOCK / 64;
    __shared__ uint32_t s_doc[2];
    __shared__ uint32_t s_cnt[WAVES][MASK_KINDS];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * MASK_BLOCK, i = i0 + threadIdx.x;  // (i0 < n_ids: the grid)
    if (threadIdx.x < 2) {
        const unsigned long long il = i0 + MASK_BLOCK - 1 < P.n_ids ? i0 + MASK_BLOCK - 1 : P.n_ids - 1;
        s_doc[threadIdx.x] = mask_doc_of(P.doc_off, threadIdx.x ? il : i0, 0, P.n_docs - 1);
    }
    __syncthreads();
    uint32_t kind = MASK_UNSELECTED;
    if (i < P.n_ids) {
        const uint32_t d = mask_doc_of(P.doc_off, i, s_doc[0], s_doc[1]);
        uint32_t new_id, label;
        kind = mask_token(P.seed, P.first_doc, d, i - P.doc_off[d], P.words ? P.words[i] : 0u, P.whole_word != 0, P.rule, P.ignore, P.ids[i], &new_id,
                          &label);
        P.out_ids[i] = new_id;
        P.out_labels[i] = label;
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < MASK_KINDS; ++k) {
        const uint32_t n = (uint32_t)__popcll(__ballot(kind == k));
        if (lane == 0) s_cnt[wib][k] = n;
    }
    __syncthreads();
    if (threadIdx.x < MASK_KINDS) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) n += s_cnt[w][threadIdx.x];
        if (n) atomicAdd(&P.counters[(blockIdx.x % MASK_SHARDS) * MASK_SHARD_STRIDE + threadIdx.x], (unsigned long long)n);
    }
}

}  // namespace yb
