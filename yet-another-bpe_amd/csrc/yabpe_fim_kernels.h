// yabpe_fim_kernels.h -- fill-in-the-middle batches: a document cut into prefix, middle and suffix and written as
// "pre P suf S mid M [eot]" (PSM) or "pre suf S mid P M [eot]" (SPM), with labels (rule in fim_logic.h; contract:
// BBPETokenizer.fim_tokens / fim_cuts, yet_another_bpe/tokenizer.py).
//
// Passes (host orchestration: yabpe_fim and yabpe_fim_cuts in yabpe.hip):
//   plan   k_fim_plan: one thread per DOCUMENT.  Mode and cut points (drawn at token level; with pieces the mode comes from
//          `cuts` and the cut points are the lengths of the three pieces), the cut to max_len, the kept lengths (info), where
//          the kept prefix and the suffix start (aux), and the length of the sequence.  One exclusive_scan over those
//          n_docs lengths gives the offsets: nothing is scanned per id.  The counters (PSM, SPM, truncated documents, ids
//          dropped) are summed per wave by shuffles and committed with one atomic per counter and wave into one of
//          MASK_SHARDS copies.
//   write  k_fim_write: one thread per OUTPUT SLOT, a workgroup per FIM_BLOCK consecutive slots.  Two threads find the
//          documents of the workgroup's first and last slot in the offsets, every thread searches between those two
//          (mask_doc_of, as k_mask does), reads its document's 24 bytes of plan and maps its slot to a sentinel or to one
//          source id by a handful of comparisons (fim_slot).  Consecutive lanes store consecutive slots and, inside a piece,
//          load consecutive ids.
//   cuts   k_enc_lead_count (yabpe_encode_kernels.h) and one scan give the lead-byte table of the text, one entry per
//          ENC_GRANULE bytes; k_fim_cuts: one thread per document counts its code points with two table reads (enc_lead),
//          draws, and finds the byte of its a-th and b-th code point by a search of the table plus at most one granule of
//          bytes (fim_select).  Nothing is linear in a document's length.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fim_logic.h"
#include "yabpe_mask_kernels.h"  // MASK_SHARDS, MASK_SHARD_STRIDE

namespace yb {

enum FimCounter : uint32_t { FIM_C_PSM = 0, FIM_C_SPM = 1, FIM_C_TRUNCATED = 2, FIM_C_DROPPED = 3, FIM_COUNTERS = 4 };

struct FimParams {
    const uint32_t *ids;
    unsigned long long n_ids;
    const unsigned long long *doc_off;  // n_in document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_in;                      // documents that came in: n_docs, with pieces 3 * n_docs
    uint32_t n_docs;                    // documents that go out
    const unsigned long long *cuts;     // with pieces: (mode, a, b) per document, only the mode is read; else nullptr
    unsigned long long seed, first_doc;
    FimRule rule;
    uint4 *info;                        // [n_docs]: (mode, p, m, s) after the cut
    uint2 *aux;                         // [n_docs]: (dp, b) of FimDoc
    unsigned long long *len;            // [n_docs]: slots of the sequence
    unsigned long long *out_off;        // [n_docs + 1]: exclusive scan of len
    unsigned long long n_out;
    uint32_t *out_ids, *out_labels;
    unsigned long long *counters;       // [MASK_SHARDS][MASK_SHARD_STRIDE], of each copy [FIM_COUNTERS]
};

__device__ __forceinline__ unsigned long long fim_in_start(const FimParams &P, unsigned long long k) { return k < P.n_in ? P.doc_off[k] : P.n_ids; }

__global__ __launch_bounds__(FIM_BLOCK) void k_fim_plan(FimParams P) {
    const unsigned long long d = (unsigned long long)blockIdx.x * FIM_BLOCK + threadIdx.x;
    unsigned long long cnt[FIM_COUNTERS] = {0, 0, 0, 0};
    if (d < P.n_docs) {
        const bool pieces = (P.rule.flags & FIM_PIECES) != 0;
        const unsigned long long k0 = pieces ? 3 * d : d, first = fim_in_start(P, k0), last = fim_in_start(P, k0 + (pieces ? 3 : 1));
        const unsigned long long n = last - first;
        uint32_t mode;
        unsigned long long a, b;
        if (pieces) {
            const unsigned long long mv = P.cuts[3 * d];
            mode = mv == FIM_PSM ? FIM_PSM : mv == FIM_SPM ? FIM_SPM : FIM_NONE;
            a = fim_in_start(P, k0 + 1) - first;
            b = fim_in_start(P, k0 + 2) - first;
        } else {
            const unsigned long long kd = fim_doc_key(P.seed, P.first_doc, d);
            mode = fim_mode(kd, P.rule.fim, P.rule.spm);
            fim_draw_cuts(kd, mode, n, &a, &b);
        }
        unsigned long long out_len, dropped;
        const FimDoc D = fim_plan(mode, n, a, b, P.rule, &out_len, &dropped);
        P.info[d] = make_uint4(D.mode, D.p, D.m, D.s);
        P.aux[d] = make_uint2(D.dp, D.b);
        P.len[d] = out_len;
        cnt[FIM_C_PSM] = mode == FIM_PSM;
        cnt[FIM_C_SPM] = mode == FIM_SPM;
        cnt[FIM_C_TRUNCATED] = dropped != 0;
        cnt[FIM_C_DROPPED] = dropped;
    }
#pragma unroll
    for (uint32_t k = 0; k < FIM_COUNTERS; ++k) {
        unsigned long long v = cnt[k];
#pragma unroll
        for (int sh = 32; sh; sh >>= 1) v += __shfl_down(v, sh);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(&P.counters[((blockIdx.x * (FIM_BLOCK / 64) + (threadIdx.x >> 6)) % MASK_SHARDS) * MASK_SHARD_STRIDE + k], v);
    }
}

__global__ __launch_bounds__(FIM_BLOCK) void k_fim_write(FimParams P) {
    __shared__ uint32_t s_doc[2];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * FIM_BLOCK, i = i0 + threadIdx.x;  // (i0 < n_out: the grid)
    if (threadIdx.x < 2) {
        const unsigned long long il = i0 + FIM_BLOCK - 1 < P.n_out ? i0 + FIM_BLOCK - 1 : P.n_out - 1;
        s_doc[threadIdx.x] = mask_doc_of(P.out_off, threadIdx.x ? il : i0, 0, P.n_docs - 1);
    }
    __syncthreads();
    if (i >= P.n_out) return;
    const uint32_t d = mask_doc_of(P.out_off, i, s_doc[0], s_doc[1]);
    const uint4 f = P.info[d];
    const uint2 x = P.aux[d];
    const FimDoc D{f.x, f.y, f.z, f.w, x.x, x.y};
    const unsigned long long first = P.doc_off[(P.rule.flags & FIM_PIECES) ? 3ull * d : (unsigned long long)d];
    uint32_t id, label;
    fim_write_slot(D, i - P.out_off[d], P.ids, first, P.rule, &id, &label);
    P.out_ids[i] = id;
    P.out_labels[i] = label;
}

struct FimCutParams {
    const uint8_t *text;                // 16-byte aligned
    unsigned long long n_bytes;
    const unsigned long long *doc_off;  // n_docs document starts (bytes), ascending
    uint32_t n_docs;
    const unsigned long long *table;    // lead-byte prefix, one entry per ENC_GRANULE bytes (+ the total)
    unsigned long long seed, first_doc, fim, spm;
    unsigned long long *piece_off, *cuts;  // [3 * n_docs] each
};

__global__ __launch_bounds__(FIM_BLOCK) void k_fim_cuts(FimCutParams P) {
    const unsigned long long d = (unsigned long long)blockIdx.x * FIM_BLOCK + threadIdx.x;
    if (d >= P.n_docs) return;
    const unsigned long long start = P.doc_off[d], end = d + 1 < P.n_docs ? P.doc_off[d + 1] : P.n_bytes;
    const unsigned long long ls = enc_lead(P.text, P.n_bytes, P.table, start), le = enc_lead(P.text, P.n_bytes, P.table, end);
    unsigned long long c3[3], p3[3];
    fim_doc_cuts(P.text, P.table, ENC_GRANULE, start, end, ls, le, fim_doc_key(P.seed, P.first_doc, d), P.fim, P.spm, c3, p3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P.cuts[3 * d + k] = c3[k];
        P.piece_off[3 * d + k] = p3[k];
    }
}

}  // namespace yb
