// yabpe_minhash_kernels.h -- MinHash signatures and LSH band keys from ragged ids (rule in minhash_logic.h; contract:
// BBPETokenizer.minhash_tokens, yet_another_bpe/tokenizer.py).  Host orchestration: yabpe_minhash in yabpe.hip.
//
//   k_minhash_plan  one thread per document: its shingle count and its piece count (a piece: up to MH_TILE consecutive shingle
//                   positions of one document).  exclusive_scan over the piece counts gives every document's first piece.
//   k_minhash_fill  one thread per signature slot: 0xFFFFFFFF into the rows of the documents that are not exactly one piece --
//                   those without shingles keep it, those of several pieces are lowered by atomicMin.
//   k_minhash       one workgroup of four waves per piece.  The piece's ids and the n - 1 ids behind them are staged in LDS;
//                   every thread hashes the shingles at its positions and leaves the u32 hashes in LDS (4 KB a full piece, the
//                   count rounded up to a multiple of four by hashing position 0 again: a repeated shingle changes no minimum).
//                   Then the WAVE is the shingle group and the LANE owns the hash functions: lane l of every wave holds a_k,
//                   b_k and the running minimum of k = k0 + l and k0 + 64 + l in registers (derived from the seed in the
//                   kernel: no parameter table in memory), wave w walks the quads w, w + 4, ... of hashes -- one 128-bit LDS
//                   read at an address the whole wave shares (a broadcast, no bank conflict) feeds eight multiply-shift-min
//                   steps a lane.  Past 128 functions the workgroup passes over the hashes again for the next 128; a pass with
//                   64 functions or fewer left runs with one function a lane.  The four waves' minima meet in LDS; a document
//                   that is one piece stores its row with plain stores, a document of several pieces lowers it with atomicMin
//                   (min commutes: the result does not depend on the order the workgroups arrive in).
//   k_minhash_keys  one thread per (document, band), in a launch of its own once every row is complete.
//
// The alternative, 128 function lanes x 2 shingle groups with one function a lane, reads LDS twice as often: a wave as the
// shingle group keeps the broadcast read (all 64 lanes of a wave are in one group by construction) and lets one read serve two
// functions.  An integer multiply-add-shift-min has no matrix instruction on gfx950 (MFMA accumulates sums): this is VALU work.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minhash_logic.h"

namespace yb {

constexpr uint32_t MH_BLOCK = 256, MH_WAVES = MH_BLOCK / 64;
constexpr uint32_t MH_CHUNK = 128;  // hash functions of one pass over a piece's hashes: two a lane

struct MinhashParams {
    const uint32_t *ids;
    unsigned long long n_ids;
    const unsigned long long *doc_off;  // n_docs document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_docs;
    MinhashRule rule;
    unsigned long long *n_shingles;     // [n_docs]
    uint32_t *pieces;                   // [n_docs] piece counts
    const unsigned long long *piece_off;  // [n_docs + 1] their exclusive scan
    uint32_t *sig;                      // [n_docs][num_perm]
    unsigned long long *keys;           // [n_docs][bands], or nullptr
};

__device__ __forceinline__ unsigned long long mh_doc_len(const MinhashParams &P, uint32_t d) {
    return (d + 1 < P.n_docs ? P.doc_off[d + 1] : P.n_ids) - P.doc_off[d];
}

__global__ __launch_bounds__(MH_BLOCK) void k_minhash_plan(MinhashParams P) {
    const uint32_t d = blockIdx.x * MH_BLOCK + threadIdx.x;
    if (d >= P.n_docs) return;
    const unsigned long long S = mh_shingles(mh_doc_len(P, d), P.rule.ngram);
    P.n_shingles[d] = S;
    P.pieces[d] = (uint32_t)mh_pieces(S);
}

__global__ __launch_bounds__(MH_BLOCK) void k_minhash_fill(MinhashParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * MH_BLOCK + threadIdx.x;
    if (i >= (unsigned long long)P.n_docs * P.rule.num_perm) return;
    if (P.pieces[i / P.rule.num_perm] != 1) P.sig[i] = MH_EMPTY;
}

// One pass of a wave over its quads of hashes for F functions a lane (k0 + lane, k0 + 64 + lane); the minima go to s_min.
template <int F>
__device__ __forceinline__ void mh_pass(const uint32_t *s_h, uint32_t n_quads, uint32_t wave, uint32_t lane, unsigned long long seed, uint32_t k0,
                                        uint32_t K, uint32_t *s_min) {
    unsigned long long a[F], b[F];
    uint32_t mn[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const uint32_t k = k0 + f * 64 + lane;  // (past K: a function that gives 0xFFFFFFFF for every hash, never stored)
        a[f] = k < K ? mh_param_a(seed, k) : 0ull;
        b[f] = k < K ? mh_param_b(seed, k) : ~0ull;
        mn[f] = MH_EMPTY;
    }
    for (uint32_t q = wave; q < n_quads; q += MH_WAVES) {
        const uint4 h = *reinterpret_cast<const uint4 *>(s_h + 4 * q);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const uint32_t lo = min(mh_perm(a[f], b[f], h.x), mh_perm(a[f], b[f], h.y));
            const uint32_t hi = min(mh_perm(a[f], b[f], h.z), mh_perm(a[f], b[f], h.w));
            mn[f] = min(mn[f], min(lo, hi));
        }
    }
#pragma unroll
    for (int f = 0; f < F; ++f) s_min[wave * MH_CHUNK + f * 64 + lane] = mn[f];
}

__global__ __launch_bounds__(MH_BLOCK) void k_minhash(MinhashParams P) {
    __shared__ uint32_t s_ids[MH_TILE + MH_MAX_NGRAM - 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_h[MH_TILE];
    __shared__ uint32_t s_min[MH_WAVES * MH_CHUNK];
    const unsigned long long p = blockIdx.x;  // (p < the number of pieces: the grid)
    const uint32_t d = mh_doc_of(P.piece_off, p, P.n_docs);
    const unsigned long long L = mh_doc_len(P, d), S = mh_shingles(L, P.rule.ngram);
    const unsigned long long s0 = (p - P.piece_off[d]) * MH_TILE;  // the piece's first shingle position (s0 < S: d has this piece)
    const uint32_t m = mh_shingle_ids(L, P.rule.ngram), K = P.rule.num_perm;
    const uint32_t cnt = S - s0 < MH_TILE ? (uint32_t)(S - s0) : MH_TILE;
    // the ids of the piece: positions s0 .. s0 + cnt - 1 and the m - 1 ids behind the last one (s0 + cnt + m - 1 <= L)
    const uint32_t *src = P.ids + P.doc_off[d] + s0;
    for (uint32_t i = threadIdx.x; i < cnt + m - 1; i += MH_BLOCK) s_ids[i] = src[i];
    __syncthreads();
    const uint32_t padded = (cnt + 3u) & ~3u;
    const unsigned long long init = mh_hash_init(m);
    for (uint32_t i = threadIdx.x; i < padded; i += MH_BLOCK) {
        const uint32_t pos = i < cnt ? i : 0u;
        unsigned long long s = init;
        for (uint32_t j = 0; j < m; ++j) s = mh_hash_step(s, s_ids[pos + j]);
        s_h[i] = mh_hash_final(s);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool one_piece = S <= MH_TILE;
    uint32_t *row = P.sig + (unsigned long long)d * K;
    for (uint32_t k0 = 0; k0 < K; k0 += MH_CHUNK) {
        if (K - k0 > 64u) mh_pass<2>(s_h, padded / 4, wave, lane, P.rule.seed, k0, K, s_min);
        else mh_pass<1>(s_h, padded / 4, wave, lane, P.rule.seed, k0, K, s_min);
        __syncthreads();
        const uint32_t k = k0 + threadIdx.x;
        if (threadIdx.x < MH_CHUNK && k < K) {  // (a pass with one function a lane: K - k0 <= 64, so threadIdx.x < 64 here)
            uint32_t v = s_min[threadIdx.x];
#pragma unroll
            for (uint32_t w = 1; w < MH_WAVES; ++w) v = min(v, s_min[w * MH_CHUNK + threadIdx.x]);
            if (one_piece) row[k] = v;
            else atomicMin(&row[k], v);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MH_BLOCK) void k_minhash_keys(MinhashParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * MH_BLOCK + threadIdx.x;
    const uint32_t bands = P.rule.bands, r = P.rule.num_perm / bands;
    if (i >= (unsigned long long)P.n_docs * bands) return;
    const uint32_t band = (uint32_t)(i % bands);
    P.keys[i] = mh_band_key(P.sig + (i / bands) * P.rule.num_perm + (unsigned long long)band * r, band, r);
}

}  // namespace yb
