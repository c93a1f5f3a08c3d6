// yabpe_rep_kernels.h -- repetition signals of ragged ids: per document and per n-gram length the largest class of equal
// windows, the number of classes and the ids inside repeated windows (rule in rep_logic.h; contract:
// BBPETokenizer.repetition_stats, yet_another_bpe/tokenizer.py).  Host orchestration: yabpe_repetition in yabpe.hip.
//
//   k_rep_plan     one thread per document: the results of the document zeroed for every length; whether the short form takes
//                  it (0 < L <= the boundary), else its piece count at the smallest length (a piece: up to DUP_TILE consecutive
//                  window positions of one document; a longer length has fewer windows, and a piece without any leaves at
//                  once) and its tile count (a tile: up to DUP_TILE consecutive ids).  exclusive_scan over each gives the
//                  document of every workgroup of the kernels below.
//   k_rep_short    one workgroup of four waves per short document.  The ids go to LDS ONCE, padded to 2,048; the Horner prefix
//                  P over them is built ONCE (the affine scan of k_dup_insert: eight elements a thread, six shuffle steps, the
//                  four waves through LDS).  Then, for every requested n in turn: the first 2^lg slots of the LDS table are
//                  cleared, 2^lg the smallest power of two >= 2 x windows; lane l of round j inserts window j * 256 + l from the
//                  home slot of H = P[i + n] - P[i] * B^n: an empty slot is claimed with an LDS atomicCAS(EMPTY -> i << 12 | 1),
//                  a resident is compared with i id by id in LDS -- equal: LDS atomicAdd(slot, 1) bumps the count in the low
//                  bits, done; unequal: next slot.  The representative of a class never moves, so a comparison stays valid
//                  whatever the other threads do.  slot_of[i] stays in LDS as u16.  After a barrier thread t takes windows
//                  8 t .. 8 t + 7 into registers: the count behind each (top: their maximum), and "i + 1 if count >= 2, else 0",
//                  max-scanned serially, across the wave by shuffles and across the waves through LDS to "the last repeating
//                  window at or before i"; id i is covered iff that window starts less than n back.  The claims a thread won
//                  are the classes.  Three u32 stores a length; the ids come from HBM once for all lengths.
//                  LDS: ids 8 KiB + P 16 KiB + table 16 KiB + slot_of 4 KiB = 44.1 KiB: three workgroups a CU of 160 KiB.
//   k_rep_insert   the long form, per n: one workgroup per piece, staging and prefix as k_dup_insert; the table in HBM holds
//                  the GLOBAL position of a class's representative, the document mixed into the home slot, and a resident is
//                  equal only if it lies in the same document and its ids match (read straight from ids[]).  A parallel u32
//                  array holds the count: atomicAdd by the claimer and by every equal window.  slot_of[p] = the slot.
//   k_rep_mark     in a launch of its own, once the counts are final: one workgroup per tile.  Flags count >= 2 of the tile's
//                  windows and of the n positions in front of it, the max-scan of k_dup_mark, covered ids counted; top by one
//                  atomicMax, covered by one atomicAdd a tile; distinct: the windows that are their own class's
//                  representative (table[slot_of[p]] == p), one atomicAdd a tile.
//
// Hashing, equality, counting and compare-and-swap have no matrix instruction on gfx950 (MFMA multiplies and sums): VALU, LDS
// and LDS atomics in the short form, VALU and global atomics in the long one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rep_logic.h"
#include "yabpe_dup_kernels.h"

namespace yb {

static_assert(REP_DOC == BLOCK * DUP_ITEMS, "one Horner scan of 256 threads x 8 elements spans a short document");

struct RepParams {
    const uint32_t *ids;
    uint32_t n_ids;
    const unsigned long long *doc_off;    // n_docs document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_docs;
    uint32_t n_ngrams, boundary;          // documents of more than `boundary` ids take the long form
    uint32_t ngram[REP_MAX_NGRAMS];
    unsigned long long pow_n[REP_MAX_NGRAMS];  // B^ngram[k]
    uint32_t k;                           // the long form's launch: which length
    uint32_t slots_log2;                  // of the global table
    uint32_t *shorts, *pieces, *tiles;    // [n_docs] counts
    const unsigned long long *short_off, *piece_off, *tile_off;  // [n_docs + 1] their exclusive scans
    uint32_t *table, *count;              // [slots] representative positions, class counts
    uint32_t *slot_of;                    // [n_ids] (written at window positions of long documents only)
    uint32_t *top, *distinct, *covered;   // [n_docs][n_ngrams] the results
};

__device__ __forceinline__ uint32_t rep_doc_end(const RepParams &P, uint32_t d) { return (uint32_t)(d + 1 < P.n_docs ? P.doc_off[d + 1] : P.n_ids); }

__global__ __launch_bounds__(BLOCK) void k_rep_plan(RepParams P) {
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= P.n_docs) return;
    const unsigned long long L = rep_doc_end(P, d) - P.doc_off[d];
    const bool lng = rep_is_long(L, P.boundary);
    P.shorts[d] = L && !lng ? 1u : 0u;
    P.pieces[d] = lng ? (uint32_t)dup_tiles(dup_windows(L, P.ngram[0])) : 0u;
    P.tiles[d] = lng ? (uint32_t)dup_tiles(L) : 0u;
    for (uint32_t k = 0; k < P.n_ngrams; ++k) {
        const unsigned long long o = (unsigned long long)d * P.n_ngrams + k;
        P.top[o] = 0; P.distinct[o] = 0; P.covered[o] = 0;
    }
}

// The Horner prefix over s_ids[0 .. 2,047] into s_P[0 .. 2,048]: the affine scan of k_dup_insert, thread t spanning elements
// 8 t .. 8 t + 7.  Every thread of the workgroup calls it, s_ids complete behind a barrier; s_P is complete behind the next one.
__device__ __forceinline__ void rep_prefix(const uint32_t *s_ids, unsigned long long *s_P, unsigned long long *s_w) {
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t e0 = threadIdx.x * DUP_ITEMS;
    const uint4 a = *reinterpret_cast<const uint4 *>(s_ids + e0), b = *reinterpret_cast<const uint4 *>(s_ids + e0 + 4);
    const unsigned long long mv[DUP_ITEMS] = {dup_m(a.x), dup_m(a.y), dup_m(a.z), dup_m(a.w), dup_m(b.x), dup_m(b.y), dup_m(b.z), dup_m(b.w)};
    unsigned long long inc = 0;
#pragma unroll
    for (uint32_t k = 0; k < DUP_ITEMS; ++k) inc = inc * DUP_B + mv[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long u = __shfl_up(inc, 1u << k);
        if (lane >= (1u << k)) inc = u * dup_step_pow(k) + inc;
    }
    if (lane == 63) s_w[wave] = inc;
    unsigned long long x = __shfl_up(inc, 1);  // exclusive inside the wave
    if (lane == 0) x = 0;
    __syncthreads();
    unsigned long long carry = 0;
    for (uint32_t w = 0; w < wave; ++w) carry = carry * DUP_POW_WAVE + s_w[w];
    x += carry * dup_pow(dup_step_pow(0), lane);
    if (threadIdx.x == 0) s_P[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < DUP_ITEMS; ++k) {
        x = x * DUP_B + mv[k];
        s_P[e0 + k + 1] = x;
    }
}

// Inclusive max-scan of eight values a thread across the workgroup: v[] holds the thread's elements 8 t .. 8 t + 7 and leaves
// with the maximum of everything at or before each.  Every thread calls it (one barrier inside; s_w may be reused after the
// caller's next barrier).
__device__ __forceinline__ void rep_max_scan(uint32_t (&v)[DUP_ITEMS], uint32_t *s_w) {
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll
    for (uint32_t k = 1; k < DUP_ITEMS; ++k) v[k] = max(v[k], v[k - 1]);
    uint32_t inc = v[DUP_ITEMS - 1];
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc = max(inc, u);
    }
    if (lane == 63) s_w[wave] = inc;
    uint32_t x = __shfl_up(inc, 1);
    if (lane == 0) x = 0;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) x = max(x, s_w[w]);
#pragma unroll
    for (uint32_t k = 0; k < DUP_ITEMS; ++k) v[k] = max(v[k], x);
}

__device__ __forceinline__ uint32_t rep_wave_max(uint32_t x) {
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) x = max(x, (uint32_t)__shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ uint32_t rep_wave_sum(uint32_t x) {
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

enum { REP_R_TOP, REP_R_DISTINCT, REP_R_COVERED, REP_RESULTS };

__global__ __launch_bounds__(BLOCK) void k_rep_short(RepParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ids[REP_DOC];
    __shared__ unsigned long long s_P[REP_DOC + 1];
    __shared__ uint32_t s_tab[REP_SHORT_SLOTS];
    __shared__ uint16_t s_slot[REP_DOC];
    __shared__ unsigned long long s_w64[WPB];
    __shared__ uint32_t s_w[WPB], s_res[REP_RESULTS];
    const uint32_t d = mh_doc_of(P.short_off, blockIdx.x, P.n_docs);  // (blockIdx.x < the number of short documents: the grid)
    const uint32_t lo = (uint32_t)P.doc_off[d], L = rep_doc_end(P, d) - lo;  // (0 < L <= boundary <= REP_DOC: k_rep_plan)
    for (uint32_t i = threadIdx.x; i < REP_DOC; i += BLOCK) s_ids[i] = i < L ? P.ids[lo + i] : 0u;  // (padding: its P is never read)
    if (threadIdx.x < REP_RESULTS) s_res[threadIdx.x] = 0;
    __syncthreads();
    rep_prefix(s_ids, s_P, s_w64);
    const uint32_t lane = threadIdx.x & 63u, e0 = threadIdx.x * DUP_ITEMS;
    for (uint32_t k = 0; k < P.n_ngrams; ++k) {
        const uint32_t n = P.ngram[k];
        if (L < n) break;  // (ascending lengths: no windows from here on; the zeros of k_rep_plan stand)
        const uint32_t W = L - n + 1, lg = rep_short_slots_log2(W), n_slots = 1u << lg, mask = n_slots - 1;
        const unsigned long long pow_n = P.pow_n[k];
        for (uint32_t i = threadIdx.x; i < n_slots; i += BLOCK) s_tab[i] = REP_EMPTY;
        __syncthreads();  // (the first round: s_P is complete too)
        uint32_t claims = 0;
        for (uint32_t i = threadIdx.x; i < W; i += BLOCK) {
            uint32_t slot = dup_home(dup_window_hash(s_P[i], s_P[i + n], pow_n), lg), found = 0;
            for (uint32_t probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask) {  // (2 W <= slots: a free slot exists)
                uint32_t r = s_tab[slot];
                if (r == REP_EMPTY) {
                    r = atomicCAS(&s_tab[slot], REP_EMPTY, rep_pack(i, 1));
                    if (r == REP_EMPTY) {  // claimed: this window represents its class
                        ++claims;
                        found = slot;
                        break;
                    }
                }
                const uint32_t q = rep_pos(r);  // (q + n <= L: q starts a window.  q != i: only this thread inserts i)
                bool equal = true;
                for (uint32_t j = 0; j < n; ++j)
                    if (s_ids[q + j] != s_ids[i + j]) {
                        equal = false;
                        break;
                    }
                if (equal) {
                    atomicAdd(&s_tab[slot], 1u);
                    found = slot;
                    break;
                }
            }
            s_slot[i] = (uint16_t)found;
        }
        __syncthreads();
        // thread t: windows 8 t .. 8 t + 7
        uint32_t v[DUP_ITEMS], top = 0;
#pragma unroll
        for (uint32_t e = 0; e < DUP_ITEMS; ++e) {
            const uint32_t i = e0 + e, cnt = i < W ? rep_count(s_tab[s_slot[i]]) : 0u;
            top = max(top, cnt);
            v[e] = cnt >= 2 ? i + 1 : 0u;
        }
        rep_max_scan(v, s_w);
        uint32_t cov = 0;
#pragma unroll
        for (uint32_t e = 0; e < DUP_ITEMS; ++e) cov += e0 + e < L && rep_is_covered(v[e], e0 + e, n) ? 1u : 0u;
        top = rep_wave_max(top);
        claims = rep_wave_sum(claims);
        cov = rep_wave_sum(cov);
        if (lane == 0) {
            atomicMax(&s_res[REP_R_TOP], top);
            atomicAdd(&s_res[REP_R_DISTINCT], claims);
            atomicAdd(&s_res[REP_R_COVERED], cov);
        }
        __syncthreads();
        if (threadIdx.x < REP_RESULTS) {  // (the thread that reads a value is the one that clears it for the next length)
            const unsigned long long o = (unsigned long long)d * P.n_ngrams + k;
            uint32_t *out = threadIdx.x == REP_R_TOP ? P.top : threadIdx.x == REP_R_DISTINCT ? P.distinct : P.covered;
            out[o] = s_res[threadIdx.x];
            s_res[threadIdx.x] = 0;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_rep_insert(RepParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ids[2 * DUP_TILE];
    __shared__ unsigned long long s_P[2 * DUP_TILE + 1];
    __shared__ unsigned long long s_w64[WPB];
    const unsigned long long piece = blockIdx.x;  // (< the number of pieces: the grid)
    const uint32_t d = mh_doc_of(P.piece_off, piece, P.n_docs), n = P.ngram[P.k];
    const uint32_t lo = (uint32_t)P.doc_off[d], hi = rep_doc_end(P, d), W = (uint32_t)dup_windows(hi - lo, n);
    const uint32_t w0 = (uint32_t)(piece - P.piece_off[d]) * DUP_TILE;
    if (w0 >= W) return;  // (the pieces are counted at the smallest length: this one has fewer windows.  Uniform: before any barrier)
    const uint32_t cnt = W - w0 < DUP_TILE ? W - w0 : DUP_TILE, E = cnt + n - 1;  // (lo + w0 + E <= hi; E <= 1,087)
    const uint32_t base = lo + w0;
    for (uint32_t i = threadIdx.x; i < 2 * DUP_TILE; i += BLOCK) s_ids[i] = i < E ? P.ids[base + i] : 0u;
    __syncthreads();
    rep_prefix(s_ids, s_P, s_w64);
    __syncthreads();
    const uint32_t n_slots = 1u << P.slots_log2, mask = n_slots - 1;
    const unsigned long long pow_n = P.pow_n[P.k];
    for (uint32_t i = threadIdx.x; i < cnt; i += BLOCK) {
        const uint32_t p = base + i;
        uint32_t slot = rep_home(dup_window_hash(s_P[i], s_P[i + n], pow_n), d, P.slots_log2), found = REP_EMPTY;
        for (uint32_t probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask) {
            uint32_t r = dup_load(&P.table[slot]);
            if (r == REP_EMPTY) {
                r = atomicCAS(&P.table[slot], REP_EMPTY, p);
                if (r == REP_EMPTY) r = p;  // claimed
            }
            bool equal = r >= lo && r < hi;  // (another document's window is never equal.  r + n <= hi then: r starts a window)
            if (equal && r != p)
                for (uint32_t j = 0; j < n; ++j)
                    if (P.ids[r + j] != s_ids[i + j]) {
                        equal = false;
                        break;
                    }
            if (equal) {
                atomicAdd(&P.count[slot], 1u);
                found = slot;
                break;
            }
        }
        P.slot_of[p] = found;  // (REP_EMPTY only in a table without a free slot, which yabpe_repetition refuses)
    }
}

__global__ __launch_bounds__(BLOCK) void k_rep_mark(RepParams P) {
    __shared__ uint32_t s_w[WPB], s_res[REP_RESULTS];
    if (threadIdx.x < REP_RESULTS) s_res[threadIdx.x] = 0;  // (the barrier of the scan lies between this and the adds)
    const unsigned long long tile = blockIdx.x;  // (< the number of tiles: the grid)
    const uint32_t d = mh_doc_of(P.tile_off, tile, P.n_docs), n = P.ngram[P.k];
    const uint32_t lo = (uint32_t)P.doc_off[d], hi = rep_doc_end(P, d);
    const uint32_t t0 = (uint32_t)(tile - P.tile_off[d]) * DUP_TILE;  // the tile's first id inside the document (t0 < hi - lo)
    const uint32_t cnt = hi - lo - t0 < DUP_TILE ? hi - lo - t0 : DUP_TILE;
    const uint32_t halo = t0 ? n : 0u;  // (t0 >= DUP_TILE >= n when it is not 0)
    const uint32_t g0 = lo + t0 - halo, E = halo + cnt;  // positions g0 .. g0 + E - 1, E <= 1,088: thread t takes 8 t .. 8 t + 7
    const uint32_t lane = threadIdx.x & 63u, e0 = threadIdx.x * DUP_ITEMS;
    uint32_t v[DUP_ITEMS], top = 0, own = 0;
#pragma unroll
    for (uint32_t e = 0; e < DUP_ITEMS; ++e) {
        const uint32_t j = e0 + e, p = g0 + j;
        uint32_t c = 0;
        if (j < E && p + n <= hi) {
            const uint32_t slot = P.slot_of[p];
            if (slot != REP_EMPTY) {
                c = P.count[slot];
                if (j >= halo) {  // the tile's own windows
                    top = max(top, c);
                    own += P.table[slot] == p ? 1u : 0u;
                }
            }
        }
        v[e] = c >= 2 ? j + 1 : 0u;
    }
    rep_max_scan(v, s_w);
    uint32_t cov = 0;
#pragma unroll
    for (uint32_t e = 0; e < DUP_ITEMS; ++e) {
        const uint32_t j = e0 + e;
        cov += j >= halo && j < E && rep_is_covered(v[e], j, n) ? 1u : 0u;
    }
    top = rep_wave_max(top);
    own = rep_wave_sum(own);
    cov = rep_wave_sum(cov);
    if (lane == 0) {
        atomicMax(&s_res[REP_R_TOP], top);
        atomicAdd(&s_res[REP_R_DISTINCT], own);
        atomicAdd(&s_res[REP_R_COVERED], cov);
    }
    __syncthreads();
    const unsigned long long o = (unsigned long long)d * P.n_ngrams + P.k;
    if (threadIdx.x == REP_R_TOP && s_res[REP_R_TOP]) atomicMax(&P.top[o], s_res[REP_R_TOP]);
    if (threadIdx.x == REP_R_DISTINCT && s_res[REP_R_DISTINCT]) atomicAdd(&P.distinct[o], s_res[REP_R_DISTINCT]);
    if (threadIdx.x == REP_R_COVERED && s_res[REP_R_COVERED]) atomicAdd(&P.covered[o], s_res[REP_R_COVERED]);
}

}  // namespace yb
