// yabpe_dropout_kernels.h -- BBPETokenizer.encode_dropout on the device (rules: encode_logic.h "BPE-dropout").
//
// Every occurrence of a word draws on its own, so nothing is pooled: the split and pretok passes of yabpe_encode, then
//   long      k_drop_long_list lists the pre-tokens of more than ENC_SHORT bytes and hands each its piece of the walk's
//             scratch; k_drop_long runs the sequential walk once per listed word (one lane each) and leaves its count and,
//             in its scratch, its tokens
//   count     k_drop_words<false>: per pre-token, the number of ids it becomes (long ones excepted: k_drop_long's)
//   emit      exclusive_scan -> id offsets; k_drop_words<true> merges again -- the draws are a pure function of (seed,
//             document, position, step) -- and writes the ids in place; k_drop_long_emit copies the long words' ids;
//             k_enc_docs: the per-document offsets
// k_drop_words: a wave takes 64 consecutive pre-tokens, one per lane for the bookkeeping (offsets, document, word key).
// Specials and one-byte words are done there.  Words of 2 .. DROP_PACK bytes are merged four at a time, each in a 16-lane
// group of its own with reductions that stay inside the group; words of up to ENC_SHORT bytes one at a time over the wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_logic.h"
#include "yabpe_encode_kernels.h"

namespace yb {

constexpr uint32_t DROP_PACK = 16;  // words of at most this many bytes share a wave, four at a time

struct DropParams {
    const uint8_t *text;
    const unsigned long long *off;        // pre-token offsets
    unsigned long long n_pre;
    const unsigned long long *doc_start;  // document starts (n_docs of them, ascending, the first one 0)
    uint32_t n_docs;
    uint32_t pack;                        // DROP_PACK, or 0: every word of up to ENC_SHORT bytes takes the whole wave
    const uint8_t *sflag;                 // nullptr without specials
    EncTable tab;
    const uint32_t *out_id;               // internal id -> output id
    const uint32_t *sp_id;
    const uint8_t *sp_has;
    unsigned long long seed, T;
    uint32_t *cnt;                        // per pre-token: number of ids (written by the count pass, read by the scan)
    const unsigned long long *id_off;     // emit pass: first id slot of every pre-token
    uint32_t *ids;                        // emit pass: out
    unsigned long long *sums;             // [0] specials met (count pass)
};

// last d in [lo, hi] with doc_start[d] <= pos
__device__ __forceinline__ uint32_t drop_doc_of(const unsigned long long *doc_start, unsigned long long pos, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (doc_start[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The word key of the pre-token at text offset s.  Empty documents share their start with the next one; the last of equal
// starts is the document the byte belongs to.
__device__ __forceinline__ unsigned long long drop_word_key(const unsigned long long *doc_start, unsigned long long seed, unsigned long long s,
                                                            uint32_t lo, uint32_t hi) {
    const uint32_t d = drop_doc_of(doc_start, s, lo, hi);
    return enc_drop_word_key(enc_drop_doc_key(seed, d), s - doc_start[d]);
}

// The lane form of k_enc_words with draws, in groups of G lanes (G = 16 or 64; every lane of the wave calls it together).
// The lanes of a group hold one word: L bytes from text + s (L = 0: the group idles), key kw.  Lane p of the group holds
// the token that starts at byte p while one does.  Every step each lane with a ranked pair draws for (t, p); a dropped lane
// passes ~0 into the group's min reduction; the winner merges and only it and its left neighbour look the table up again.
// A group without a survivor is finished and stays so (its t no longer moves, so its draws repeat); the loop ends when
// that holds for every group of the wave.  Returns the group's alive mask (bit p: a token starts at byte p); *tok_out = the
// lane's token.
template <int G>
__device__ __forceinline__ unsigned long long drop_merge_lanes(const uint8_t *text, unsigned long long s, uint32_t L, const EncTable &tab,
                                                               unsigned long long kw, unsigned long long T, uint32_t *tok_out) {
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << G) - 1ull;
    uint32_t tok = gl < (int)L ? text[s + gl] : 0u;
    bool alive = gl < (int)L, dirty = true;
    uint32_t rk = ENC_NONE, res = 0;
    unsigned long long am = (__ballot(alive) >> gbase) & gmask;
    unsigned long long draw = enc_drop_lane(kw, (uint32_t)gl); // + ENC_RND_S per merge performed
    while (true) {
        const unsigned long long above = am & ~((2ull << gl) - 1ull);
        const int nx = above ? __ffsll((long long)above) - 1 : -1;
        const uint32_t ntok = __shfl(tok, gbase + (nx < 0 ? gl : nx));
        if (dirty) {
            rk = ENC_NONE;
            if (alive && nx >= 0 && !enc_lookup(tab, tok, ntok, &rk, &res)) rk = ENC_NONE;
            dirty = false;
        }
        unsigned long long m = (alive && rk != ENC_NONE && !enc_dropped(draw, T)) ? (((unsigned long long)rk << 6) | (unsigned)gl) : ~0ull;
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(m, o);
            m = y < m ? y : m;
        }
        if (__all(m == ~0ull)) break;
        const bool go = m != ~0ull;            // (uniform over the group)
        const int win = go ? (int)(m & 63) : 0;
        const int right = __shfl(nx, gbase + win);
        if (go) {
            const unsigned long long below = am & ((1ull << win) - 1ull);
            const int pv = below ? 63 - __clzll((long long)below) : -1;
            if (gl == win) {
                tok = res;
                dirty = true;
            }
            if (gl == right) alive = false;
            if (gl == pv) dirty = true;
            am &= ~(1ull << right);
            draw += ENC_RND_S;
        }
    }
    *tok_out = tok;
    return am;
}

template <bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_drop_words(DropParams P) {
    const int lane = threadIdx.x & 63;
    const unsigned long long chunks = (P.n_pre + 63) / 64, waves = (unsigned long long)gridDim.x * WPB;
    unsigned long long specials = 0; // (lane 0's)
    for (unsigned long long ch = (unsigned long long)blockIdx.x * WPB + (threadIdx.x >> 6); ch < chunks; ch += waves) {
        const unsigned long long w = ch * 64 + lane;
        const bool valid = w < P.n_pre;
        const unsigned long long s = valid ? P.off[w] : 0ull;
        const uint32_t L = valid ? (uint32_t)(P.off[w + 1] - s) : 0u;
        const uint8_t sf = (valid && P.sflag) ? P.sflag[s] : 0;
        const unsigned long long base = (EMIT && valid) ? P.id_off[w] : 0ull;
        // one lane per pre-token: specials and single bytes
        if (valid && sf) {
            const uint32_t k = sf - 1u;
            if (EMIT) {
                if (P.sp_has[k]) P.ids[base] = P.sp_id[k];
            } else {
                P.cnt[w] = P.sp_has[k] ? 1u : 0u;
            }
        } else if (valid && L == 1) {
            if (EMIT) P.ids[base] = P.out_id[P.text[s]]; else P.cnt[w] = 1u;
        }
        if (!EMIT) specials += (unsigned long long)__popcll(__ballot(valid && sf));
        const bool merges = valid && !sf && L >= 2 && L <= ENC_SHORT;
        const bool packed = merges && L <= P.pack;
        unsigned long long mp = __ballot(packed), mw = __ballot(merges && !packed);
        if (!(mp | mw)) continue;
        // the word keys: the documents of the chunk's first and last pre-token bound every lane's search (nearly always equal)
        const unsigned long long s_first = __shfl(s, 0), s_last = __shfl(s, (int)((P.n_pre - ch * 64 < 64 ? P.n_pre - ch * 64 : 64) - 1));
        const uint32_t d_mine = lane < 2 ? drop_doc_of(P.doc_start, lane ? s_last : s_first, 0, P.n_docs - 1) : 0u;
        const uint32_t d_lo = __shfl(d_mine, 0), d_hi = __shfl(d_mine, 1);
        const unsigned long long kw = merges ? drop_word_key(P.doc_start, P.seed, s, d_lo, d_hi) : 0ull;
        while (mp) { // four packed words at a time: group g takes the g-th lowest set bit
            int src = -1;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int b = mp ? __ffsll((long long)mp) - 1 : -1;
                if (mp) mp &= mp - 1;
                if ((lane >> 4) == g) src = b;
            }
            const int from = src < 0 ? lane : src;
            const unsigned long long gs = __shfl(s, from), gk = __shfl(kw, from), gb = __shfl(base, from);
            const uint32_t fL = __shfl(L, from), gL = src < 0 ? 0u : fL;
            uint32_t tok = 0;
            const unsigned long long am = drop_merge_lanes<16>(P.text, gs, gL, P.tab, gk, P.T, &tok);
            const int gl = lane & 15;
            if (EMIT) {
                if (gL && ((am >> gl) & 1ull)) P.ids[gb + __popcll(am & ((1ull << gl) - 1ull))] = P.out_id[tok];
            } else if (gL && gl == 0) {
                P.cnt[ch * 64 + src] = (uint32_t)__popcll(am);
            }
        }
        while (mw) { // one word over the whole wave
            const int src = __ffsll((long long)mw) - 1;
            mw &= mw - 1;
            const unsigned long long gs = __shfl(s, src), gk = __shfl(kw, src), gb = __shfl(base, src);
            const uint32_t gL = __shfl(L, src);
            uint32_t tok = 0;
            const unsigned long long am = drop_merge_lanes<64>(P.text, gs, gL, P.tab, gk, P.T, &tok);
            if (EMIT) {
                if ((am >> lane) & 1ull) P.ids[gb + __popcll(am & ((1ull << lane) - 1ull))] = P.out_id[tok];
            } else if (lane == 0) {
                P.cnt[ch * 64 + src] = (uint32_t)__popcll(am);
            }
        }
    }
    if (!EMIT && lane == 0 && specials) atomicAdd(&P.sums[0], specials);
}

// The pre-tokens of more than ENC_SHORT bytes: llist[j] = the pre-token, lbase[j] = the first slot of its walk scratch.
// ctr[0] = the words listed, ctr[1] = the slots handed out.  (The order of the list is whatever the atomics make it; it
// decides where a word's scratch lies and nothing else.)  cap = entries of llist / lbase: n_bytes / (ENC_SHORT + 1) + 1.
__global__ void k_drop_long_list(const unsigned long long *off, unsigned long long n_pre, const uint8_t *sflag, unsigned long long cap,
                                 uint32_t *llist, unsigned long long *lbase, unsigned long long *ctr) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_pre) return;
    const unsigned long long s = off[w], L = off[w + 1] - s;
    if (L <= ENC_SHORT || (sflag && sflag[s])) return;
    const unsigned long long j = atomicAdd(&ctr[0], 1ull);
    if (j >= cap) return; // (cannot happen: the long words are disjoint pieces of the text)
    llist[j] = (uint32_t)w;
    lbase[j] = atomicAdd(&ctr[1], L);
}

struct DropLongParams {
    const uint8_t *text;
    const unsigned long long *off;
    const unsigned long long *doc_start;
    uint32_t n_docs;
    const uint32_t *llist;
    const unsigned long long *lbase;
    unsigned long long n_long;
    EncTable tab;
    unsigned long long seed, T;
    uint32_t *cnt;                 // out, per pre-token
    uint32_t *ltok, *lnxt, *lprv;  // the walk's scratch; ltok[lbase[j] ..] keeps word j's tokens (internal ids) for the emit
    unsigned long long *lheap;
};

__global__ void k_drop_long(DropLongParams P) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.n_long) return;
    const uint32_t w = P.llist[j];
    const unsigned long long s = P.off[w], lb = P.lbase[j];
    const uint32_t L = (uint32_t)(P.off[w + 1] - s);
    const unsigned long long kw = drop_word_key(P.doc_start, P.seed, s, 0, P.n_docs - 1);
    P.cnt[w] = enc_merge_heap_dropout(P.text + s, L, P.tab, kw, P.T, P.ltok + lb, P.lnxt + lb, P.lprv + lb, P.lheap + 3 * lb);
}

__global__ void k_drop_long_emit(const uint32_t *llist, const unsigned long long *lbase, unsigned long long n_long, const uint32_t *ltok,
                                 const unsigned long long *id_off, const uint32_t *out_id, uint32_t *ids) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_long) return;
    const uint32_t w = llist[j];
    const unsigned long long a = id_off[w], e = id_off[w + 1];
    const uint32_t *src = ltok + lbase[j];
    for (unsigned long long k = a; k < e; ++k) ids[k] = out_id[src[k - a]];
}

} // namespace yb
