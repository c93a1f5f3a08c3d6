// yabpe_replay_kernels.h -- loading words in the state a trained model's merges leave them in (rules in replay_logic.h).
//
// Passes (host orchestration: load_replay, load_tiles and load_long_words in yabpe.hip, after the optional pooling of equal words):
//   segment   k_replay_llen / exclusive_scan (scratch of the words of more than RP_SHORT bytes) -> k_replay_words: one wave
//             per pooled word -- its u16 tokens after the replay (written where its bytes start) and their number
//   place     exclusive_scan of the token counts: packed position of word w = its token offset + w (every earlier word
//             contributed its tokens + 1 SEP), which replaces the byte offsets k_load_words relies on
//   build     k_load_words_tok / k_long_lengths_tok / k_load_long_tok: the token forms of k_load_words / k_long_lengths /
//             k_load_long (tile stream, tile_len, tile_wbase, long-word buffer; a word is long by its TOKEN count)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "replay_logic.h"
#include "yabpe_encode_kernels.h" // wave_min_u64
#include "yabpe_kernels.h"

namespace yb {

// llen[w] = the word's length when it takes the sequential path (scratch per byte), else 0
__global__ void k_replay_llen(const unsigned long long *off, unsigned long long n, uint32_t *llen, uint32_t *too_long) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const unsigned long long L = off[w + 1] - off[w];
    if (L > 0xFFFFFFFFull) atomicExch(too_long, 1u);
    llen[w] = L > RP_SHORT ? (uint32_t)L : 0u;
}

struct ReplayWordsParams {
    const uint8_t *bytes;
    const unsigned long long *off;   // word offsets (absolute)
    unsigned long long off_base;     // off[0]
    unsigned long long n_words;
    const unsigned long long *lbase; // per word: first slot of its sequential-path scratch
    RpTable tab;
    uint32_t *wcnt;                  // out, per word: number of tokens
    uint16_t *wtok;                  // out: the tokens of word w at wtok[off[w] - off_base ...]
    uint32_t *ltok, *lnxt, *lprv;    // sequential-path scratch
    unsigned long long *lheap;
};

// One wave per pooled word.  Words of at most 64 bytes: lane p holds the token that starts at byte p (while one does) and
// the smallest rank >= t of the pair it begins; each step takes the smallest (rank, position) by a wave reduction, t becomes
// that rank, and only the merged lane and its left neighbour look the table up again (every other lane's rank is >= the
// new t, so it is still its pair's smallest).  Longer words: lane 0 runs the heap walk of replay_logic.h in global scratch.
__global__ __launch_bounds__(BLOCK) void k_replay_words(ReplayWordsParams P) {
    const int lane = threadIdx.x & 63;
    const unsigned long long wave0 = (unsigned long long)blockIdx.x * WPB + (threadIdx.x >> 6), waves = (unsigned long long)gridDim.x * WPB;
    for (unsigned long long w = wave0; w < P.n_words; w += waves) {
        const unsigned long long s = P.off[w];
        const uint32_t L = (uint32_t)(P.off[w + 1] - s);
        uint16_t *dst = P.wtok + (s - P.off_base);
        if (L > RP_SHORT) {
            if (lane == 0) {
                const unsigned long long lb = P.lbase[w];
                uint32_t *tok = P.ltok + lb;
                const uint32_t cnt = rp_walk_heap(P.bytes + s, L, P.tab, tok, P.lnxt + lb, P.lprv + lb, P.lheap + 3 * lb);
                for (uint32_t k = 0; k < cnt; ++k) dst[k] = (uint16_t)tok[k];
                P.wcnt[w] = cnt;
            }
            continue;
        }
        uint32_t tok = lane < (int)L ? P.bytes[s + lane] : 0u;
        bool alive = lane < (int)L, dirty = true;
        uint32_t rk = RP_NONE, res = 0, tmin = 0;
        unsigned long long am = __ballot(alive);
        while (true) {
            const unsigned long long above = am & ~((2ull << lane) - 1ull);
            const int nx = above ? __ffsll((long long)above) - 1 : -1;
            const uint32_t ntok = __shfl(tok, nx < 0 ? lane : nx);
            if (dirty) {
                rk = RP_NONE;
                if (alive && nx >= 0 && !rp_lookup(P.tab, tok, ntok, tmin, &rk, &res)) rk = RP_NONE;
                dirty = false;
            }
            const unsigned long long m = wave_min_u64(rp_lane_key(alive, rk, (uint32_t)lane));
            if (m == ~0ull) break;
            const int win = (int)(m & 63);
            tmin = (uint32_t)(m >> 6);
            const int right = __shfl(nx, win);
            const unsigned long long below = am & ((1ull << win) - 1ull);
            const int pv = below ? 63 - __clzll((long long)below) : -1;
            if (lane == win) {
                tok = res;
                dirty = true;
            }
            if (lane == right) alive = false;
            if (lane == pv) dirty = true;
            am &= ~(1ull << right);
        }
        if (alive) dst[__popcll(am & ((1ull << lane) - 1ull))] = (uint16_t)tok;
        if (lane == 0) P.wcnt[w] = (uint32_t)__popcll(am);
    }
}

// ---------------------------------------------------------------- token forms of the loaders (pooled layout only)
struct LoadTokParams {
    const uint16_t *wtok;
    const uint32_t *wcnt;
    const unsigned long long *tok_off; // exclusive scan of wcnt
    const unsigned long long *off;
    unsigned long long off_base;
    unsigned long long n_words;
    uint16_t *tiles;
    uint32_t *tile_len;
    uint32_t *tile_wbase;
    uint32_t *long_count;
    unsigned long long *long_total;
    uint32_t *long_word;
    uint32_t long_cap;
};

__global__ __launch_bounds__(BLOCK) void k_load_words_tok(LoadTokParams P) {
    const unsigned long long w = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (w >= P.n_words) return;
    const uint32_t L = P.wcnt[w];
    const unsigned long long pos = P.tok_off[w] + w; // packed position: every earlier word contributed its tokens + 1 SEP
    const unsigned long long tile = pos / SPAN;
    const uint32_t slot = (uint32_t)(pos - tile * SPAN);
    uint16_t *dst = P.tiles + tile * CAP + slot;
    atomicMin(&P.tile_wbase[tile], (uint32_t)w);
    if (L + 1 > (uint32_t)LMAX) {
        const uint32_t idx = atomicAdd(P.long_count, 1u);
        if (idx < P.long_cap) P.long_word[idx] = (uint32_t)w;
        atomicAdd(P.long_total, (unsigned long long)L);
        dst[0] = YB_SEP; // placeholder keeps word indices aligned
        atomicMax(&P.tile_len[tile], slot + 1);
        return;
    }
    const uint16_t *src = P.wtok + (P.off[w] - P.off_base);
    for (uint32_t j = 0; j < L; ++j) dst[j] = src[j];
    dst[L] = YB_SEP;
    atomicMax(&P.tile_len[tile], slot + L + 1);
}

__global__ void k_long_lengths_tok(const uint32_t *wcnt, const uint32_t *long_word, uint32_t n_long, uint32_t *out_len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_long) out_len[i] = wcnt[long_word[i]];
}

struct LoadLongTokParams {
    const uint16_t *wtok;
    const uint32_t *wcnt;
    const unsigned long long *off;
    unsigned long long off_base;
    const unsigned long long *wfreq64;
    const uint32_t *long_word;
    const unsigned long long *long_off;
    uint16_t *long_tok;
    uint32_t *long_len;
    uint32_t *long_freq;
    uint32_t n_long;
};

__global__ __launch_bounds__(BLOCK) void k_load_long_tok(LoadLongTokParams P) {
    const uint32_t i = blockIdx.x;
    if (i >= P.n_long) return;
    const uint32_t w = P.long_word[i];
    const uint32_t L = P.wcnt[w];
    const uint16_t *src = P.wtok + (P.off[w] - P.off_base);
    uint16_t *dst = P.long_tok + P.long_off[i];
    for (uint32_t j = threadIdx.x; j < L; j += BLOCK) dst[j] = src[j];
    if (threadIdx.x == 0) {
        P.long_len[i] = L;
        P.long_freq[i] = (uint32_t)P.wfreq64[w];
    }
}

// k_stream_checksum's fold over the long-word buffer (one thread per long word; debug only): a word is long by its token
// count at load, which differs between a job that started from bytes and one resumed from a model -- the checksum of the
// resident words must not.
struct LongChecksumParams {
    const uint16_t *long_tok;
    const unsigned long long *long_off;
    const uint32_t *long_len;
    const uint32_t *long_freq; // may be NULL (flat layout)
    uint32_t n_long;
    TokTable tt;
    unsigned long long *sum, *words, *tokens;
};

__global__ __launch_bounds__(BLOCK) void k_long_checksum(LongChecksumParams P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n_long) return;
    const uint16_t *t = P.long_tok + P.long_off[i];
    const uint32_t n = P.long_len[i];
    if (!n) return;
    unsigned long long h = 1469598103934665603ull;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t v = t[p];
        const uint8_t *pb = P.tt.pool + P.tt.off[v];
        for (uint32_t k = 0; k < P.tt.len[v]; ++k) { h ^= pb[k]; h *= 1099511628211ull; }
        h ^= 0x1ffull; h *= 1099511628211ull;
    }
    const unsigned long long f = P.long_freq ? P.long_freq[i] : 1ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    atomicAdd(P.sum, h * f);
    atomicAdd(P.words, f);
    atomicAdd(P.tokens, (unsigned long long)n * f);
}

} // namespace yb
