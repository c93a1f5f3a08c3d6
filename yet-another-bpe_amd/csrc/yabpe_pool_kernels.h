// yabpe_pool_kernels.h -- the persistent word pool (yabpe_pool_add): words arrive call by call, each call's
// words are first pooled among themselves (pool_words, yabpe_aux_kernels.h) and only its UNIQUE words meet the pool here.
//   compact   k_pool_compact: ulist[u] = the word that represents call-unique word u
//   probe     k_pool_probe: every call-unique word looks itself up; nothing is written to the pool
//   append    k_pool_append: the found words add their counts, the new ones are appended and inserted
//   rehash    k_pool_rehash: the stored hashes into a larger slot array (the arena is not read)
// The rules (masked hash, home and next slot, match, growth) are pool_logic.h's, shared with tests/hostmodel/pool_model.cpp.
// A word of up to PL_WAVE_BYTES bytes is compared and copied by its own thread; a longer one by its whole wave, lane-strided
// (the wave takes its long words one after the other).  No kernel uses LDS or scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pool_logic.h"
#include "yabpe_kernels.h"

namespace yb {

struct PoolView {
    uint8_t *arena;
    unsigned long long *off, *count, *hash;  // per pool word: start in the arena (n + 1 entries), occurrences, masked hash
    uint32_t *slots;                         // open addressing: pool indices, PL_EMPTY = free
    unsigned long long slot_cap;             // a power of two
    uint32_t hash_bits;
};

// the call's words as pool_words left them
struct PoolCall {
    const uint8_t *bytes;                    // word w = bytes[off[w], off[w + 1])
    const unsigned long long *off;
    const unsigned long long *hash;          // k_word_hash of every word
    const unsigned long long *count;         // per representative: the call's occurrences of its byte string
    const uint32_t *ulist;                   // call-unique word u -> its representative
    unsigned long long n_unique;
};

__global__ void k_pool_compact(const uint32_t *flag, const unsigned long long *uidx, unsigned long long n, uint32_t *ulist) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n && flag[w]) ulist[uidx[w]] = (uint32_t)w;
}

// lane-strided compare of L bytes by a whole wave (all 64 lanes call it with the same arguments)
__device__ __forceinline__ bool pool_wave_equal(const uint8_t *a, const uint8_t *b, unsigned long long L, int lane) {
    for (unsigned long long base = 0; base < L; base += 64) {
        const unsigned long long i = base + lane;
        if (__any(i < L && a[i] != b[i])) return false;
    }
    return true;
}

struct PoolProbeParams {
    PoolCall call;
    PoolView pool;
    uint32_t *hit;     // per call-unique word: its pool index, PL_NEW or PL_DROP
    uint32_t *nflag;   // 1 if new
    uint32_t *nlen;    // its length if new, else 0
    uint32_t *too_long;  // set when a word has more than PL_MAX_WORD_BYTES bytes
};

// Whole waves run (no early return): the long words of a wave are taken by all of its lanes.  The pool is only read here --
// the inserts are k_pool_append's, a launch later -- so a probe never meets a half-written entry.
__global__ __launch_bounds__(BLOCK) void k_pool_probe(PoolProbeParams P) {
    const unsigned long long u = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const PoolView &V = P.pool;
    unsigned long long o0 = 0, L = 0, mh = 0;
    uint32_t res = PL_DROP;
    bool wide = false;
    if (u < P.call.n_unique) {
        const uint32_t w = P.call.ulist[u];
        o0 = P.call.off[w];
        L = P.call.off[w + 1] - o0;
        mh = pl_mask_hash(P.call.hash[w], V.hash_bits);
        if (L > PL_MAX_WORD_BYTES) {  // (the host fails the call; nothing of it reaches the pool)
            *P.too_long = 1u;
            L = 0;
        }
        wide = L > PL_WAVE_BYTES;
        if (L && !wide) {
            res = PL_NEW;
            for (unsigned long long s = pl_home(mh, V.slot_cap);; s = pl_next(s, V.slot_cap)) {
                const uint32_t cur = V.slots[s];
                if (cur == PL_EMPTY) break;
                const unsigned long long c0 = V.off[cur];
                if (pl_match(V.hash[cur], V.off[cur + 1] - c0, V.arena + c0, mh, L, P.call.bytes + o0)) {
                    res = cur;
                    break;
                }
            }
        }
    }
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int j = __ffsll((long long)todo) - 1;
        const unsigned long long jo = __shfl(o0, j), jL = __shfl(L, j), jh = __shfl(mh, j);
        uint32_t r = PL_NEW;
        for (unsigned long long s = pl_home(jh, V.slot_cap);; s = pl_next(s, V.slot_cap)) {
            const uint32_t cur = V.slots[s];  // (the same slot in every lane)
            if (cur == PL_EMPTY) break;
            const unsigned long long c0 = V.off[cur];
            if (pl_match_head(V.hash[cur], V.off[cur + 1] - c0, jh, jL) && pool_wave_equal(V.arena + c0, P.call.bytes + jo, jL, lane)) {
                r = cur;
                break;
            }
        }
        if (lane == j) res = r;
    }
    if (u < P.call.n_unique) {
        P.hit[u] = res;
        P.nflag[u] = res == PL_NEW ? 1u : 0u;
        P.nlen[u] = res == PL_NEW ? (uint32_t)L : 0u;
    }
}

struct PoolAppendParams {
    PoolCall call;
    PoolView pool;                     // (after the growth, if any)
    const uint32_t *hit;
    const unsigned long long *nidx;    // exclusive scans of nflag and nlen
    const unsigned long long *noff;
    unsigned long long n_unique0, n_bytes0;  // the pool before this call
    unsigned long long *dropped;       // the call's count of zero-length words
};

// Two call-unique words are different byte strings, so they never name the same pool word: a found word's count is added
// with a plain read-modify-write, no atomic.  The new words are different from each other and from everything in the pool,
// so each takes the first free slot of its chain by CAS without comparing anything.
__global__ __launch_bounds__(BLOCK) void k_pool_append(PoolAppendParams P) {
    const unsigned long long u = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const PoolView &V = P.pool;
    unsigned long long src = 0, dst = 0, L = 0;
    bool wide = false;
    if (u < P.call.n_unique) {
        const uint32_t w = P.call.ulist[u], h = P.hit[u];
        const unsigned long long c = P.call.count[w];
        if (h == PL_DROP) {
            *P.dropped = c;  // (equal words are one call-unique word: at most one thread comes here)
        } else if (h != PL_NEW) {
            V.count[h] += c;
        } else {
            const unsigned long long p = P.n_unique0 + P.nidx[u];
            const unsigned long long mh = pl_mask_hash(P.call.hash[w], V.hash_bits);
            src = P.call.off[w];
            L = P.call.off[w + 1] - src;
            dst = P.n_bytes0 + P.noff[u];
            V.off[p + 1] = dst + L;
            V.count[p] = c;
            V.hash[p] = mh;
            wide = L > PL_WAVE_BYTES;
            if (!wide)
                for (unsigned long long i = 0; i < L; ++i) V.arena[dst + i] = P.call.bytes[src + i];
            unsigned long long s = pl_home(mh, V.slot_cap);
            while (atomicCAS(&V.slots[s], PL_EMPTY, (uint32_t)p) != PL_EMPTY) s = pl_next(s, V.slot_cap);
        }
    }
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int j = __ffsll((long long)todo) - 1;
        const unsigned long long js = __shfl(src, j), jd = __shfl(dst, j), jL = __shfl(L, j);
        for (unsigned long long i = lane; i < jL; i += 64) V.arena[jd + i] = P.call.bytes[js + i];
    }
}

__global__ void k_pool_rehash(const unsigned long long *hash, unsigned long long n, uint32_t *slots, unsigned long long slot_cap) {
    const unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    unsigned long long s = pl_home(hash[p], slot_cap);
    while (atomicCAS(&slots[s], PL_EMPTY, (uint32_t)p) != PL_EMPTY) s = pl_next(s, slot_cap);
}

}  // namespace yb
