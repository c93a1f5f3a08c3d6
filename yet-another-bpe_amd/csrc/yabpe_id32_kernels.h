// yabpe_id32_kernels.h -- the u32-id merge loop for gfx950 (MI355X, CDNA4): DESIGN.md (r).
//
// Vocabularies past 65,534 tokens.  One layout (pooled words with weights), one form (one merge per launch); the u16 kernels
// of yabpe_kernels.h are untouched.  Shared with them: DevState, TokTable and the byte-string hashes, the per-position rules
// of tile_logic.h (instantiated with YbW32) and the eligibility rule of limit_logic.h.
//
//   token stream  u32 ids in tiles of CAP32 slots (2 KiB); one wave owns one tile at a time; words never straddle tiles,
//                 every word ends with SEP.  tile_len[t] = live slots, tile_wbase[t] = index of the tile's first word in wfreq.
//   pair table    open addressing, keys u64 (left << 24 | right; EMPTY = ~0), counts i64, device-scope atomics; a per-workgroup
//                 LDS hash aggregates the deltas first.
//   k32_apply     one merge: reads the live stream once, rewrites + compacts the tiles that hold a site, flushes the deltas.
//   k32_select    the next merge: exact (count, bytes(left), bytes(right)) maximum (trainer.py:246) over the table, stop rules,
//                 token creation / id reuse (trainer.py:298); the last workgroup (by ticket) commits.
// Every loop is bounded: probe sequences by max_probe (HALT_TABLE_FULL: the host grows the table and recounts), walks by the
// lengths they are given.  Nothing waits for another workgroup.
#pragma once
#include "yabpe_kernels.h"
#include "replay_logic.h"

namespace yb {

constexpr int CAP32 = 512;                 // u32 slots per tile (2 KiB)
constexpr int LMAX32 = 64;                 // the tile's word limit: longest word (tokens + SEP) kept in the tile stream
constexpr int SPAN32 = CAP32 - LMAX32 + 1; // packed positions owned by one tile when (re)tiling
constexpr int AGG32_N = 1024;              // LDS delta-aggregator entries per workgroup
constexpr int AGG32_PROBE = 8;
constexpr unsigned long long EMPTY32 = YbW32::EMPTY;
constexpr uint32_t SEL32_MAX_BLOCKS = 1024;

// Candidate list of the selection (the idea of cand_note / k_cand_rebuild at 64-bit keys): a threshold T, and the slots of
// all pairs whose count is >= T.  A count that an add takes from below T to T or above is listed by that add; a selection
// that finds no listed pair at T or above any more (the list drained) commits nothing, lowers T and has the next selection
// scan the whole table once, which lists as it scans.  Invariant while `valid`: every slot with a count >= T is listed.
struct Cand32 {
    long long T;
    uint32_t n, overflow; // entries appended (may pass the capacity: then overflow is set)
    uint32_t valid, pad;
    unsigned long long rebuilds, drains; // (statistics)
};
struct PairTable32 {
    unsigned long long *keys;
    unsigned long long *cnt;
    uint32_t mask;      // capacity - 1 (a power of two)
    uint32_t max_probe;
    unsigned long long *entries; // where successful inserts are counted
    Cand32 *cs;                  // main table of a large job only, else NULL
    uint32_t *cand_list;         // slots
    uint32_t cand_cap;
};
__device__ __forceinline__ void cand32_append(const PairTable32 &t, uint32_t s) {
    const uint32_t idx = atomicAdd(&t.cs->n, 1u);
    if (idx < t.cand_cap) t.cand_list[idx] = s; else t.cs->overflow = 1u;
}

// cnt[key] += d.  A key enters a table only here; with a maximum token length a pair over the limit never does (limit_logic.h).
__device__ __forceinline__ void gt32_add(const PairTable32 &t, DevState *st, unsigned long long key, long long d) {
    uint32_t s = yb_hash48(key) & t.mask;
    for (uint32_t probe = 0; probe < t.max_probe; ++probe) {
        unsigned long long k = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY32) {
            const uint32_t lim = st->max_token_bytes;
            if (lim != 0u) {
                const uint32_t *len = st->tok_len;
                if (!yb_pair_fits(len[YbW32::left(key)], len[YbW32::right(key)], lim)) return;
            }
            k = atomicCAS(&t.keys[s], EMPTY32, key);
            if (k == EMPTY32) {
                atomicAdd(t.entries, 1ull);
                k = key;
            }
        }
        if (k == key) {
            if (d > 0 && t.cs) { // adds to one address are totally ordered: exactly one of them sees the count cross T
                const long long old = (long long)atomicAdd(&t.cnt[s], (unsigned long long)d), T = t.cs->T;
                if (old < T && old + d >= T) cand32_append(t, s);
            } else {
                atomicAdd(&t.cnt[s], (unsigned long long)d);
            }
            return;
        }
        s = (s + 1) & t.mask;
    }
    atomicMax(&st->halt_req, (uint32_t)HALT_TABLE_FULL);
}

// count of a key, 0 when absent; *found says which
__device__ __forceinline__ long long gt32_lookup(const PairTable32 &t, unsigned long long key, bool *found) {
    uint32_t s = yb_hash48(key) & t.mask;
    *found = false;
    for (uint32_t probe = 0; probe < t.max_probe; ++probe) {
        const unsigned long long k = t.keys[s];
        if (k == key) {
            *found = true;
            return (long long)t.cnt[s];
        }
        if (k == EMPTY32) return 0;
        s = (s + 1) & t.mask;
    }
    return 0;
}

// ---------------------------------------------------------------- LDS aggregator (per workgroup), 64-bit keys
struct Agg32 {
    unsigned long long *keys;
    unsigned long long *vals;
};
__device__ __forceinline__ void agg32_init(Agg32 g) {
    for (int i = threadIdx.x; i < AGG32_N; i += BLOCK) {
        g.keys[i] = EMPTY32;
        g.vals[i] = 0ull;
    }
}
__device__ __forceinline__ void agg32_add(Agg32 g, const PairTable32 &t, DevState *st, unsigned long long key, long long d) {
    uint32_t s = (yb_hash48(key) >> 7) & (uint32_t)(AGG32_N - 1);
    for (int probe = 0; probe < AGG32_PROBE; ++probe) {
        unsigned long long k = g.keys[s];
        if (k == EMPTY32) {
            k = atomicCAS(&g.keys[s], EMPTY32, key);
            if (k == EMPTY32) k = key;
        }
        if (k == key) {
            atomicAdd(&g.vals[s], (unsigned long long)d);
            return;
        }
        s = (s + 1) & (uint32_t)(AGG32_N - 1);
    }
    gt32_add(t, st, key, d); // the aggregator is full around this key: straight to the table
}
__device__ __forceinline__ void agg32_flush(Agg32 g, const PairTable32 &t, DevState *st) {
    for (int i = threadIdx.x; i < AGG32_N; i += BLOCK) {
        const unsigned long long k = g.keys[i];
        const long long v = (long long)g.vals[i];
        if (k != EMPTY32 && v != 0) gt32_add(t, st, k, v);
    }
}

// ---------------------------------------------------------------- a staged tile
struct TokAt32 {
    const uint32_t *stg;
    __device__ __forceinline__ uint32_t operator()(int q) const { return stg[8 + q]; }
};

// stage the live slots of a tile into the wave's LDS area; PAD before, and behind up to the end of the last round + 8
__device__ __forceinline__ int stage_tile32(uint32_t *stg, const uint32_t *tiles, uint32_t tile, uint32_t len, int lane) {
    const int rounds = (int)((len + 63u) >> 6);
    const uint32_t *src = tiles + (size_t)tile * CAP32;
    for (int k = 0; k < rounds; ++k) {
        const uint32_t p = (uint32_t)(k * 64 + lane);
        stg[8 + p] = p < len ? src[p] : YbW32::PAD;
    }
    if (lane < 8) stg[8 + rounds * 64 + lane] = YbW32::PAD;
    return rounds;
}

// merge-site bitmasks of a staged tile (greedy left-to-right rule, trainer.py:276-285): mark_sites at u32 width
__device__ __forceinline__ unsigned long long mark_sites32(const uint32_t *stg, unsigned long long *mb, int rounds, uint32_t a, uint32_t b, int lane) {
    TokAt32 T{stg};
    unsigned long long any = 0;
    if (lane == 0) mb[0] = 0ull;
    int last_non = -1; // wave-uniform: last position < current round whose token is not a
    for (int k = 0; k < rounds; ++k) {
        const int p = k * 64 + lane;
        const uint32_t x = T(p);
        const bool isa = x == a;
        int q = p; // run start: p itself when a != b (the parity term of yb_is_site is then unused)
        unsigned long long non = 0;
        if (a == b) {
            non = __ballot(!isa);
            const unsigned long long low = non & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
            q = (low ? (k * 64 + 63 - __clzll((long long)low)) : last_non) + 1;
        }
        const unsigned long long m = __ballot(yb_is_site(x, T(p + 1), a, b, p, q));
        if (lane == 0) mb[1 + k] = m;
        any |= m;
        if (non) last_non = k * 64 + 63 - __clzll((long long)non);
    }
    if (lane == 0) mb[1 + rounds] = 0ull;
    return any;
}

struct Stream32 {
    uint32_t *tiles;
    uint32_t *tile_len;
    const uint32_t *tile_wbase;
    const uint32_t *wfreq;
    uint32_t n_tiles;
};
struct Long32 {
    uint32_t *tok;
    const unsigned long long *off;
    uint32_t *len;
    const uint32_t *freq;
    uint32_t n;
};

// ================================================================ k32_count: pair histogram of the whole tile stream
struct Count32Params {
    Stream32 s;
    PairTable32 table;
    DevState *st;
};
__global__ __launch_bounds__(BLOCK) void k32_count(Count32Params P) {
    __shared__ unsigned long long s_keys[AGG32_N];
    __shared__ unsigned long long s_vals[AGG32_N];
    __shared__ uint32_t s_stage[WPB][8 + CAP32 + 72];
    Agg32 agg{s_keys, s_vals};
    agg32_init(agg);
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *stg = s_stage[wib];
    if (lane < 8) stg[lane] = YbW32::PAD;
    __syncthreads();
    TokAt32 T{stg};
    const uint32_t stride = gridDim.x * WPB;
    for (uint32_t tile = blockIdx.x * WPB + wib; tile < P.s.n_tiles; tile += stride) {
        const uint32_t len = min(P.s.tile_len[tile], (uint32_t)CAP32);
        if (len < 2) continue;
        wave_sync();
        const int rounds = stage_tile32(stg, P.s.tiles, tile, len, lane);
        wave_sync();
        uint32_t sep_carry = P.s.tile_wbase[tile];
        for (int k = 0; k < rounds; ++k) {
            const int p = k * 64 + lane;
            const uint32_t x = T(p), y = T(p + 1);
            const unsigned long long sm = __ballot(x == YbW32::SEP);
            const uint32_t widx = sep_carry + bits_below_lane(sm);
            sep_carry += __popcll(sm);
            if (x < YbW32::PAD && y < YbW32::PAD) agg32_add(agg, P.table, P.st, YbW32::key(x, y), (long long)P.s.wfreq[widx]);
        }
    }
    __syncthreads();
    agg32_flush(agg, P.table, P.st);
}

// long words: one workgroup per word, the threads stride over its positions
struct CountLong32Params {
    Long32 l;
    PairTable32 table;
    DevState *st;
};
__global__ __launch_bounds__(BLOCK) void k32_count_long(CountLong32Params P) {
    const uint32_t w = blockIdx.x;
    if (w >= P.l.n) return;
    const uint32_t len = P.l.len[w];
    const uint32_t *tok = P.l.tok + P.l.off[w];
    const long long f = (long long)P.l.freq[w];
    for (uint32_t p = threadIdx.x; p + 1 < len; p += BLOCK) gt32_add(P.table, P.st, YbW32::key(tok[p], tok[p + 1]), f);
}

// ================================================================ k32_apply: one merge over the whole live stream
struct Apply32Params {
    Stream32 s;
    PairTable32 table;
    DevState *st;
    unsigned long long *rec_sites; // per merge of this call: sites merged (weights not applied)
    uint32_t rec_base;
};
__global__ __launch_bounds__(BLOCK) void k32_apply(Apply32Params P) {
    __shared__ unsigned long long s_keys[AGG32_N];
    __shared__ unsigned long long s_vals[AGG32_N];
    __shared__ uint32_t s_stage[WPB][8 + CAP32 + 72];
    __shared__ unsigned long long s_mb[WPB][CAP32 / 64 + 2];
    DevState *st = P.st;
    if ((st->done | st->halt) || !st->n_batch) return; // (n_batch: the selection in front of this pass committed a merge)
    const uint32_t a = st->a, b = st->b, c = st->c;
    Agg32 agg{s_keys, s_vals};
    agg32_init(agg);
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *stg = s_stage[wib];
    unsigned long long *mb = s_mb[wib];
    if (lane < 8) stg[lane] = YbW32::PAD;
    __syncthreads();
    TokAt32 T{stg};
    MrgAt M{mb};
    const unsigned long long kab = YbW32::key(a, b);
    uint32_t removed = 0; // wave-uniform
    const uint32_t stride = gridDim.x * WPB;
    for (uint32_t tile = blockIdx.x * WPB + wib; tile < P.s.n_tiles; tile += stride) {
        const uint32_t len = min(P.s.tile_len[tile], (uint32_t)CAP32);
        if (len < 3) continue; // (a site needs two tokens and the word's SEP)
        wave_sync();
        const int rounds = stage_tile32(stg, P.s.tiles, tile, len, lane);
        wave_sync();
        const unsigned long long any = mark_sites32(stg, mb, rounds, a, b, lane);
        if (!any) continue;
        wave_sync();
        uint32_t *dst = P.s.tiles + (size_t)tile * CAP32;
        uint32_t sep_carry = P.s.tile_wbase[tile];
        uint32_t out_n = 0;
        for (int k = 0; k < rounds; ++k) {
            const int p = k * 64 + lane;
            const uint32_t x = T(p);
            const unsigned long long sm = __ballot(x == YbW32::SEP);
            const uint32_t widx = sep_carry + bits_below_lane(sm);
            sep_carry += __popcll(sm);
            if (M(p)) {
                const long long w = (long long)P.s.wfreq[widx];
                YbDeltasT<YbW32> d;
                yb_site_deltas_w<YbW32>(p, a, b, c, T, M, d);
                agg32_add(agg, P.table, st, kab, -w);
                if (d.left) {
                    agg32_add(agg, P.table, st, d.lo, -w);
                    agg32_add(agg, P.table, st, d.ln, w);
                }
                if (d.right) {
                    agg32_add(agg, P.table, st, d.ro, -w);
                    agg32_add(agg, P.table, st, d.rn, w);
                }
            }
            uint32_t o = 0;
            const int keep = yb_keep_w<YbW32>(p, c, false, T, M, o);
            const unsigned long long km = __ballot(keep);
            if (keep) dst[out_n + bits_below_lane(km)] = o; // (out_n + rank <= p < CAP32: never past the tile)
            out_n += __popcll(km);
        }
        if (lane == 0) P.s.tile_len[tile] = out_n;
        removed += len - out_n;
    }
    __syncthreads();
    agg32_flush(agg, P.table, st);
    if (lane == 0 && removed) {
        atomicAdd(&st->sites, (unsigned long long)removed);
        atomicAdd(&P.rec_sites[st->iter - 1u - P.rec_base], (unsigned long long)removed);
    }
}

// long words: one lane per word, sequentially.  A word that holds a site gives up all its old pairs, is rewritten in place
// and adds all its new pairs (work in the word's length only when it holds a site).
struct ApplyLong32Params {
    Long32 l;
    PairTable32 table;
    DevState *st;
    unsigned long long *rec_sites;
    uint32_t rec_base;
};
__global__ __launch_bounds__(64) void k32_apply_long(ApplyLong32Params P) {
    DevState *st = P.st;
    if ((st->done | st->halt) || !st->n_batch) return;
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= P.l.n) return;
    const uint32_t a = st->a, b = st->b, c = st->c;
    const uint32_t len = P.l.len[w];
    uint32_t *tok = P.l.tok + P.l.off[w];
    bool any = false;
    for (uint32_t p = 0; p + 1 < len; ++p)
        if (tok[p] == a && tok[p + 1] == b) {
            any = true;
            break;
        }
    if (!any) return;
    const long long f = (long long)P.l.freq[w];
    for (uint32_t p = 0; p + 1 < len; ++p) gt32_add(P.table, st, YbW32::key(tok[p], tok[p + 1]), -f);
    uint32_t n = 0;
    for (uint32_t p = 0; p < len;) { // greedy from the left (n <= p: only positions already read are overwritten)
        if (p + 1 < len && tok[p] == a && tok[p + 1] == b) {
            tok[n++] = c;
            p += 2;
        } else {
            tok[n++] = tok[p++];
        }
    }
    P.l.len[w] = n;
    for (uint32_t p = 0; p + 1 < n; ++p) gt32_add(P.table, st, YbW32::key(tok[p], tok[p + 1]), f);
    atomicAdd(&st->sites, (unsigned long long)(len - n));
    atomicAdd(&P.rec_sites[st->iter - 1u - P.rec_base], (unsigned long long)(len - n));
}

// ================================================================ k32_select: the next merge
struct Best32 {
    long long cnt;           // <= 0: nothing
    unsigned long long key;
};
// Python bytes order of two tokens: unsigned bytewise, a proper prefix sorts lower
__device__ __forceinline__ int tok32_cmp(const TokTable &tt, uint32_t x, uint32_t y) {
    if (x == y) return 0;
    const uint8_t *px = tt.pool + tt.off[x], *py = tt.pool + tt.off[y];
    const uint32_t lx = tt.len[x], ly = tt.len[y];
    const uint32_t n = lx < ly ? lx : ly;
    for (uint32_t i = 0; i < n; ++i) {
        const int d = (int)px[i] - (int)py[i];
        if (d) return d;
    }
    return (lx > ly) - (lx < ly);
}
// x beats y in max(pair_counts, key=(count, bytes(left), bytes(right))) (trainer.py:246); equal byte strings mean equal ids
// (the vocabulary holds every byte string once), so the order is total
__device__ __forceinline__ bool best32_gt(const TokTable &tt, const Best32 &x, const Best32 &y) {
    if (x.cnt != y.cnt) return x.cnt > y.cnt;
    if (x.cnt <= 0 || x.key == y.key) return false;
    const int dl = tok32_cmp(tt, YbW32::left(x.key), YbW32::left(y.key));
    if (dl) return dl > 0;
    return tok32_cmp(tt, YbW32::right(x.key), YbW32::right(y.key)) > 0;
}

struct Select32Params {
    PairTable32 table;
    TokTable tt;
    DevState *st;
    Best32 *partials;  // one per workgroup
    uint32_t *ticket;
    uint32_t *rec_left, *rec_right, *rec_merged;
    unsigned long long *rec_count;
    uint32_t rec_base;
    uint32_t tok_cap;  // ids the token arrays hold
    uint32_t id_limit; // YbW32::MAX_TOKENS (lower in tests of the bound)
};

__device__ __forceinline__ Best32 best32_block_reduce(const TokTable &tt, Best32 v, Best32 *s_best) {
    s_best[threadIdx.x] = v;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const Best32 o = s_best[threadIdx.x + w];
            if (best32_gt(tt, o, s_best[threadIdx.x])) s_best[threadIdx.x] = o;
        }
        __syncthreads();
    }
    return s_best[0];
}

__global__ __launch_bounds__(BLOCK) void k32_select(Select32Params P) {
    __shared__ Best32 s_best[BLOCK];
    __shared__ uint32_t s_new[4]; // [0] write bytes, [1] c, [2] pool offset
    DevState *st = P.st;
    if (st->done | st->halt) return;
    // (1) this workgroup's share of the candidate list, or of the whole table (which lists as it goes when a list is kept)
    Best32 v{0, EMPTY32};
    const uint32_t cap = P.table.mask + 1u;
    Cand32 *cs = P.table.cs;
    const bool by_list = cs && cs->valid && !cs->overflow; // (the same in every workgroup: written by the last one of a launch only)
    const long long T = cs ? cs->T : 0;
    if (by_list) {
        const uint32_t n = min(cs->n, P.table.cand_cap);
        for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
            const uint32_t s = P.table.cand_list[i];
            if (s >= cap) continue;
            const long long cn = (long long)P.table.cnt[s];
            if (cn < T || cn <= 0) continue;
            const Best32 e{cn, P.table.keys[s]};
            if (best32_gt(P.tt, e, v)) v = e;
        }
    } else {
        for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < cap; s += gridDim.x * BLOCK) {
            const long long cn = (long long)P.table.cnt[s];
            if (cn <= 0) continue;
            if (cs && cn >= T) cand32_append(P.table, s);
            const Best32 e{cn, P.table.keys[s]};
            if (best32_gt(P.tt, e, v)) v = e;
        }
    }
    v = best32_block_reduce(P.tt, v, s_best);
    if (threadIdx.x == 0) {
        st_coherent(reinterpret_cast<unsigned long long *>(&P.partials[blockIdx.x].cnt), (unsigned long long)v.cnt);
        st_coherent(&P.partials[blockIdx.x].key, v.key);
    }
    if (!last_workgroup(P.ticket)) return; // (waits for the stores above; the whole workgroup calls it)
    // (2) the last workgroup: maximum over the partials, then the commit
    Best32 m{0, EMPTY32};
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += BLOCK) {
        const Best32 e{(long long)ld_coherent(reinterpret_cast<const unsigned long long *>(&P.partials[i].cnt)), ld_coherent(&P.partials[i].key)};
        if (best32_gt(P.tt, e, m)) m = e;
    }
    __syncthreads();
    m = best32_block_reduce(P.tt, m, s_best);
    if (threadIdx.x == 0) {
        s_new[0] = 0;
        st->n_batch = 0;
        const uint32_t hr = st->halt_req;
        bool drained = false;
        if (cs && hr == HALT_NONE) {
            if (by_list) {
                if (m.cnt < T && st->iter < st->num_merges) { // drained: nothing is committed; the next selection scans the table and lists at a lower T
                    drained = true;
                    cs->T = max(1ll, T - max(1ll, T / 4));
                    cs->n = 0;
                    cs->valid = 0;
                    cs->drains += 1;
                }
            } else { // a scan of the whole table: the list it made is good unless it overflowed or T lies above every count
                cs->rebuilds += 1;
                if (cs->overflow) {
                    cs->T = T + max(1ll, T / 4);
                    cs->n = 0;
                    cs->overflow = 0;
                    cs->valid = 0;
                } else if (m.cnt > 0 && m.cnt < T) {
                    cs->T = max(1ll, m.cnt - m.cnt / 4);
                    cs->n = 0;
                    cs->valid = 0;
                } else {
                    cs->valid = 1;
                }
            }
        }
        if (hr != HALT_NONE) { // raised by the apply pass before this selection: the table is not complete
            st->halt = hr;
        } else if (drained) {
        } else if (st->iter >= st->num_merges || m.cnt <= 0 || (unsigned long long)m.cnt < st->min_freq) {
            st->done = 1; // trainer.py:238, 242-243, 247-248
        } else {
            const uint32_t a = YbW32::left(m.key), b = YbW32::right(m.key);
            const uint32_t la = P.tt.len[a], lb = P.tt.len[b], lc = la + lb;
            const unsigned long long h = yb_hash_concat(P.tt.rec[a].hash, P.tt.rec[b].hash, lb);
            const uint8_t *pa = P.tt.pool + P.tt.off[a], *pb = P.tt.pool + P.tt.off[b];
            // "merged not in vocab" (trainer.py:298): the byte-string set, full compare where hash and length agree
            uint32_t s = yb_vset_home(h, lc) & P.tt.vset_mask, c = 0xFFFFFFFFu, free_slot = 0xFFFFFFFFu;
            for (uint32_t probe = 0; probe <= P.tt.vset_mask; ++probe) {
                const unsigned long long e = P.tt.vset[s];
                if (e == VSET_EMPTY) {
                    free_slot = s;
                    break;
                }
                if ((e >> 32) == (h >> 32)) {
                    const uint32_t t = (uint32_t)e;
                    if (P.tt.len[t] == lc) {
                        const uint8_t *pt = P.tt.pool + P.tt.off[t];
                        bool eq = true;
                        for (uint32_t i = 0; i < lc && eq; ++i) eq = pt[i] == (i < la ? pa[i] : pb[i - la]);
                        if (eq) {
                            c = t;
                            break;
                        }
                    }
                }
                s = (s + 1) & P.tt.vset_mask;
            }
            uint32_t is_new = 0, halt = HALT_NONE;
            if (c == 0xFFFFFFFFu) {
                const uint32_t nt = st->n_tokens, used = st->pool_used;
                if (nt >= P.id_limit || nt >= P.tok_cap || free_slot == 0xFFFFFFFFu)
                    halt = HALT_VOCAB_FULL;
                else if ((unsigned long long)used + ((lc + 3u) & ~3u) > (unsigned long long)P.tt.pool_cap)
                    halt = HALT_POOL_FULL;
                else {
                    c = nt;
                    is_new = 1;
                    P.tt.off[c] = used;
                    P.tt.len[c] = lc;
                    TokRec r;
                    r.rank = 0;
                    r.len = lc;
                    r.hash = h;
                    r.pre8 = 0;
                    r.pad = 0;
                    P.tt.rec[c] = r;
                    P.tt.vset[free_slot] = yb_vset_entry(c, h);
                    st->n_tokens = nt + 1;
                    st->pool_used = used + ((lc + 3u) & ~3u);
                    s_new[0] = 1;
                    s_new[1] = c;
                    s_new[2] = used;
                }
            }
            if (halt != HALT_NONE) {
                st->halt = halt;
            } else {
                const uint32_t r = st->iter - P.rec_base;
                P.rec_left[r] = a;
                P.rec_right[r] = b;
                P.rec_merged[r] = c;
                P.rec_count[r] = (unsigned long long)m.cnt;
                st->a = a;
                st->b = b;
                st->c = c;
                st->c_is_new = is_new;
                st->best_count = (unsigned long long)m.cnt;
                st->tokens_now -= st->sites;
                st->sites = 0;
                st->iter = st->iter + 1;
                st->n_batch = 1;
            }
        }
    }
    __syncthreads();
    if (s_new[0]) { // the new token's bytes
        const uint32_t c = s_new[1];
        const uint32_t a = st->a, b = st->b;
        const uint8_t *pa = P.tt.pool + P.tt.off[a], *pb = P.tt.pool + P.tt.off[b];
        const uint32_t la = P.tt.len[a], lc = la + P.tt.len[b];
        uint8_t *dst = P.tt.pool + s_new[2];
        for (uint32_t i = threadIdx.x; i < lc; i += BLOCK) dst[i] = i < la ? pa[i] : pb[i - la];
        (void)c;
    }
}

// ================================================================ table growth, verify
struct Rehash32Params {
    PairTable32 from, to;
    DevState *st;
};
__global__ __launch_bounds__(BLOCK) void k32_rehash(Rehash32Params P) {
    const uint32_t cap = P.from.mask + 1u;
    for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < cap; s += gridDim.x * BLOCK) {
        const unsigned long long k = P.from.keys[s];
        const long long cn = (long long)P.from.cnt[s];
        if (k != EMPTY32 && cn != 0) gt32_add(P.to, P.st, k, cn);
    }
}
// keys of x whose count differs from y's (both_ways = 0: only keys y does not hold at all)
struct Compare32Params {
    PairTable32 x, y;
    unsigned long long *mismatches;
    uint32_t only_absent;
};
__global__ __launch_bounds__(BLOCK) void k32_table_compare(Compare32Params P) {
    const uint32_t cap = P.x.mask + 1u;
    uint32_t bad = 0;
    for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < cap; s += gridDim.x * BLOCK) {
        const unsigned long long k = P.x.keys[s];
        if (k == EMPTY32) continue;
        const long long cx = (long long)P.x.cnt[s];
        bool found = false;
        const long long cy = gt32_lookup(P.y, k, &found);
        if (P.only_absent ? (!found && cx != 0) : (cx != cy)) ++bad;
    }
    if (bad) atomicAdd(P.mismatches, (unsigned long long)bad);
}
__global__ void k32_fill_u64(unsigned long long *p, unsigned long long n, unsigned long long v) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ __launch_bounds__(BLOCK) void k32_sum_len(const uint32_t *tile_len, uint32_t n, unsigned long long *out) {
    unsigned long long s = 0;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) s += tile_len[i];
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

// ================================================================ repack: the live slots packed again, word by word
// As at the load: with the live slots numbered end to end (base[t] = slots in front of tile t), a word goes to the tile its
// first slot's number / SPAN32 names, and the words of a tile lie end to end from slot 0.  Two passes over the old stream:
// the plan finds every new tile's first word (its packed start and its index in wfreq), the move copies.
struct Repack32Params {
    Stream32 s;                       // the old stream
    const unsigned long long *base;   // exclusive scan of tile_len
    unsigned long long *first_g;      // per new tile: packed start of its first word (~0: none)
    uint32_t *dst, *dst_len, *dst_wbase;
    uint32_t n_new;
};
template <bool MOVE>
__global__ __launch_bounds__(BLOCK) void k32_repack(Repack32Params P) {
    __shared__ uint32_t s_stage[WPB][8 + CAP32 + 72];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *stg = s_stage[wib];
    if (lane < 8) stg[lane] = YbW32::PAD;
    __syncthreads();
    TokAt32 T{stg};
    const uint32_t stride = gridDim.x * WPB;
    for (uint32_t tile = blockIdx.x * WPB + wib; tile < P.s.n_tiles; tile += stride) {
        const uint32_t len = min(P.s.tile_len[tile], (uint32_t)CAP32);
        if (len == 0) continue;
        wave_sync();
        const int rounds = stage_tile32(stg, P.s.tiles, tile, len, lane);
        wave_sync();
        const unsigned long long base = P.base[tile];
        uint32_t sep_carry = P.s.tile_wbase[tile];
        int last_sep = -1; // wave-uniform: last SEP in front of the current round
        for (int k = 0; k < rounds; ++k) {
            const int p = k * 64 + lane;
            const uint32_t x = T(p);
            const unsigned long long sm = __ballot(x == YbW32::SEP);
            const unsigned long long below = sm & lanemask_lt(lane);
            const int start = (below ? (k * 64 + 63 - __clzll((long long)below)) : last_sep) + 1; // first slot of p's word
            if ((uint32_t)p < len) {
                const unsigned long long nt = (base + (unsigned long long)start) / SPAN32;
                if (nt < P.n_new) {
                    if (!MOVE) {
                        if (p == start) {
                            atomicMin(&P.first_g[nt], base + (unsigned long long)p);
                            atomicMin(&P.dst_wbase[nt], sep_carry + bits_below_lane(sm));
                        }
                    } else {
                        const unsigned long long o = base + (unsigned long long)p - P.first_g[nt];
                        if (o < (unsigned long long)CAP32) { // (always: a tile's words start inside one span and are at most LMAX32 long)
                            P.dst[(size_t)nt * CAP32 + o] = x;
                            if (x == YbW32::SEP) atomicMax(&P.dst_len[nt], (uint32_t)o + 1u);
                        }
                    }
                }
            }
            sep_carry += __popcll(sm);
            if (sm) last_sep = k * 64 + 63 - __clzll((long long)sm);
        }
    }
}

// ================================================================ load: bytes + offsets -> pooled words of u32 ids -> tiles
// (the id-pair table of a resumed load at 64-bit keys: Rp32Table and rp32_lookup of replay_logic.h)
struct Words32Params {
    const uint8_t *bytes;
    const unsigned long long *off; // absolute
    unsigned long long off_base, n_words;
    uint32_t *wtok;                // word w's tokens start at off[w] - off_base
    uint32_t *wcnt;
    Rp32Table rp;
    uint32_t *too_long;            // raised when a word has 2^32 - 1 bytes or more
};
// One lane per word: bytes -> ids, then the per-word form of the replay (replay_logic.h): the leftmost adjacent pair whose
// smallest rank >= t is the minimum over the word merges, t follows.  At most len - 1 steps of one scan each.
__global__ __launch_bounds__(BLOCK) void k32_words(Words32Params P) {
    const unsigned long long w = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (w >= P.n_words) return;
    const unsigned long long o = P.off[w], e = P.off[w + 1];
    if (e - o >= 0xFFFFFFFFull) {
        atomicOr(P.too_long, 1u);
        P.wcnt[w] = 0;
        return;
    }
    uint32_t n = (uint32_t)(e - o);
    uint32_t *tok = P.wtok + (o - P.off_base);
    for (uint32_t i = 0; i < n; ++i) tok[i] = P.bytes[o + i];
    if (P.rp.n) {
        uint32_t tmin = 0;
        const uint32_t steps = n;
        for (uint32_t step = 0; step < steps && n > 1; ++step) {
            uint32_t best_r = 0xFFFFFFFFu, best_p = 0, best_m = 0;
            for (uint32_t p = 0; p + 1 < n; ++p) {
                uint32_t r = 0, m = 0;
                if (rp32_lookup(P.rp, tok[p], tok[p + 1], tmin, &r, &m) && r < best_r) {
                    best_r = r;
                    best_p = p;
                    best_m = m;
                }
            }
            if (best_r == 0xFFFFFFFFu) break;
            tmin = best_r;
            tok[best_p] = best_m;
            for (uint32_t p = best_p + 1; p + 1 < n; ++p) tok[p] = tok[p + 1];
            --n;
        }
    }
    P.wcnt[w] = n;
}

// per word: slots in the tile stream (tokens + SEP; 0 for long and for empty words), short / long flags, long length
struct Slots32Params {
    const uint32_t *wcnt;
    unsigned long long n_words;
    uint32_t *slots, *is_short, *is_long, *long_len;
};
__global__ __launch_bounds__(BLOCK) void k32_word_slots(Slots32Params P) {
    const unsigned long long w = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (w >= P.n_words) return;
    const uint32_t n = P.wcnt[w];
    const bool sh = n >= 1 && n + 1 <= (uint32_t)LMAX32, lg = n + 1 > (uint32_t)LMAX32;
    P.slots[w] = sh ? n + 1 : 0u;
    P.is_short[w] = sh ? 1u : 0u;
    P.is_long[w] = lg ? 1u : 0u;
    P.long_len[w] = lg ? n : 0u;
}

struct Tiles32Params {
    const uint32_t *wtok;
    const uint32_t *wcnt;
    const unsigned long long *off;
    unsigned long long off_base, n_words;
    const unsigned long long *pos;   // exclusive scan of slots, n_words + 1
    const unsigned long long *srank; // exclusive scan of is_short
    uint32_t *tiles, *tile_len, *tile_wbase;
    uint32_t n_tiles;
};
// first index in [0, n] whose pos is >= x (pos has n + 1 entries, ascending)
__device__ __forceinline__ unsigned long long lower_bound64(const unsigned long long *pos, unsigned long long n, unsigned long long x) {
    unsigned long long lo = 0, hi = n;
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// One workgroup per tile: tile t holds the words whose packed start lies in [t SPAN32, (t + 1) SPAN32), end to end from slot 0.
__global__ __launch_bounds__(BLOCK) void k32_build_tiles(Tiles32Params P) {
    const uint32_t t = blockIdx.x;
    if (t >= P.n_tiles) return;
    const unsigned long long wlo = lower_bound64(P.pos, P.n_words, (unsigned long long)t * SPAN32);
    const unsigned long long whi = lower_bound64(P.pos, P.n_words, (unsigned long long)(t + 1) * SPAN32);
    const unsigned long long p0 = P.pos[wlo], p1 = P.pos[whi];
    const uint32_t len = (uint32_t)min(p1 - p0, (unsigned long long)CAP32);
    for (uint32_t g = threadIdx.x; g < len; g += BLOCK) {
        // the last word in [wlo, whi) that starts at or before p0 + g (words of no slots share their successor's start)
        unsigned long long lo = wlo, hi = whi;
        for (int it = 0; it < 64 && lo < hi; ++it) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (P.pos[mid] <= p0 + g) lo = mid + 1; else hi = mid;
        }
        const unsigned long long w = lo - 1; // (lo > wlo: pos[wlo] = p0 <= p0 + g)
        const uint32_t k = (uint32_t)(p0 + g - P.pos[w]);
        P.tiles[(size_t)t * CAP32 + g] = k < P.wcnt[w] ? P.wtok[P.off[w] - P.off_base + k] : YbW32::SEP;
    }
    if (threadIdx.x == 0) {
        P.tile_len[t] = len;
        P.tile_wbase[t] = (uint32_t)P.srank[wlo];
    }
}

struct Place32Params {
    const uint32_t *wtok;
    const uint32_t *wcnt;
    const unsigned long long *off;
    unsigned long long off_base, n_words;
    const unsigned long long *freq; // NULL: every word counts once
    const uint32_t *is_short, *is_long;
    const unsigned long long *srank, *lrank, *lpos;
    uint32_t *wfreq;                // by short rank
    uint32_t *long_tok;
    unsigned long long *long_off;
    uint32_t *long_len, *long_freq;
    uint32_t *overflow;             // a frequency above 2^32 - 1
};
// one lane per word: its weight, and a long word's tokens into the long-word buffer
__global__ __launch_bounds__(BLOCK) void k32_place_words(Place32Params P) {
    const unsigned long long w = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (w >= P.n_words) return;
    const unsigned long long f = P.freq ? P.freq[w] : 1ull;
    if (P.is_short[w]) {
        if (f > 0xFFFFFFFFull) atomicOr(P.overflow, 1u);
        P.wfreq[P.srank[w]] = (uint32_t)f;
    } else if (P.is_long[w]) {
        if (f > 0xFFFFFFFFull) atomicOr(P.overflow, 1u);
        const unsigned long long r = P.lrank[w], at = P.lpos[w];
        const uint32_t n = P.wcnt[w];
        P.long_off[r] = at;
        P.long_len[r] = n;
        P.long_freq[r] = (uint32_t)f;
        const uint32_t *src = P.wtok + (P.off[w] - P.off_base);
        for (uint32_t i = 0; i < n; ++i) P.long_tok[at + i] = src[i];
    }
}

} // namespace yb
