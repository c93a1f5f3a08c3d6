// replay_logic.h -- the rules that bring a word to the state a training run leaves it in, shared by the HIP kernels
// (yabpe_replay_kernels.h) and by the CPU unit-test model (tests/hostmodel/replay_model.cpp).
//
// A trained model's merges, as id triples (left, right, merged) in rank order, are the record of a merge loop: every word
// was rewritten by merge 0, then merge 1, ... each over its ID pair, greedily from left to right (tile_logic.h; for
// left == right the sites of a run a a a ... are its even positions).  That literal replay is the specification.  It is NOT
// the tokenizer's rule (lowest rank first, keyed by BYTES, last rank of a duplicated pair wins): an id that a later merge
// re-creates (trainer.py:298-300) meets pairs whose only ranks are already behind the loop, and they stay.
//
// Per-word form, equal to the literal replay (tests/test_replay_model.py holds the proof by comparison):
//   t = the rank applied last to this word (0 at the start).  The next merge is the leftmost adjacent pair whose smallest
//   rank >= t is the minimum over the word; a pair all of whose ranks are below t stays.  A pair may own several ranks
//   (duplicate entries of the merges list).  Why it is the same: ranks between t and the chosen one have no site in the
//   word (the literal replay passes them without a change), the chosen rank's sites are taken from the left one at a time
//   (>= t keeps that rank eligible until none is left; the merged token differs from both operands, so no new site of the
//   same rank appears), and every cached "smallest rank >= t" of an untouched pair is >= the chosen rank, so it stays valid.
#pragma once
#include <stdint.h>

#include "tile_logic.h" // YB_HD, yb_pairkey, the width traits YbW16 / YbW32, yb_hash48

constexpr uint32_t RP_NONE = 0xFFFFFFFFu; // no rank / no token / free index slot (a pair key is never 0xFFFFFFFF: ids < 0xFFFE)
constexpr uint32_t RP_SHORT = 64;         // words of at most this many bytes: one lane per byte

// ---------------------------------------------------------------- id-pair table: (left, right) -> its ranks, ascending
// One table for both id widths (tile_logic.h's traits): W::key_t keys, W::EMPTY (RP_NONE at 16 bits) for a free index slot
// and for the key of the closing entry, rp_index_hash for the slot a key starts at.
template <class W>
struct RpEntryT {
    typename W::key_t key; // W::key(left, right)
    uint32_t rank, merged;
};

template <class W>
struct RpTableT {
    const typename W::key_t *idx_key; // open addressing, load <= 1/2; W::EMPTY = free
    const uint32_t *idx_first;        // first entry of the key in `ent`
    uint32_t mask;                    // capacity - 1 (a power of two)
    const RpEntryT<W> *ent;           // sorted by (key, rank); closed by an entry with key W::EMPTY
};
typedef RpEntryT<YbW16> RpEntry;
typedef RpTableT<YbW16> RpTable;
typedef RpEntryT<YbW32> Rp32Entry;
// (the u32 load's kernel reads n as "anything to replay", and rp32_lookup bounds its walk over `ent` by it; the u16 kernels'
// arguments stay as they are)
struct Rp32Table : RpTableT<YbW32> {
    uint32_t n; // merges (0: nothing to replay)
};

YB_HD uint32_t rp_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
YB_HD uint32_t rp_index_hash(YbW16, uint32_t key) { return rp_mix(key); }
YB_HD uint32_t rp_index_hash(YbW32, unsigned long long key) { return yb_hash48(key); }

// The smallest rank >= tmin of the pair (a, b), and the id that merge writes.
YB_HD bool rp_lookup(const RpTable &t, uint32_t a, uint32_t b, uint32_t tmin, uint32_t *rank, uint32_t *merged) {
    const uint32_t key = yb_pairkey(a, b);
    uint32_t s = rp_mix(key) & t.mask;
    while (true) {
        const uint32_t k = t.idx_key[s];
        if (k == key) break;
        if (k == RP_NONE) return false;
        s = (s + 1) & t.mask;
    }
    for (uint32_t i = t.idx_first[s]; t.ent[i].key == key; ++i)
        if (t.ent[i].rank >= tmin) {
            *rank = t.ent[i].rank;
            *merged = t.ent[i].merged;
            return true;
        }
    return false;
}
// The same at 64-bit keys.  Two bodies on purpose: the one above is the inner loop of k_replay_words, unbounded (it relies on
// load <= 1/2); this one gives up after mask + 1 probes and never reads past the n entries.
YB_HD bool rp32_lookup(const Rp32Table &t, uint32_t a, uint32_t b, uint32_t tmin, uint32_t *rank, uint32_t *merged) {
    const unsigned long long key = YbW32::key(a, b);
    uint32_t s = yb_hash48(key) & t.mask;
    bool hit = false;
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = t.idx_key[s];
        if (k == key) {
            hit = true;
            break;
        }
        if (k == YbW32::EMPTY) return false;
        s = (s + 1) & t.mask;
    }
    if (!hit) return false;
    for (uint32_t i = t.idx_first[s]; i < t.n && t.ent[i].key == key; ++i)
        if (t.ent[i].rank >= tmin) {
            *rank = t.ent[i].rank;
            *merged = t.ent[i].merged;
            return true;
        }
    return false;
}

// ---------------------------------------------------------------- one word, sequentially (any length)
// A binary min-heap of (rank << 32 | position) with lazy invalidation: an entry is current iff its position still starts a
// token that has a right neighbour and the smallest rank >= t of the pair there is still the entry's.  Entries leave the
// heap in (rank, position) order, so t -- the rank of the last entry applied -- never exceeds a live entry's rank, and a
// live entry's rank is still the pair's smallest >= t.  O(L log L).
// Scratch: tok, nxt, prv of L entries, heap of 3 L entries.  Returns the number of tokens; tok[0..count) = their ids.
YB_HD void rp_heap_push(unsigned long long *heap, uint32_t &hn, unsigned long long v) {
    uint32_t k = hn++;
    while (k > 0) {
        const uint32_t p = (k - 1) >> 1;
        if (heap[p] <= v) break;
        heap[k] = heap[p];
        k = p;
    }
    heap[k] = v;
}

YB_HD unsigned long long rp_heap_pop(unsigned long long *heap, uint32_t &hn) {
    const unsigned long long top = heap[0];
    const unsigned long long v = heap[--hn];
    uint32_t k = 0;
    while (true) {
        uint32_t c = 2 * k + 1;
        if (c >= hn) break;
        if (c + 1 < hn && heap[c + 1] < heap[c]) ++c;
        if (v <= heap[c]) break;
        heap[k] = heap[c];
        k = c;
    }
    if (hn) heap[k] = v;
    return top;
}

YB_HD uint32_t rp_walk_heap(const uint8_t *w, uint32_t L, const RpTable &t, uint32_t *tok, uint32_t *nxt, uint32_t *prv,
                            unsigned long long *heap) {
    for (uint32_t p = 0; p < L; ++p) {
        tok[p] = w[p]; // ids 0..255 are the single bytes
        nxt[p] = p + 1 < L ? p + 1 : RP_NONE;
        prv[p] = p ? p - 1 : RP_NONE;
    }
    uint32_t hn = 0, r = 0, res = 0, tmin = 0;
    for (uint32_t p = 0; p + 1 < L; ++p)
        if (rp_lookup(t, tok[p], tok[p + 1], 0u, &r, &res)) rp_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
    while (hn) {
        const unsigned long long e = rp_heap_pop(heap, hn);
        const uint32_t p = (uint32_t)e, er = (uint32_t)(e >> 32);
        if (tok[p] == RP_NONE) continue; // no longer a token start
        const uint32_t q = nxt[p];
        if (q == RP_NONE) continue;
        if (!rp_lookup(t, tok[p], tok[q], tmin, &r, &res) || r != er) continue; // the pair there changed
        tmin = er;
        tok[p] = res;
        tok[q] = RP_NONE;
        nxt[p] = nxt[q];
        if (nxt[q] != RP_NONE) prv[nxt[q]] = p;
        if (nxt[p] != RP_NONE && rp_lookup(t, tok[p], tok[nxt[p]], tmin, &r, &res)) rp_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
        const uint32_t a = prv[p];
        if (a != RP_NONE && rp_lookup(t, tok[a], tok[p], tmin, &r, &res)) rp_heap_push(heap, hn, ((unsigned long long)r << 32) | a);
    }
    uint32_t k = 0, p = L ? 0 : RP_NONE;
    while (p != RP_NONE) { // compact (k <= p: only entries already read are overwritten)
        const uint32_t np = nxt[p];
        tok[k++] = tok[p];
        p = np;
    }
    return k;
}

// ---------------------------------------------------------------- one word of at most RP_SHORT bytes, in the lane form
// What k_replay_words does with a wave, written over arrays of 64 lanes so that the host can run it: lane p holds the token
// that starts at byte p (while one does) and the smallest rank >= t of the pair it begins; each step takes the smallest
// (rank << 6 | lane) over the lanes, and only the merged lane and its left neighbour look the table up again.
YB_HD unsigned long long rp_lane_key(bool alive, uint32_t rk, uint32_t lane) {
    return (alive && rk != RP_NONE) ? (((unsigned long long)rk << 6) | lane) : ~0ull;
}

inline uint32_t rp_walk_lanes(const uint8_t *w, uint32_t L, const RpTable &t, uint16_t *out) {
    uint32_t tok[RP_SHORT], rk[RP_SHORT], res[RP_SHORT];
    bool alive[RP_SHORT], dirty[RP_SHORT];
    for (uint32_t l = 0; l < RP_SHORT; ++l) {
        tok[l] = l < L ? w[l] : 0u;
        alive[l] = l < L;
        dirty[l] = true;
        rk[l] = RP_NONE;
        res[l] = 0;
    }
    uint32_t tmin = 0;
    auto next_alive = [&](uint32_t l) -> int {
        for (uint32_t q = l + 1; q < RP_SHORT; ++q)
            if (alive[q]) return (int)q;
        return -1;
    };
    while (true) {
        unsigned long long m = ~0ull;
        for (uint32_t l = 0; l < RP_SHORT; ++l) {
            if (dirty[l]) {
                rk[l] = RP_NONE;
                const int nx = next_alive(l);
                if (alive[l] && nx >= 0 && !rp_lookup(t, tok[l], tok[nx], tmin, &rk[l], &res[l])) rk[l] = RP_NONE;
                dirty[l] = false;
            }
            const unsigned long long key = rp_lane_key(alive[l], rk[l], l);
            m = key < m ? key : m;
        }
        if (m == ~0ull) break;
        const uint32_t win = (uint32_t)(m & 63);
        tmin = (uint32_t)(m >> 6);
        const int right = next_alive(win);
        tok[win] = res[win];
        dirty[win] = true;
        alive[right] = false;
        for (int q = (int)win - 1; q >= 0; --q)
            if (alive[q]) {
                dirty[q] = true;
                break;
            }
    }
    uint32_t k = 0;
    for (uint32_t l = 0; l < RP_SHORT; ++l)
        if (alive[l]) out[k++] = (uint16_t)tok[l];
    return k;
}

// ---------------------------------------------------------------- the table, built on the host
#include <algorithm>
#include <vector>

template <class W>
struct RpTableHostT {
    std::vector<typename W::key_t> idx_key;
    std::vector<uint32_t> idx_first;
    std::vector<RpEntryT<W>> ent;
    uint32_t n_merges() const { return (uint32_t)ent.size() - 1u; }
    RpTableT<W> table() const { return RpTableT<W>{idx_key.data(), idx_first.data(), (uint32_t)idx_key.size() - 1u, ent.data()}; }
};
typedef RpTableHostT<YbW16> RpTableHost;
typedef RpTableHostT<YbW32> Rp32TableHost;

// The one builder of both widths: entries sorted by (key, rank) and closed by an empty one, an index of at least 16 slots
// and at least twice the merges, every key at the first free slot from its hash on.
template <class W>
inline void rp_build_table(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n, RpTableHostT<W> *m) {
    typedef RpEntryT<W> Entry;
    m->ent.resize((size_t)n + 1);
    for (uint32_t i = 0; i < n; ++i) m->ent[i] = Entry{W::key(left[i], right[i]), i, merged[i]};
    std::sort(m->ent.begin(), m->ent.begin() + n, [](const Entry &x, const Entry &y) { return x.key != y.key ? x.key < y.key : x.rank < y.rank; });
    m->ent[n] = Entry{W::EMPTY, RP_NONE, RP_NONE};
    size_t cap = 16;
    while (cap < 2 * (size_t)n) cap <<= 1;
    m->idx_key.assign(cap, W::EMPTY);
    m->idx_first.assign(cap, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        if (i && m->ent[i - 1].key == m->ent[i].key) continue;
        uint32_t s = rp_index_hash(W(), m->ent[i].key) & (uint32_t)(cap - 1);
        while (m->idx_key[s] != W::EMPTY) s = (s + 1) & (uint32_t)(cap - 1);
        m->idx_key[s] = m->ent[i].key;
        m->idx_first[s] = i;
    }
}
