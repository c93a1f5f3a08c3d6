// CPU model of the persistent word pool: the rules of yet-another-bpe_amd/csrc/pool_logic.h (the functions the HIP kernels
// call), run sequentially in the kernels' shape -- the call's words pooled among themselves, then every call-unique word
// probed against an unchanging pool, then the growth, then every new word appended and inserted.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/pool_logic.h"

namespace {
struct Pool {
    std::vector<uint8_t> arena;  // (size = capacity; n_bytes of it used)
    std::vector<unsigned long long> off, count, hash;
    std::vector<uint32_t> slots;
    unsigned long long n = 0, n_bytes = 0;
    uint32_t hash_bits = 64;
    unsigned long long slot_growths = 0, arena_growths = 0, dropped = 0, probe_steps = 0;
};

void size_words(Pool &P, unsigned long long slot_cap) {
    P.off.resize(pl_words_for(slot_cap) + 1);
    P.count.resize(pl_words_for(slot_cap));
    P.hash.resize(pl_words_for(slot_cap));
}
void insert(Pool &P, uint32_t p) {  // first free slot of the chain (k_pool_append / k_pool_rehash)
    unsigned long long s = pl_home(P.hash[p], P.slots.size());
    while (P.slots[s] != PL_EMPTY) s = pl_next(s, P.slots.size());
    P.slots[s] = p;
}
} // namespace

extern "C" void *pool_model_new(uint64_t init_slots, uint64_t init_bytes, uint32_t hash_bits) {
    Pool *P = new Pool();
    const unsigned long long cap = pl_pow2(init_slots < 2 ? 2 : init_slots);
    P->slots.assign(cap, PL_EMPTY);
    size_words(*P, cap);
    P->off[0] = 0;
    P->arena.resize(init_bytes < 1 ? 1 : init_bytes);
    P->hash_bits = hash_bits > 64 ? 64 : hash_bits;
    return P;
}
extern "C" void pool_model_free(void *h) { delete (Pool *)h; }

// word i = bytes[off[i], off[i + 1]); freq == NULL: every word counts once.  Returns 0, or -4 past the word limit.
extern "C" int pool_model_add(void *h, const uint8_t *bytes, const uint64_t *off, const uint64_t *freq, uint64_t n_words) {
    Pool &P = *(Pool *)h;
    // 1. the call's words among themselves (what pool_words leaves: one representative and one count per byte string)
    std::vector<std::pair<uint64_t, unsigned long long>> uniq;  // (representative, count)
    std::unordered_map<std::string, size_t> seen;
    for (uint64_t w = 0; w < n_words; ++w) {
        std::string key((const char *)bytes + off[w], off[w + 1] - off[w]);
        auto it = seen.find(key);
        if (it == seen.end()) {
            seen.emplace(std::move(key), uniq.size());
            uniq.push_back({w, freq ? freq[w] : 1ull});
        } else {
            uniq[it->second].second += freq ? freq[w] : 1ull;
        }
    }
    // 2. probe: the pool is only read
    std::vector<uint32_t> hit(uniq.size());
    unsigned long long n_new = 0, new_bytes = 0;
    for (size_t u = 0; u < uniq.size(); ++u) {
        const uint64_t w = uniq[u].first;
        const unsigned long long L = off[w + 1] - off[w];
        if (L == 0) {
            hit[u] = PL_DROP;
            continue;
        }
        const unsigned long long mh = pl_mask_hash(pl_word_hash(bytes + off[w], L), P.hash_bits);
        hit[u] = PL_NEW;
        for (unsigned long long s = pl_home(mh, P.slots.size());; s = pl_next(s, P.slots.size())) {
            const uint32_t cur = P.slots[s];
            ++P.probe_steps;
            if (cur == PL_EMPTY) break;
            if (pl_match(P.hash[cur], P.off[cur + 1] - P.off[cur], P.arena.data() + P.off[cur], mh, L, bytes + off[w])) {
                hit[u] = cur;
                break;
            }
        }
        if (hit[u] == PL_NEW) {
            ++n_new;
            new_bytes += L;
        }
    }
    // 3. room for the new words
    if (P.n + n_new > PL_MAX_WORDS) return -4;
    if (pl_slots_full(P.n + n_new, P.slots.size())) {
        const unsigned long long cap = pl_slots_for(P.slots.size(), P.n + n_new);
        size_words(P, cap);
        P.slots.assign(cap, PL_EMPTY);
        for (unsigned long long p = 0; p < P.n; ++p) insert(P, (uint32_t)p);  // from the stored hashes: the arena is not read
        ++P.slot_growths;
    }
    if (P.n_bytes + new_bytes > P.arena.size()) {
        P.arena.resize(pl_grow(P.arena.size(), P.n_bytes + new_bytes));
        ++P.arena_growths;
    }
    // 4. append
    for (size_t u = 0; u < uniq.size(); ++u) {
        const uint64_t w = uniq[u].first;
        const unsigned long long L = off[w + 1] - off[w];
        if (hit[u] == PL_DROP) {
            P.dropped += uniq[u].second;
        } else if (hit[u] != PL_NEW) {
            P.count[hit[u]] += uniq[u].second;
        } else {
            const unsigned long long p = P.n++;
            memcpy(P.arena.data() + P.n_bytes, bytes + off[w], L);
            P.n_bytes += L;
            P.off[p + 1] = P.n_bytes;
            P.count[p] = uniq[u].second;
            P.hash[p] = pl_mask_hash(pl_word_hash(bytes + off[w], L), P.hash_bits);
            insert(P, (uint32_t)p);
        }
    }
    return 0;
}

// out[0..7]: n_unique, n_bytes, slot capacity, arena capacity, slot growths, arena growths, zero-length dropped, probe steps
extern "C" void pool_model_stats(void *h, uint64_t *out) {
    Pool &P = *(Pool *)h;
    const uint64_t v[8] = {P.n, P.n_bytes, P.slots.size(), P.arena.size(), P.slot_growths, P.arena_growths, P.dropped, P.probe_steps};
    memcpy(out, v, sizeof v);
}
// the pool as yabpe_pool_get hands it out: n_bytes bytes, n_unique + 1 offsets, n_unique counts
extern "C" void pool_model_get(void *h, uint8_t *out_bytes, uint64_t *out_off, uint64_t *out_count) {
    Pool &P = *(Pool *)h;
    memcpy(out_bytes, P.arena.data(), P.n_bytes);
    for (unsigned long long p = 0; p <= P.n; ++p) out_off[p] = P.off[p];
    for (unsigned long long p = 0; p < P.n; ++p) out_count[p] = P.count[p];
}
// invariants of the slot array: a power of two, at most half full, every word in exactly one slot of its own chain
extern "C" int pool_model_check(void *h) {
    Pool &P = *(Pool *)h;
    const unsigned long long cap = P.slots.size();
    if (cap & (cap - 1)) return 1;
    if (P.n * 2 > cap) return 2;
    std::vector<uint8_t> seen(P.n, 0);
    for (unsigned long long s = 0; s < cap; ++s)
        if (P.slots[s] != PL_EMPTY) {
            if (P.slots[s] >= P.n || seen[P.slots[s]]++) return 3;
        }
    for (unsigned long long p = 0; p < P.n; ++p) {
        if (!seen[p]) return 4;
        unsigned long long s = pl_home(P.hash[p], cap);
        while (P.slots[s] != p) {
            if (P.slots[s] == PL_EMPTY) return 5;  // a gap between the home slot and the word
            s = pl_next(s, cap);
        }
    }
    return 0;
}

#ifdef POOL_MODEL_MAIN
// stand-alone run (for a sanitizer build of the model: g++ -DPOOL_MODEL_MAIN -fsanitize=address,undefined)
#include <stdio.h>
int main() {
    for (uint32_t bits : {64u, 4u, 0u}) {
        void *h = pool_model_new(2, 1, bits);
        std::unordered_map<std::string, unsigned long long> ref;
        unsigned long long x = 12345;
        for (int call = 0; call < 40; ++call) {
            std::vector<uint8_t> bytes;
            std::vector<uint64_t> off{0};
            for (int w = 0; w < call * 3; ++w) {
                x = pl_mix(x + 0x9E3779B97F4A7C15ull);
                const unsigned L = (unsigned)(x % 5) + (w % 17 == 0 ? 70 : 0);
                std::string s;
                for (unsigned i = 0; i < L; ++i) s.push_back((char)('a' + (pl_mix(x + i) % 3)));
                bytes.insert(bytes.end(), s.begin(), s.end());
                off.push_back(bytes.size());
                if (L) ++ref[s];
            }
            bytes.push_back(0);
            if (pool_model_add(h, bytes.data(), off.data(), nullptr, off.size() - 1) != 0 || pool_model_check(h) != 0) return 1;
        }
        uint64_t st[8];
        pool_model_stats(h, st);
        std::vector<uint8_t> b(st[1] + 1);
        std::vector<uint64_t> o(st[0] + 1), c(st[0] + 1);
        pool_model_get(h, b.data(), o.data(), c.data());
        if (st[0] != ref.size()) return 2;
        for (uint64_t p = 0; p < st[0]; ++p)
            if (ref[std::string((const char *)b.data() + o[p], o[p + 1] - o[p])] != c[p]) return 3;
        printf("hash_bits %u: %llu unique words, %llu slot growths, %llu arena growths: ok\n", bits, (unsigned long long)st[0],
               (unsigned long long)st[4], (unsigned long long)st[5]);
        pool_model_free(h);
    }
    return 0;
}
#endif
