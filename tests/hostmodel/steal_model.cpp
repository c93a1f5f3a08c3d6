// CPU model of the sparse launch's second round (yet-another-bpe_amd/csrc/steal_logic.h): the piece sizes, and the tagged
// counter under every interleaving of its claimers' atomic operations.  Built by tests/test_steal_model.py.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/steal_logic.h"

namespace {
struct PlainOps { // the counter word as one thread sees it: yb_steal_claim as the kernel calls it
    unsigned long long *p;
    unsigned long long add(unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
    void max(unsigned long long v) { if (*p < v) *p = v; }
};

// One claimer = one workgroup's thread 0: claims until it is told that nothing is left.  yb_steal_claim cut at its atomics.
struct Claimer {
    int state = 0; // 0: first add of a claim, 1: the max that arms the word, 2: the add after it, 3: done
};
struct World {
    unsigned long long word, tag;
    uint32_t n_pieces;
    std::vector<Claimer> cl;
    std::vector<uint32_t> handed; // times each piece was handed out
    uint32_t empty_answers = 0;   // claims answered with "nothing left"
    bool stale_claimed = false;   // a value was taken from a word of another tag
};
void take(World &w, Claimer &c, unsigned long long old) {
    if (!yb_steal_current(old, w.tag)) w.stale_claimed = true;
    const uint32_t idx = yb_steal_idx(old);
    if (idx < w.n_pieces) {
        w.handed[idx]++;
        c.state = 0;
    } else {
        w.empty_answers++;
        c.state = 3;
    }
}
void step(World &w, uint32_t i) {
    Claimer &c = w.cl[i];
    PlainOps ops{&w.word};
    if (c.state == 0) {
        const unsigned long long old = ops.add(1ull);
        if (yb_steal_current(old, w.tag)) take(w, c, old);
        else c.state = 1;
    } else if (c.state == 1) {
        ops.max(yb_steal_arm(w.tag));
        c.state = 2;
    } else if (c.state == 2) {
        take(w, c, ops.add(1ull));
    }
}
bool finished(const World &w) {
    for (const Claimer &c : w.cl)
        if (c.state != 3) return false;
    return true;
}
bool good(const World &w) {
    if (w.stale_claimed || w.empty_answers != w.cl.size()) return false;
    for (uint32_t h : w.handed)
        if (h != 1u) return false;
    return true;
}
long long dfs(const World &w) { // every interleaving: number of complete schedules, or -1 at the first bad one
    if (finished(w)) return good(w) ? 1 : -1;
    long long n = 0;
    for (uint32_t i = 0; i < w.cl.size(); ++i) {
        if (w.cl[i].state == 3) continue;
        World v = w;
        step(v, i);
        const long long r = dfs(v);
        if (r < 0) return -1;
        n += r;
    }
    return n;
}
} // namespace

extern "C" {
uint32_t steal_piece_tiles(uint32_t rest, uint32_t blocks, uint32_t chunk) { return yb_piece_tiles(rest, blocks, chunk); }
uint32_t steal_piece_count(uint32_t rest, uint32_t piece) { return yb_piece_count(rest, piece); }
unsigned long long steal_arm(unsigned long long tag) { return yb_steal_arm(tag); }

// One thread, the kernel's own function: claims until nothing is left; out[] gets the pieces in the order handed out.
// Returns their number; *word is the counter before and after.
uint32_t steal_claim_all(unsigned long long *word, unsigned long long tag, uint32_t n_pieces, uint32_t *out, uint32_t cap) {
    PlainOps ops{word};
    uint32_t n = 0;
    for (;;) {
        const uint32_t idx = yb_steal_claim(ops, tag);
        if (idx >= n_pieces) return n;
        if (n < cap) out[n] = idx;
        ++n;
    }
}

// All interleavings of n_claimers over n_pieces, from the counter value `word` (any older launch's leftovers).
long long steal_exhaustive(unsigned long long word, unsigned long long tag, uint32_t n_pieces, uint32_t n_claimers) {
    World w{word, tag, n_pieces, std::vector<Claimer>(n_claimers), std::vector<uint32_t>(n_pieces, 0u)};
    return dfs(w);
}

// One interleaving given as a list of claimer indices (a finished claimer's turn is skipped; when the list ends the rest runs
// round robin).  Returns 1 if every piece went out exactly once, every claimer got one "nothing left" and no stale word was used.
int steal_schedule(unsigned long long word, unsigned long long tag, uint32_t n_pieces, uint32_t n_claimers, const uint32_t *sched, uint32_t n_sched,
                   unsigned long long *word_out) {
    World w{word, tag, n_pieces, std::vector<Claimer>(n_claimers), std::vector<uint32_t>(n_pieces, 0u)};
    for (uint32_t k = 0; k < n_sched && !finished(w); ++k) step(w, sched[k] % n_claimers);
    for (uint32_t i = 0; !finished(w); i = (i + 1) % n_claimers) step(w, i);
    if (word_out) *word_out = w.word;
    return good(w) ? 1 : 0;
}
}
