// Stand-alone check of the replay table at 64-bit keys (rp_build_table<YbW32> + rp32_lookup through replay_model.cpp's
// entry point) against a std::map, for a build with -fsanitize=address,undefined: the cases of tests/test_replay_model.py.
// Prints the number of lookups it compared; any difference ends it with status 1.  Test infrastructure only.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <utility>

#include "replay_model.cpp"

namespace {

constexpr unsigned RANDOM_SEED = 15;  // (argv[1] overrides it, to look for another one)

struct Case {
    const char *name;
    std::vector<uint32_t> l, r, m;
    void add(uint32_t a, uint32_t b, uint32_t c) { l.push_back(a), r.push_back(b), m.push_back(c); }
};

unsigned long long run(const Case &C, bool want_wrap) {
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> ranks;  // (left, right) -> its ranks, ascending
    for (uint32_t i = 0; i < C.l.size(); ++i) ranks[{C.l[i], C.r[i]}].push_back(i);
    std::vector<uint32_t> a, b, tmin;
    std::vector<long long> want;  // the rank expected, -1: none
    auto ask = [&](uint32_t x, uint32_t y, uint32_t t) {
        a.push_back(x), b.push_back(y), tmin.push_back(t);
        long long w = -1;
        auto it = ranks.find({x, y});
        if (it != ranks.end())
            for (uint32_t rk : it->second)
                if (rk >= t) {
                    w = rk;
                    break;
                }
        want.push_back(w);
    };
    for (const auto &kv : ranks) {
        ask(kv.first.first, kv.first.second, 0);
        for (uint32_t rk : kv.second) ask(kv.first.first, kv.first.second, rk);
        ask(kv.first.first, kv.first.second, kv.second.back() + 1);
        ask(kv.first.second, kv.first.first + 1, 0);  // (mostly absent; the map says which)
    }
    ask(0, 0, 0), ask(0xFFFFFDu, 0xFFFFFDu, 0), ask(65536, 1, 0);
    const uint32_t n_q = (uint32_t)a.size();
    std::vector<uint8_t> found(n_q);
    std::vector<uint32_t> rank(n_q), res(n_q);
    uint32_t displaced = 0, wrapped = 0;
    replay_model_lookup32(C.l.data(), C.r.data(), C.m.data(), (uint32_t)C.l.size(), a.data(), b.data(), tmin.data(), n_q, found.data(), rank.data(),
                          res.data(), &displaced, &wrapped);
    for (uint32_t q = 0; q < n_q; ++q) {
        const bool ok = want[q] < 0 ? !found[q] : (found[q] && rank[q] == (uint32_t)want[q] && res[q] == C.m[rank[q]]);
        if (!ok) {
            fprintf(stderr, "%s: lookup (%u, %u) at tmin %u: want rank %lld, got %d / %u\n", C.name, a[q], b[q], tmin[q], want[q], (int)found[q], rank[q]);
            exit(1);
        }
    }
    if (want_wrap && (!displaced || !wrapped)) {
        fprintf(stderr, "%s: %u keys displaced, %u wrapped: the case does not reach the wrap\n", C.name, displaced, wrapped);
        exit(1);
    }
    return n_q;
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : RANDOM_SEED;
    unsigned long long n = 0;
    Case none{"no merges"};
    n += run(none, false);
    Case one{"one merge"};
    one.add(97, 98, 256);
    n += run(one, false);
    Case three{"one pair, three ranks"};
    three.add(1, 2, 300), three.add(2, 2, 301), three.add(1, 2, 300), three.add(3, 1, 302), three.add(1, 2, 300);
    n += run(three, false);
    Case wide{"ids above 65,535"};
    const uint32_t top = 0xFFFFFDu;  // 2^24 - 3
    wide.add(top, top, 70000), wide.add(65536, top, 70001), wide.add(top, 65536, 70002), wide.add(70000, 70001, top), wide.add(top, top, 70000);
    wide.add(65535, 65536, 70003), wide.add(1, 65536, 70004), wide.add(65536, 1, 70005);
    n += run(wide, false);
    Case rnd{"2,000 random triples over 40 ids"};
    std::mt19937 rng(seed);  // (a seed at which a probe sequence runs past the end of the index: run() checks it)
    uint32_t ids[40];
    for (uint32_t &id : ids) id = rng() % (top + 1);
    for (int i = 0; i < 2000; ++i) {
        const uint32_t a = ids[rng() % 40], b = ids[rng() % 40];
        rnd.add(a, b, rng() % (top + 1));
    }
    n += run(rnd, true);
    printf("ok: %llu lookups\n", n);
    return 0;
}
