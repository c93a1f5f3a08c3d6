// id32_model.cpp -- TEST-ONLY CPU model of one word's rewrite under the width-parameterised rules of
// yet-another-bpe_amd/csrc/tile_logic.h (the header the HIP kernels include), at u16 and at u32 width.
// A word is staged as the kernels stage a tile (its tokens, SEP, PAD outside), the sites are marked with yb_is_site, the
// neighbour deltas come from yb_site_deltas_w and the rewritten word from yb_keep_w.  Never loaded by the product.
#include <cstdint>
#include <map>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/tile_logic.h"

namespace {

template <class W>
int apply_word(const uint32_t *ids, int n, uint32_t a, uint32_t b, uint32_t c, long long w, uint32_t *out_ids, int *out_n,
               uint32_t *d_left, uint32_t *d_right, long long *d_val, int *n_deltas) {
    std::vector<uint32_t> v(ids, ids + n);
    v.push_back(W::SEP);
    const int len = n + 1;
    auto T = [&](int q) -> uint32_t { return (q < 0 || q >= len) ? W::PAD : v[q]; };
    std::vector<uint8_t> mr(len + 8, 0);
    int run_start = 0;
    for (int p = 0; p < len; p++) {
        if (T(p) != a) { run_start = p + 1; continue; }
        mr[p] = yb_is_site(T(p), T(p + 1), a, b, p, run_start);
    }
    auto M = [&](int q) -> int { return (q < 0 || q >= len) ? 0 : mr[q]; };
    std::map<typename W::key_t, long long> delta;
    for (int p = 0; p < len; p++) {
        if (!mr[p]) continue;
        YbDeltasT<W> d;
        yb_site_deltas_w<W>(p, a, b, c, T, M, d);
        delta[W::key(a, b)] -= w;
        if (d.left) { delta[d.lo] -= w; delta[d.ln] += w; }
        if (d.right) { delta[d.ro] -= w; delta[d.rn] += w; }
    }
    int k = 0;
    for (int p = 0; p < len; p++) {
        uint32_t o = 0;
        if (yb_keep_w<W>(p, c, false, T, M, o) && o != W::SEP) out_ids[k++] = o;
    }
    *out_n = k;
    int nd = 0;
    for (auto &kv : delta) {
        if (kv.second == 0) continue;
        if (kv.first == W::EMPTY) return -1;
        d_left[nd] = W::left(kv.first);
        d_right[nd] = W::right(kv.first);
        d_val[nd] = kv.second;
        nd++;
    }
    *n_deltas = nd;
    return 0;
}

template <class W>
void key_info(uint32_t left, uint32_t right, unsigned long long *key, uint32_t *l2, uint32_t *r2, int *is_empty) {
    const typename W::key_t k = W::key(left, right);
    *key = (unsigned long long)k;
    *l2 = W::left(k);
    *r2 = W::right(k);
    *is_empty = k == W::EMPTY;
}

}  // namespace

extern "C" {

// width 16 or 32.  out_ids: room for n ids; the delta arrays: room for 5 n + 5 entries.
int id32_model_apply(int width, const uint32_t *ids, int n, uint32_t a, uint32_t b, uint32_t c, long long w, uint32_t *out_ids,
                     int *out_n, uint32_t *d_left, uint32_t *d_right, long long *d_val, int *n_deltas) {
    if (width == 16) return apply_word<YbW16>(ids, n, a, b, c, w, out_ids, out_n, d_left, d_right, d_val, n_deltas);
    return apply_word<YbW32>(ids, n, a, b, c, w, out_ids, out_n, d_left, d_right, d_val, n_deltas);
}

void id32_model_key(int width, uint32_t left, uint32_t right, unsigned long long *key, uint32_t *l2, uint32_t *r2, int *is_empty) {
    if (width == 16) key_info<YbW16>(left, right, key, l2, r2, is_empty);
    else key_info<YbW32>(left, right, key, l2, r2, is_empty);
}

// the sentinels and limits of a width: [0] SEP, [1] PAD, [2] MAX_TOKENS
void id32_model_limits(int width, uint32_t out[3]) {
    if (width == 16) { out[0] = YbW16::SEP; out[1] = YbW16::PAD; out[2] = YbW16::MAX_TOKENS; }
    else { out[0] = YbW32::SEP; out[1] = YbW32::PAD; out[2] = YbW32::MAX_TOKENS; }
}

// what the macros of tile_logic.h say (the u16 instantiation must mean the same)
void id32_model_macros(uint32_t out[4]) {
    out[0] = YB_SEP; out[1] = YB_PAD; out[2] = YB_MAX_TOKENS; out[3] = yb_pairkey(0x1234u, 0xABCDu);
}
}
