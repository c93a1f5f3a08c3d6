// CPU model of the candidate list and of the selection's window (yet-another-bpe_amd/csrc/select_logic.h): the list kept
// under the listing rule before the "listed" bitmap (a count that crosses T again is listed again) and under the rule with
// it, and the window found the old way (distinct pairs through a set) and the new way (a plain count of list entries).
// Built by tests/test_select_logic_model.py.
#include <stdint.h>

#include <algorithm>
#include <set>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/select_logic.h"

namespace {
// k_cand_rebuild: 64 consecutive slots per wave, the wave's ballot is the bitmap's word
uint32_t rebuild(const std::vector<long long> &cnt, unsigned long long T, bool bitmap, std::vector<uint32_t> &list, std::vector<unsigned long long> &bits) {
    list.clear();
    bits.assign(yb_cand_bitmap_words(cnt.size()), bitmap ? ~0ull : 0ull); // (stale words: the rebuild has to write every one)
    for (size_t s0 = 0; s0 < cnt.size(); s0 += 64) {
        unsigned long long word = 0;
        for (size_t lane = 0; lane < 64 && s0 + lane < cnt.size(); ++lane)
            if (yb_cand_rebuild_lists((unsigned long long)cnt[s0 + lane], T)) {
                word |= 1ull << lane;
                list.push_back((uint32_t)(s0 + lane));
            }
        if (bitmap) bits[yb_cand_word((uint32_t)s0)] = word;
    }
    return (uint32_t)list.size();
}
} // namespace

extern "C" {
uint32_t sel_win_attempts() { return YB_WIN_ATTEMPTS; }

// A rebuild at threshold T over counts[n_slots], then n_events adds (slot, delta) in order, as gt_bump sees them.
// rule 0: every crossing appends.  rule 1: a crossing appends if the slot's bit was clear.  counts[] is updated in place.
// -> length of the list (list_out holds up to list_cap of it); bits_out: yb_cand_bitmap_words(n_slots) words (rule 1).
uint32_t sel_list_replay(uint32_t n_slots, uint64_t T, int64_t *counts, uint32_t n_events, const uint32_t *ev_slot, const int64_t *ev_delta, int rule,
                         uint32_t *list_out, uint32_t list_cap, uint64_t *bits_out) {
    std::vector<long long> cnt(counts, counts + n_slots);
    std::vector<uint32_t> list;
    std::vector<unsigned long long> bits;
    rebuild(cnt, T, rule == 1, list, bits);
    for (uint32_t i = 0; i < n_events; ++i) {
        const uint32_t s = ev_slot[i];
        const unsigned long long old = (unsigned long long)cnt[s], now = old + (unsigned long long)ev_delta[i];
        cnt[s] = (long long)now;
        if (ev_delta[i] <= 0 || !yb_cand_crosses(old, now, T)) continue; // (gt_bump: only an add that raises a count looks)
        if (rule == 1) {
            const unsigned long long before = bits[yb_cand_word(s)];
            bits[yb_cand_word(s)] = before | yb_cand_bit(s);
            if (!yb_cand_lists(before, s)) continue;
        }
        list.push_back(s);
    }
    for (uint32_t s = 0; s < n_slots; ++s) counts[s] = cnt[s];
    for (size_t i = 0; i < list.size() && i < list_cap; ++i) list_out[i] = list[i];
    if (bits_out)
        for (size_t w = 0; w < bits.size(); ++w) bits_out[w] = bits[w];
    return (uint32_t)list.size();
}

// The window over list[n_list] (slots) with counts[slot].  rule 0: repeats allowed on the list, the window is the set of
// DISTINCT slots with count >= L, as the selection built it through its hash set.  rule 1: no repeats, a plain count
// (yb_win_search).  out[5]: L, n_win (0: no window), narrowed, fallback, attempts made; window_out: up to `win` slots, sorted.
void sel_window(uint32_t n_list, const uint32_t *list, const int64_t *counts, uint32_t kmax, uint32_t wshift, uint64_t T, uint32_t win, int rule,
                uint64_t *out, uint32_t *window_out) {
    unsigned long long cmax = 0;
    for (uint32_t i = 0; i < n_list; ++i)
        if (counts[list[i]] > 0) cmax = std::max(cmax, (unsigned long long)counts[list[i]]);
    std::vector<uint32_t> wnd;
    uint32_t attempts = 0;
    YbWindow w{0ull, 0u, 0u};
    if (rule == 1) {
        w = yb_win_search(cmax, kmax, wshift, T, win, [&](unsigned long long L, int) -> uint32_t {
            ++attempts;
            wnd.clear();
            for (uint32_t i = 0; i < n_list; ++i)
                if (counts[list[i]] > 0 && (unsigned long long)counts[list[i]] >= L) wnd.push_back(list[i]);
            return (uint32_t)wnd.size();
        });
    } else if (cmax) { // the loop as it stood before the bitmap
        unsigned long long delta = kmax > 1u ? std::min(std::max((unsigned long long)kmax, cmax >> wshift), 1ull << 31) : 0ull;
        for (int attempt = 0; attempt < 8; ++attempt) {
            ++attempts;
            w.L = cmax > delta ? cmax - delta : 1ull;
            if (kmax > 1u && w.L < T && cmax >= T) w.L = T;
            std::set<uint32_t> seen;
            for (uint32_t i = 0; i < n_list; ++i)
                if (counts[list[i]] > 0 && (unsigned long long)counts[list[i]] >= w.L) seen.insert(list[i]);
            wnd.assign(seen.begin(), seen.end());
            if (seen.size() <= win) {
                w.n = (uint32_t)seen.size();
                break;
            }
            if (delta == 0ull) break;
            delta >>= 2;
            w.narrowed += 2;
        }
    }
    out[0] = w.L;
    out[1] = w.n;
    out[2] = w.narrowed;
    out[3] = yb_win_fallback(cmax, w) ? 1u : 0u;
    out[4] = attempts;
    if (w.n) {
        std::sort(wnd.begin(), wnd.end());
        for (uint32_t i = 0; i < w.n; ++i) window_out[i] = wnd[i];
    }
}
}
