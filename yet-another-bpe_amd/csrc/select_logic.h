// select_logic.h -- the pure rules of the candidate list and of the selection's window (the select_eval row).
// Shared by the kernels that keep the list (cand_note, k_cand_rebuild in yabpe_kernels.h), the fused selection
// (select_eval) and the CPU model (tests/hostmodel/select_model.cpp).
//
// The list: between two rebuilds every table slot whose count is >= T is on it, and no slot is on it twice.  One "listed"
// bit per table slot keeps repeats out: a count that crosses T sets its slot's bit with ONE returning OR and appends the
// slot only if the bit was clear.  A rebuild writes list and bitmap together.
//
// The window: the list entries with count >= L, L = cmax - delta, never below T while the maximum is on the list.  The list
// holds every pair once, so the window's size is a plain count of entries; more than the window holds: a quarter of the
// distance, again; more than that tie at the top (or eight attempts did not do): no window, a batch of one.
#pragma once
#include <stdint.h>

#include "tile_logic.h"

#define YB_WIN_ATTEMPTS 8

// ---- the list
// The add that took a count from `old` to `now` crosses the threshold.  (Signed: a count can be transiently negative while
// the deltas of one merge arrive in any order.)  Adds to one address are totally ordered: one adder sees each crossing.
YB_HD bool yb_cand_crosses(unsigned long long old, unsigned long long now, unsigned long long T) {
    return (long long)now >= (long long)T && (long long)old < (long long)T && (long long)now > 0;
}
YB_HD uint64_t yb_cand_bitmap_words(uint64_t table_cap) { return (table_cap + 63u) / 64u; }
YB_HD uint32_t yb_cand_word(uint32_t slot) { return slot >> 6; }
YB_HD unsigned long long yb_cand_bit(uint32_t slot) { return 1ull << (slot & 63u); }
// A crossing lists its slot when the word its OR returned had the slot's bit clear.
YB_HD bool yb_cand_lists(unsigned long long word_before, uint32_t slot) { return (word_before & yb_cand_bit(slot)) == 0ull; }
// A rebuild lists a slot with this count.
YB_HD bool yb_cand_rebuild_lists(unsigned long long count, unsigned long long T) { return (long long)count > 0 && count >= T; }

// ---- the window
// How far under the maximum the first attempt reaches: the batch limit at least, cmax >> wshift, 2^31 at the most (the sort
// key keeps count - L in 32 bits); a batch of one needs the top level only.
YB_HD unsigned long long yb_win_delta0(uint32_t kmax, unsigned long long cmax, uint32_t wshift) {
    if (kmax <= 1u) return 0ull;
    unsigned long long d = cmax >> wshift;
    if (d < (unsigned long long)kmax) d = (unsigned long long)kmax;
    return d < (1ull << 31) ? d : (1ull << 31);
}
// The window's floor.  Never below the list's threshold: only pairs with count >= T are on EVERY replica's list -- a pair
// below it may be listed on one rank and not on another, and the window's size decides how far a batch can go.
YB_HD unsigned long long yb_win_floor(unsigned long long cmax, unsigned long long delta, uint32_t kmax, unsigned long long T) {
    unsigned long long L = cmax > delta ? cmax - delta : 1ull;
    if (kmax > 1u && L < T && cmax >= T) L = T;
    return L;
}
YB_HD unsigned long long yb_win_narrow(unsigned long long delta) { return delta >> 2; }

struct YbWindow {
    unsigned long long L; // floor of the last attempt
    uint32_t n;           // entries of the window; 0 with cmax != 0: no window (the fallback finds ONE merge the plain way)
    uint32_t narrowed;    // what the narrowing added to the shift (2 per step)
};
// The search for the floor.  count(L, attempt) -> number of list entries with count >= L (the device also writes the first
// `win` of them to LDS).  The same loop on the device and in the CPU model.
template <class CountF>
YB_HD YbWindow yb_win_search(unsigned long long cmax, uint32_t kmax, uint32_t wshift, unsigned long long T, uint32_t win, CountF count) {
    YbWindow w{0ull, 0u, 0u};
    if (!cmax) return w;
    unsigned long long delta = yb_win_delta0(kmax, cmax, wshift);
    for (int attempt = 0; attempt < YB_WIN_ATTEMPTS; ++attempt) {
        w.L = yb_win_floor(cmax, delta, kmax, T);
        const uint32_t n = count(w.L, attempt);
        if (n <= win) {
            w.n = n;
            break;
        }
        if (delta == 0ull) break; // more than `win` pairs tie at the top: no window
        delta = yb_win_narrow(delta);
        w.narrowed += 2u;
    }
    return w;
}
YB_HD bool yb_win_fallback(unsigned long long cmax, const YbWindow &w) { return cmax != 0ull && w.n == 0u; }
