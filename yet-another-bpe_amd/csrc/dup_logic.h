// dup_logic.h -- the exact-substring rule (BBPETokenizer.duplicate_spans, yet_another_bpe/tokenizer.py), host- and device-
// callable: yabpe_dup_kernels.h and yabpe_dup_spans (yabpe.hip) call the same functions.
//
// Inputs ids u32[n_ids], n_docs document starts, min_len = n in [1, 1024].  All of it integer:
//   window      n consecutive ids inside one document: global position p starts one iff p + n <= the end of p's document.
//   first[p]    the smallest global position whose window holds the same n ids as p's, in any document.
//   repeat      window p iff first[p] + n <= p: an equal window ENDS at or before p begins.  (When the smallest equal window
//               overlaps p, every later equal one before p overlaps it too, so first[] decides.)
//   dup[i]      1 iff i lies inside a repeat window of its document; n_dup[d] counts them; a span is a maximal run of them.
// The table of the device: open addressing, linear probing, a power of two of slots; a slot holds the POSITION of a window,
// DUP_EMPTY before, and only ever moves between positions of equal windows, downwards: it ends at first[].
// The window hash only chooses the home slot and never decides equality.  With m(id) = mix(G * (id + 1)) and the Horner prefix
// P[i + 1] = P[i] * B + m(id_i) mod 2^64: H(p) = P[p + n] - P[p] * B^n = sum m(id_{p+j}) B^(n-1-j), a function of the window
// alone wherever the prefix started -- one multiply-subtract per window.  Home slot: the high bits of mix(H).
#pragma once
#include <stdint.h>

#include "minhash_logic.h"

constexpr uint32_t DUP_EMPTY = 0xFFFFFFFFu;               // a free slot; "no slot"
constexpr uint32_t DUP_MAX_LEN = 1024;                    // min_len at most: the mask's halo stays within one tile
constexpr uint32_t DUP_TILE = 1024;                       // window positions of one piece; id positions of one mark tile
constexpr unsigned long long DUP_MAX_IDS = 1ull << 30;    // positions and slots stay below 2^32
constexpr uint32_t DUP_MIN_SLOTS_LOG2 = 10, DUP_MAX_SLOTS_LOG2 = 31;
constexpr unsigned long long DUP_B = 0xD6E8FEB86659FD93ull;  // the Horner base: odd, so a unit mod 2^64
constexpr uint32_t DUP_F_COMPACT = 1;                     // YABPE_DUP_COMPACT

// the rule's argument checks (yabpe_dup_spans and BBPETokenizer._dup_len refuse the same things)
YB_HD bool dup_rule_valid(uint32_t min_len, uint32_t flags) { return min_len >= 1 && min_len <= DUP_MAX_LEN && !(flags & ~DUP_F_COMPACT); }

YB_HD unsigned long long dup_windows(unsigned long long L, uint32_t n) { return L >= n ? L - n + 1 : 0ull; }
YB_HD unsigned long long dup_tiles(unsigned long long count) { return (count + DUP_TILE - 1) / DUP_TILE; }  // pieces of windows, tiles of ids

// auto size: the smallest power of two >= 2 x windows, at least 2^10 (windows <= 2^30: at most 2^31 slots)
YB_HD uint32_t dup_slots_log2(unsigned long long windows) {
    uint32_t lg = DUP_MIN_SLOTS_LOG2;
    while ((1ull << lg) < 2 * windows) ++lg;
    return lg;
}

YB_HD constexpr unsigned long long dup_pow(unsigned long long b, uint32_t e) {  // b^e mod 2^64
    unsigned long long r = 1;
    for (; e; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

YB_HD unsigned long long dup_m(uint32_t id) { return enc_mix(ENC_RND_G * ((unsigned long long)id + 1)); }
YB_HD unsigned long long dup_horner(unsigned long long P, uint32_t id) { return P * DUP_B + dup_m(id); }
// H(p) from P[p], P[p + n] and B^n
YB_HD unsigned long long dup_window_hash(unsigned long long P_lo, unsigned long long P_hi, unsigned long long pow_n) { return P_hi - P_lo * pow_n; }
YB_HD uint32_t dup_home(unsigned long long H, uint32_t slots_log2) { return (uint32_t)(enc_mix(H) >> (64 - slots_log2)); }

// the repeat predicate (positions below 2^30, n <= 1024: no overflow)
YB_HD bool dup_is_repeat(uint32_t first, uint32_t p, uint32_t n) { return first != DUP_EMPTY && first + n <= p; }
