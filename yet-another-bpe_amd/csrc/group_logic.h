// group_logic.h -- digit groups: the GPT-2 pattern with \p{N}+ replaced by \p{N}{1,G} (option "digit_group"), shared by
// the HIP kernels (k_grp_* in yabpe_pretok_kernels.h) and by the CPU unit-test model (tests/hostmodel/group_model.cpp).
//
// What is reproduced: regex.findall with
//     '(?:[sdmt]|ll|ve|re)| ?\p{L}+| ?\p{N}{1,G}| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
// (training: the special tokens in front of it; encode: after the tokenizer's special split).  A digit run that GPT-2
// keeps as one pre-token is cut after every G characters, counted from the run's first digit; an optional U+0020 in front
// stays with the first group.  Nothing else changes: after a group of G digits the next alternative that matches a digit
// is " ?\p{N}{1,G}" again, without a space to take.
//
// The rule as the device computes it, on the flags the GPT-2 rules left (pretok_logic.h):
//   flags[j]   0 no start, GRP_START a pre-token starts here, GRP_INSIDE a byte of a special token after its first (only
//              written when G >= 1; the grouping pass turns it back into 0)
//   d(j)       number of \p{N} lead bytes in [s, j), where s is the nearest byte at or before j with flags[s] != 0
//   new start  at every \p{N} lead byte j with flags[j] == 0 and d(j) a POSITIVE multiple of G
// d(j) counts characters, not bytes (only lead bytes count).  d(j) = 0 happens for the first digit after the " " that
// starts its token: that digit belongs to group 0.  A \p{N} character that is not a start and not inside a special is
// always part of a " ?\p{N}+" token (the only other tokens that hold several characters are runs of another class,
// contractions, which are letters, and specials), so no other token is ever cut.  With G >= 1 no special token of the
// TRAINING pattern may begin with a \p{N} character: it could match at a group boundary, where GPT-2 has no token start
// and the special pass therefore never looks ("77" in "123774", G = 3: regex gives 123|77|4).
//
// d(j) has no bounded reach, so it is carried as a segmented scan.  A state is what a stretch of bytes does to the count:
//   GRP_RESET   set: the stretch holds a byte with flags != 0, and cnt counts from the last of them
//   cnt         \p{N} lead bytes counted, FOLDED: x for x < G, G + x % G otherwise -- keeps "positive multiple of G"
//               (folded value == G) and stays below 2 G <= 510
// grp_combine is associative, so bytes, 16-byte pieces and windows can be combined in any grouping that keeps the order.
#pragma once
#include <stdint.h>

#include "pretok_logic.h"

enum : uint8_t { GRP_START = 1, GRP_INSIDE = 2 };

typedef uint32_t GrpState;
constexpr GrpState GRP_RESET = 1u << 16;
constexpr uint32_t GRP_CNT = 0xFFFFu;
constexpr int GRP_PIECE = 16;   // bytes one thread owns: one 16-B load of meta and of flags
constexpr int GRP_WIN = 4096;   // bytes per workgroup and iteration (PT_WIN)
constexpr uint32_t GRP_MAX = 255; // largest group

YB_HD bool grp_is_digit(uint8_t meta) { return (meta & (PT_CLS | PT_CONT)) == PT_N; } // lead byte of a \p{N} character

// x < 4 G -> folded
YB_HD uint32_t grp_fold(uint32_t x, uint32_t G) {
    if (x >= 2 * G) x -= G;
    if (x >= 2 * G) x -= G;
    return x;
}

// first a, then b
YB_HD GrpState grp_combine(GrpState a, GrpState b, uint32_t G) {
    if (b & GRP_RESET) return b;
    return (a & GRP_RESET) | grp_fold((a & GRP_CNT) + (b & GRP_CNT), G);
}

// the state of one byte
YB_HD GrpState grp_byte(uint8_t meta, uint8_t flag) { return (flag ? GRP_RESET : 0u) | (grp_is_digit(meta) ? 1u : 0u); }

// THE rule: `before` = the combined state of every byte in front of this one.  Returns the byte's final flag (0 / 1).
YB_HD uint8_t grp_flag(GrpState before, uint8_t meta, uint8_t flag, uint32_t G) {
    if (flag) return flag == GRP_START ? 1 : 0;
    return grp_is_digit(meta) && (before & GRP_CNT) == G ? 1 : 0;
}

// One piece of GRP_PIECE bytes: get(k, &meta, &flag) gives byte k of it (bytes past the text: meta PT_O, flag 0).
template <class Get>
YB_HD GrpState grp_piece_state(Get get, uint32_t G) {
    GrpState s = 0;
#pragma unroll
    for (int k = 0; k < GRP_PIECE; ++k) {
        uint8_t m, f;
        get(k, &m, &f);
        s = grp_combine(s, grp_byte(m, f), G);
    }
    return s;
}

// The piece's final flags through put(k, flag); `before` = the state in front of its first byte.
template <class Get, class Put>
YB_HD void grp_piece_flags(GrpState before, Get get, Put put, uint32_t G) {
    GrpState s = before;
#pragma unroll
    for (int k = 0; k < GRP_PIECE; ++k) {
        uint8_t m, f;
        get(k, &m, &f);
        put(k, grp_flag(s, m, f, G));
        s = grp_combine(s, grp_byte(m, f), G);
    }
}
