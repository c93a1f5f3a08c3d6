// split4_logic.h -- the cl100k split pattern (GPT-4, Llama-3, Qwen2; option "split_pattern" = 1), shared by the HIP kernels
// (k_pt4_fused / k_pt4_special / k_nl_* in yabpe_pretok_kernels.h) and by the CPU unit-test model
// (tests/hostmodel/split4_model.cpp).
//
// What is reproduced: regex.findall with
//     (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,G}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
// (training: the special tokens in front of it; encode: after the tokenizer's special split).  As with the GPT-2 pattern the
// pre-tokens partition the text, so one flag per byte describes the result.  Classes L N S O as in pretok_logic.h, and
// R = {U+000A, U+000D} (a subset of S), SP = U+0020, both known by their byte.  For the character c at j, with p the
// character before it and x the one after it in the same text:
//
//   0  a text start (chunk start, encode piece start, end of a taken special) is a start
//   1  an apostrophe at q is TAKEN iff one of s S U+017F d D m M t T, [lL][lL], [vV][eE], [rR][eE] follows and q is a text
//      start or p(q) is L, N or S other than SP.  Then q is a start, the suffix letters are not, and the character behind
//      the suffix is a start whatever it is (it sits at q + 2 or q + 3)
//   2  c is N: a start iff p is not N (no space prefix; the groups of G are cut by group_logic.h, unchanged)
//   3  c is L: p is L: no; p is N: yes; p is S: iff p is in R; p is O: iff p is NOT itself a start (the one character in
//      front of a letter run that is neither letter, digit, CR nor LF belongs to the run unless it is taken already)
//   4  c is O: a start iff p is neither O nor SP
//   5  c is in R: a start iff p is L or N (behind an O it belongs to that token, behind whitespace it is inside the run)
//   6  c is in S \ R: p is not S: yes; p is in S \ R: iff x exists in this text and is not S; p is in R: iff not F(j) or B(j):
//        F(j)  a character of R occurs later in this whitespace run (before the next non-S character or the text end):
//              \s*[\r\n]+ then takes the run up to its last R, and j is inside
//        B(j)  every character of the run in front of j is in R and the character in front of the run is an O of this
//              text: "O+[\r\n]*" has swallowed them, and the whitespace starts anew at j
//
// Rules 0 .. 5 and the first two lines of 6 look at most 11 bytes back and 4 ahead (pt4_is_start).  F and B have no bounded
// reach -- a file of blank lines, a newline and a gigabyte of spaces -- so pt4_is_start answers PT4_PENDING there, and a pass
// of two segmented scans (one in each direction) over meta and flags resolves it.  Both scans carry one of three values,
// "keep / set to 0 / set to 1", combined as (b == keep ? a : b): associative, so bytes, 16-byte pieces and windows combine
// in any grouping that keeps the order.
//
// Flags between the local pass and the scan pass: 0, 1 (start), GRP_INSIDE (a byte of a taken special after its first),
// PT4_FIRST (the first byte of a taken special: a one-byte special that is an O character must not count as the O of B),
// PT4_PENDING.  The scan pass leaves 0 / 1 / GRP_INSIDE, which is what the digit-group pass reads.
#pragma once
#include <stdint.h>

#include "group_logic.h"
#include "pretok_logic.h"

enum : uint8_t {
    PT4_FIRST = 3,
    PT4_PENDING = 4,
    PT4_NL = 16, // meta bit, set by the cl100k local pass only: the byte is U+000A or U+000D
};

YB_HD bool pt4_is_nl(uint8_t b) { return b == '\n' || b == '\r'; }

// lead byte of the character in front of j (j > 0, not a text start; bounded: malformed text is reported, not followed)
YB_HD uint64_t pt4_prev(const PtView &v, uint64_t j) {
    uint64_t prev = j - 1;
    for (int k = 0; k < 3 && prev > 0 && (v.M(prev) & PT_CONT); ++k) --prev;
    return prev;
}

YB_HD bool pt4_exists(const PtView &v, uint64_t j) { return j < v.n && !(v.M(j) & PT_CHUNK0); }

// Contraction suffix behind an apostrophe at q, in BYTES: 1 (s d m t), 2 (ll ve re, or U+017F), 0 for none.
YB_HD int pt4_contraction_len(const PtView &v, uint64_t q) {
    if (v.T(q) != '\'' || !pt4_exists(v, q + 1)) return 0;
    const uint8_t x = v.T(q + 1), xl = (uint8_t)(x | 0x20);
    if (xl == 's' || xl == 'd' || xl == 'm' || xl == 't') return 1; // (x | 0x20 is a lower-case letter only for that letter)
    if (!pt4_exists(v, q + 2)) return 0;
    const uint8_t y = v.T(q + 2), yl = (uint8_t)(y | 0x20);
    if (x == 0xC5 && y == 0xBF) return 2; // U+017F, the one non-ASCII character (?i:s) matches
    if ((xl == 'l' && yl == 'l') || (xl == 'v' && yl == 'e') || (xl == 'r' && yl == 'e')) return 2;
    return 0;
}

YB_HD bool pt4_contraction_taken(const PtView &v, uint64_t q, int64_t forced) {
    if (pt4_contraction_len(v, q) == 0) return false;
    if (pt_text_start(v, q, forced)) return true;
    const uint64_t p = pt4_prev(v, q);
    const uint8_t pc = v.M(p) & PT_CLS;
    return pc == PT_L || pc == PT_N || (pc == PT_S && v.T(p) != ' ');
}

// THE rule: 0, 1 or PT4_PENDING for byte j.  forced: -1, or the end of a taken special (a text start).  DEPTH 1 is the one
// call rule 3 makes for the O character in front of a letter; it never asks again (no recursion on the device).
template <int DEPTH>
YB_HD uint8_t pt4_is_start_t(const PtView &v, uint64_t j, int64_t forced) {
    if (v.M(j) & PT_CONT) return 0;
    if (pt_text_start(v, j, forced)) return 1;
    // rule 1: j - 1 exists and belongs to this text
    if (pt4_contraction_taken(v, j - 1, forced)) return 0; // first byte of the suffix
    if (j >= 2 && !pt_text_start(v, j - 1, forced)) {
        if (pt4_contraction_taken(v, j - 2, forced)) return pt4_contraction_len(v, j - 2) == 1 ? 1 : 0;
        if (j >= 3 && !pt_text_start(v, j - 2, forced) && pt4_contraction_taken(v, j - 3, forced) && pt4_contraction_len(v, j - 3) == 2)
            return 1;
    }
    const uint64_t p = pt4_prev(v, j);
    const uint8_t c = v.M(j) & PT_CLS, pc = v.M(p) & PT_CLS, pb = v.T(p);
    if (c == PT_N) return pc != PT_N;
    if (c == PT_L) {
        if (pc == PT_L) return 0;
        if (pc == PT_N) return 1;
        if (pc == PT_S) return pt4_is_nl(pb);
        if constexpr (DEPTH == 0) return pt4_is_start_t<1>(v, p, forced) ? 0 : 1;
        return 0; // (not reached: DEPTH 1 is called for an O character)
    }
    if (c == PT_O) return !(pc == PT_O || pb == ' ');
    if (pt4_is_nl(v.T(j))) return pc == PT_L || pc == PT_N;
    if (pc != PT_S) return 1;
    if (!pt4_is_nl(pb)) {
        const uint64_t nx = j + (uint64_t)pt_char_len(v, j);
        return pt4_exists(v, nx) && (v.M(nx) & PT_CLS) != PT_S;
    }
    return PT4_PENDING;
}

YB_HD uint8_t pt4_is_start(const PtView &v, uint64_t j, int64_t forced) { return pt4_is_start_t<0>(v, j, forced); }

// ---------------------------------------------------------------- special tokens (training pattern)
// As pt_special_is_head / pt_special_walk, with the reach of this pattern.  What the end of a taken special (`cover`, a text
// start) can change: the character AT cover becomes a start; if it is an O character (up to 4 bytes) the letter behind it, at
// cover + 1 .. cover + 4, no longer is one (rule 3); if it is an apostrophe it is taken (rule 1), which decides cover + 1 ..
// cover + 3 -- the character behind a suffix matters only when it is a letter (anything else is a start behind a letter
// anyway), and what follows a letter depends on its class alone.  Nothing at cover + 5 or later asks where the text starts:
// the rules look at the startness of another character only in rule 3, one character back.  So an occurrence at most
// len + 4 bytes behind another belongs to its chain, and the redo covers cover .. cover + 4.  No special begins with \s or
// \p{N} (refused by the caller), so an occurrence is never at a pending position or at a digit-group cut.
constexpr int PT4_REACH = 4;

template <class OccF>
YB_HD bool pt4_special_is_head(const PtView &v, const PtSpecials &sp, OccF occ, uint64_t i) {
    if (v.M(i) & PT_CHUNK0) return true;
    const uint64_t window = (uint64_t)sp.max_len + PT4_REACH;
    for (uint64_t d = 1; d <= window && d <= i; ++d) {
        const uint64_t q = i - d;
        const uint32_t o = occ(q);
        if (o && (uint64_t)pt_special_len(sp, o) + PT4_REACH >= d) return false;
        if (v.M(q) & PT_CHUNK0) break;
    }
    return true;
}

template <class OccF>
YB_HD void pt4_special_walk(const PtView &v, const PtSpecials &sp, OccF occ, uint8_t *flags, uint64_t i, uint32_t o0) {
    int64_t cover = -1;
    uint64_t q = i;
    uint32_t oq = o0;
    uint64_t reach = i;
    while (true) {
        const uint32_t len = pt_special_len(sp, oq);
        if (q + len + PT4_REACH > reach) reach = q + len + PT4_REACH;
        bool taken;
        if (cover >= 0 && (int64_t)q < cover) taken = false; // inside the previous match
        else taken = pt4_is_start(v, q, cover >= 0 && (int64_t)q <= cover + PT4_REACH ? cover : -1) == 1;
        if (taken) {
            flags[q] = PT4_FIRST;
            for (uint32_t k = 1; k < len; ++k) flags[q + k] = GRP_INSIDE;
            cover = (int64_t)(q + len);
            for (uint64_t j = (uint64_t)cover; j <= (uint64_t)cover + PT4_REACH && j < v.n; ++j) {
                if (v.M(j) & PT_CHUNK0) break; // the next chunk is a text of its own
                flags[j] = pt4_is_start(v, j, cover);
            }
        }
        uint64_t nq = q + 1;
        uint32_t no = 0;
        for (; nq <= reach && nq < v.n; ++nq) {
            if (v.M(nq) & PT_CHUNK0) break;
            no = occ(nq);
            if (no) break;
        }
        if (!no) return;
        q = nq;
        oq = no;
    }
}

// ---------------------------------------------------------------- the two scans
// A state holds both directions: bits 0-1 the forward value (B), bits 2-3 the backward one (F); 0 keep, 1 set to 0, 2 set to 1.
typedef uint32_t NlState;
constexpr uint32_t NL_KEEP = 0, NL_SET0 = 1, NL_SET1 = 2, NL_MASK = 3, NL_BWD = 2; // NL_BWD: shift of the backward value

YB_HD uint32_t nl_comb(uint32_t a, uint32_t b) { return b ? b : a; } // first a, then b (backward: a is the farther one)

// what one byte does to B, seen by the bytes behind it
YB_HD uint32_t nl_fwd_byte(uint8_t meta, uint8_t flag) {
    if (flag == GRP_INSIDE || flag == PT4_FIRST) return NL_SET0; // a byte of a special is never the O of B
    const bool o = (meta & (PT_CLS | PT_CONT)) == PT_O;
    if (meta & PT_CHUNK0) return o ? NL_SET1 : NL_SET0;          // nothing in front of a text start counts
    if (meta & (PT_CONT | PT4_NL)) return NL_KEEP;
    return o ? NL_SET1 : NL_SET0;
}

// what one byte does to F, seen by the bytes in front of it
YB_HD uint32_t nl_bwd_byte(uint8_t meta, uint8_t flag) {
    if (flag == GRP_INSIDE || flag == PT4_FIRST || (meta & PT_CHUNK0)) return NL_SET0; // another text
    if (meta & PT_CONT) return NL_KEEP;
    if (meta & PT4_NL) return NL_SET1;
    return (meta & PT_CLS) == PT_S ? NL_KEEP : NL_SET0;
}

// One piece of GRP_PIECE bytes as the kernels hold it: four words of meta and four of flags (bytes past the text: meta PT_O,
// flag 0 -- behind every real byte, and "not S" in front of the end).  The per-byte functions above, for 16 bytes at once:
// bit k of a mask belongs to byte k.
struct NlPiece {
    uint32_t f_say, f_one; // forward: the byte is not "keep"; it sets 1
    uint32_t b_say, b_one; // backward
    uint32_t pending;      // flag == PT4_PENDING
};

// bit 0 of every byte of x -> the low four bits
YB_HD uint32_t nl_gather(uint32_t x) {
    x &= 0x01010101u;
    return (x | (x >> 7) | (x >> 14) | (x >> 21)) & 0xFu;
}

YB_HD NlPiece nl_piece(const uint32_t m[4], const uint32_t f[4]) {
    NlPiece p{0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t c0 = m[w], c1 = m[w] >> 1, cont = m[w] >> 2, chunk = m[w] >> 3, nl = m[w] >> 4; // (bit 0 of every byte)
        const uint32_t sp = f[w] >> 1;                 // GRP_INSIDE (2) or PT4_FIRST (3); 0, 1 and PT4_PENDING (4) have no bit 1
        const uint32_t o = c0 & c1 & ~cont, s = ~c0 & c1;
        const uint32_t f_say = sp | chunk | ~(cont | nl), f_one = ~sp & o;
        const uint32_t b_say = sp | chunk | (~cont & (nl | ~s)), b_one = ~sp & ~chunk & ~cont & nl;
        p.f_say |= nl_gather(f_say) << (4 * w);
        p.f_one |= nl_gather(f_one) << (4 * w);
        p.b_say |= nl_gather(b_say) << (4 * w);
        p.b_one |= nl_gather(b_one) << (4 * w);
        p.pending |= nl_gather(f[w] >> 2) << (4 * w);
    }
    return p;
}

// what the piece does to B behind it (bits 0-1) and to F in front of it (bits 2-3): its last / first byte that says something
YB_HD NlState nl_piece_state(const NlPiece &p) {
    const uint32_t f = p.f_say ? (((p.f_one >> (31 - __builtin_clz(p.f_say))) & 1u) ? NL_SET1 : NL_SET0) : NL_KEEP;
    const uint32_t b = p.b_say ? (((p.b_one >> __builtin_ctz(p.b_say)) & 1u) ? NL_SET1 : NL_SET0) : NL_KEEP;
    return f | (b << NL_BWD);
}

// The piece's flags after the pass, in place: PT4_FIRST becomes a start, every PT4_PENDING byte 0 or 1 (rule 6: a start iff
// not F or B).  before: forward value of everything in front of the piece; after: backward value of everything behind it.
YB_HD void nl_piece_flags(uint32_t before, uint32_t after, const NlPiece &p, uint32_t f[4]) {
    uint32_t starts = 0u;
    for (uint32_t todo = p.pending; todo; todo &= todo - 1u) { // (rare: one per whitespace run that follows a newline)
        const int k = __builtin_ctz(todo);
        const uint32_t lo = p.f_say & ((1u << k) - 1u), hi = p.b_say >> (k + 1);
        const bool B = lo ? ((p.f_one >> (31 - __builtin_clz(lo))) & 1u) : before == NL_SET1;
        const bool F = hi ? ((p.b_one >> (k + 1 + __builtin_ctz(hi))) & 1u) : after == NL_SET1;
        if (!F || B) starts |= 1u << k;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t first = f[w] & (f[w] >> 1) & 0x01010101u, pend = (f[w] >> 2) & 0x01010101u; // 3: bits 0 and 1; 4: bit 2
        const uint32_t res = (((starts >> (4 * w)) & 0xFu) * 0x00204081u) & 0x01010101u;           // four bits -> bit 0 of four bytes
        f[w] = ((f[w] ^ (first << 1)) & ~(pend << 2)) | (res & pend);
    }
}
