// split5_logic.h -- the o200k_base split pattern (GPT-4o, o-series, gpt-oss; option "split_pattern" = 3), shared by the HIP
// kernels (k_s5_* / k_la_* / k_fn_* in yabpe_pretok_kernels.h) and by the CPU unit-test model (tests/hostmodel/split5_model.cpp).
//
// What is reproduced: regex.findall with
//     [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?
//     |[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?
//     |\p{N}{1,G}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+
// (training: the special tokens in front of it; encode: after the tokenizer's special split).  The pre-tokens partition the
// text, so one flag per byte describes the result.  Unlike the cl100k pattern no rule here has bounded reach: the case-aware
// word rule backtracks, \p{M} is a word, a punctuation or a prefix character depending on what came before, the contraction
// is a suffix of the word ('s's's alternates) and [\r\n/]* takes slashes behind newlines.  So the pattern is run as what it
// is, a deterministic scanner, and the scanner is run as a parallel scan of state-transition functions.
//
// Classes: U = Lu Lt, l = Ll, B = Lm Lo, M = \p{M}, N = \p{N}, R = CR LF, S = other \s, O = the rest.  W = U l B M.
//
// Look-aheads of unbounded reach, both a backward scan of "keep / set 0 / set 1" over the classes alone (la_byte):
//   F(j)   a character of R occurs later in this whitespace run (as in split4_logic.h)
//   UE(j)  the run of U that starts at j is followed by a character that is not W, or by the end of the text
// Both land in one bit of meta (PT5_LA): F on whitespace, UE on U.  Look-aheads of bounded reach land in the AUX byte that
// the flags array holds until the last pass overwrites it: the class of the next character of this text, and the number of
// suffix letters of a contraction behind an apostrophe.  With them, a character is a function from the scanner's state in
// front of it to the state behind it (s5_step); a continuation byte is the identity and a text start a constant.  A
// function over the 13 states is sixteen nibbles of a uint64_t (s5_fn); functions compose associatively (s5_then), so
// bytes, 16-byte pieces and windows combine in any grouping that keeps the order, and the state in front of every piece
// comes from a three-step scan in the geometry of the digit groups.  The flag of a byte is then s5_step's `start` for the
// state in front of it.
//
// States: S5_S0 at a token boundary; WSR inside \s*[\r\n]+; WSP inside \s+(?!\S); PFX behind the one character in front of
// a word; WU / WB / WL inside a word -- the last character was U / it was B or M and no l came since the last U / an l was
// seen; PUNCT inside [^\s\p{L}\p{N}]+; PTAIL inside its [\r\n/]*; N inside a digit run (cut into groups by group_logic.h
// afterwards); SK2 / SK1 two / one suffix letters of a taken contraction still to pass; INS inside a taken special.
//
// Special tokens (training pattern): an occurrence is taken iff the scanner is at a boundary at its first byte.  Its first
// byte carries A5_HEAD, its last A5_LAST (k_s5_special); a head maps the boundary to INS, INS lasts until A5_LAST.  That needs
// occurrences that never overlap, so the caller refuses sets in which they could (s5_specials_check).  The bytes of a taken
// special behind its first get GRP_INSIDE, which the digit-group pass turns into 0.
#pragma once
#include <stdint.h>

#include "group_logic.h"
#include "pretok_logic.h"

// ---------------------------------------------------------------- meta and aux
// meta: bits 0-3 as in pretok_logic.h (PT_CLS, PT_CONT, PT_CHUNK0), then
enum : uint8_t {
    PT5_NL = 16,       // the byte is U+000A or U+000D
    PT5_SUB = 0x60,    // two bits whose meaning depends on the class:
    PT5_SUB_SHIFT = 5, //   L: 1 = U, 2 = l, 0 = B;  O: 3 = M, 1 = U+002F;  S: 1 = U+0020
    PT5_LA = 0x80,     // F(j) on a whitespace character, UE(j) on a U character
};
// the class table of this pattern: unicode_classes.inc | unicode_subclasses.inc << PT5_SUB_SHIFT, then U+0020 and U+002F
YB_HD uint8_t pt5_table_entry(uint32_t cp, uint8_t cls, uint8_t sub) {
    if (cp == 0x20 || cp == 0x2F) sub = 1;
    return (uint8_t)(cls | (sub << PT5_SUB_SHIFT) | (cp == 0x0A || cp == 0x0D ? PT5_NL : 0));
}

enum : uint8_t { C5_U, C5_l, C5_B, C5_M, C5_N, C5_R, C5_S, C5_O };

YB_HD uint8_t s5_class(uint8_t meta) {
    const uint8_t sub = (meta & PT5_SUB) >> PT5_SUB_SHIFT;
    switch (meta & PT_CLS) {
    case PT_L: return sub == 1 ? C5_U : sub == 2 ? C5_l : C5_B;
    case PT_N: return C5_N;
    case PT_S: return (meta & PT5_NL) ? C5_R : C5_S;
    default: return sub == 3 ? C5_M : C5_O;
    }
}
YB_HD bool s5_is_w(uint8_t c) { return c <= C5_M; }

// aux (in the flags array between k_s5_aux and k_fn_apply)
enum : uint8_t {
    A5_HEAD = 1,       // first byte of an occurrence of a special
    A5_LAST = 2,       // its last byte
    A5_NEXT_SHIFT = 2, // three bits: the next character of this text
    A5_NEXT = 7 << 2,
    A5_CLEN_SHIFT = 5, // two bits: an apostrophe with 1 or 2 suffix letters behind it in this text
    A5_CLEN = 3 << 5,
};
enum : uint8_t { NX_NONE, NX_W, NX_O, NX_RS, NX_N }; // no next character / W / O / R or S / N

// Contraction suffix behind an apostrophe at q, in CHARACTERS: 1 (s S U+017F d D m M t T), 2 ([lL][lL] [vV][eE] [rR][eE]), 0.
YB_HD int s5_clen(const PtView &v, uint64_t q) {
    auto exists = [&](uint64_t j) { return j < v.n && !(v.M(j) & PT_CHUNK0); };
    if (v.T(q) != '\'' || !exists(q + 1)) return 0;
    const uint8_t x = v.T(q + 1), xl = (uint8_t)(x | 0x20);
    if (xl == 's' || xl == 'd' || xl == 'm' || xl == 't') return 1;
    if (!exists(q + 2)) return 0;
    const uint8_t y = v.T(q + 2), yl = (uint8_t)(y | 0x20);
    if (x == 0xC5 && y == 0xBF) return 1; // U+017F, the one non-ASCII character (?i:s) matches
    if ((xl == 'l' && yl == 'l') || (xl == 'v' && yl == 'e') || (xl == 'r' && yl == 'e')) return 2;
    return 0;
}

// the aux byte of j without the special marks (v.meta: final classes; valid text)
YB_HD uint8_t s5_aux(const PtView &v, uint64_t j) {
    if (v.M(j) & PT_CONT) return 0;
    const int len = pt_lead_len(v.T(j));
    const uint64_t nx = j + (uint64_t)(len ? len : 1);
    uint8_t next = NX_NONE;
    if (nx < v.n && !(v.M(nx) & PT_CHUNK0)) {
        const uint8_t c = s5_class(v.M(nx));
        next = s5_is_w(c) ? NX_W : c == C5_N ? NX_N : c == C5_O ? NX_O : NX_RS;
    }
    return (uint8_t)((next << A5_NEXT_SHIFT) | (s5_clen(v, j) << A5_CLEN_SHIFT));
}

// ---------------------------------------------------------------- the two look-aheads: one backward scan
// A value holds F in bits 0-1 and UE in bits 2-3, each 0 keep, 1 set to 0, 2 set to 1.
constexpr uint32_t LA_KEEP = 0, LA_SET0 = 1, LA_SET1 = 2, LA_UE = 2; // LA_UE: shift of the UE value

// a: the bytes farther behind, b: the nearer ones
YB_HD uint32_t la_comb(uint32_t a, uint32_t b) { return ((b & 3u) ? (b & 3u) : (a & 3u)) | ((b & 12u) ? (b & 12u) : (a & 12u)); }

// what one byte does to F and UE of the bytes in front of it
YB_HD uint32_t la_byte(uint8_t meta) {
    if (meta & PT_CHUNK0) return LA_SET0 | (LA_SET1 << LA_UE); // another text: the run and the text end here
    if (meta & PT_CONT) return LA_KEEP;
    const uint8_t c = s5_class(meta);
    const uint32_t f = c == C5_R ? LA_SET1 : c == C5_S ? LA_KEEP : LA_SET0;
    const uint32_t ue = c == C5_U ? LA_KEEP : s5_is_w(c) ? LA_SET0 : LA_SET1;
    return f | (ue << LA_UE);
}

// PT5_LA of a byte; after: everything behind it combined (the end of the text keeps: F is 0 there and UE is 1)
YB_HD uint8_t la_bit(uint8_t meta, uint32_t after) {
    if (meta & PT_CONT) return 0;
    const uint8_t c = s5_class(meta);
    if (c == C5_R || c == C5_S) return (after & 3u) == LA_SET1 ? PT5_LA : 0;
    if (c == C5_U) return ((after >> LA_UE) & 3u) != LA_SET0 ? PT5_LA : 0;
    return 0;
}

// One piece of GRP_PIECE meta bytes (bytes past the text: PT_O).  What it does to the bytes in front of it:
YB_HD uint32_t la_piece_state(const uint32_t m[4]) {
    uint32_t s = LA_KEEP;
#pragma unroll
    for (int k = GRP_PIECE - 1; k >= 0; --k) s = la_comb(s, la_byte((uint8_t)(m[k >> 2] >> ((k & 3) * 8))));
    return s;
}
// its meta with PT5_LA set, in place; after: everything behind the piece
YB_HD void la_piece_bits(uint32_t after, uint32_t m[4]) {
    uint32_t s = after;
#pragma unroll
    for (int k = GRP_PIECE - 1; k >= 0; --k) {
        const uint8_t b = (uint8_t)(m[k >> 2] >> ((k & 3) * 8));
        m[k >> 2] |= (uint32_t)la_bit(b, s) << ((k & 3) * 8);
        s = la_comb(s, la_byte(b));
    }
}

// ---------------------------------------------------------------- the scanner
enum : uint8_t { S5_S0, S5_WSR, S5_WSP, S5_PFX, S5_WU, S5_WB, S5_WL, S5_PUNCT, S5_PTAIL, S5_N, S5_SK1, S5_SK2, S5_INS, S5_NSTATES };

// the state behind a character at which a token starts
YB_HD uint8_t s5_boundary(uint8_t meta, uint8_t aux) {
    if (aux & A5_HEAD) return (aux & A5_LAST) ? S5_S0 : S5_INS; // the special is taken
    const uint8_t c = s5_class(meta), next = (aux & A5_NEXT) >> A5_NEXT_SHIFT, sub = (meta & PT5_SUB) >> PT5_SUB_SHIFT;
    if (c == C5_U) return S5_WU;
    if (c == C5_l) return S5_WL;
    if (c == C5_B || c == C5_M) return S5_WB;
    if (c == C5_N) return S5_N;
    if (c != C5_R && next == NX_W) return S5_PFX;                // the one character in front of a word
    if (c == C5_S && sub == 1 && next == NX_O) return S5_PUNCT;  // " ?" of the punctuation rule
    if (c == C5_O) return S5_PUNCT;
    if (c == C5_R || (meta & PT5_LA)) return S5_WSR;             // \s*[\r\n]+ up to the run's last R
    if (next == NX_RS) return S5_WSP;                            // \s+(?!\S)
    return S5_S0;                                                // one whitespace character alone
}

// THE rule: the state behind byte j for the state s in front of it, and whether a pre-token starts at j.
YB_HD uint8_t s5_step(uint8_t s, uint8_t meta, uint8_t aux, bool *start) {
    *start = false;
    if (meta & PT_CHUNK0) { // a text of its own starts here
        *start = true;
        return s5_boundary(meta, aux);
    }
    if (s == S5_INS) return (aux & A5_LAST) ? S5_S0 : S5_INS;
    if (meta & PT_CONT) return s;
    if (s == S5_SK2) return S5_SK1;
    if (s == S5_SK1) return S5_S0;
    const uint8_t c = s5_class(meta), next = (aux & A5_NEXT) >> A5_NEXT_SHIFT;
    switch (s) {
    case S5_WSR:
        if (c == C5_R || (c == C5_S && (meta & PT5_LA))) return S5_WSR;
        break;
    case S5_WSP:
        if (next == NX_RS || next == NX_NONE) return S5_WSP; // (the last character of the run in front of a \S is a start)
        break;
    case S5_PFX:
        if (s5_is_w(c)) return c == C5_U ? S5_WU : c == C5_l ? S5_WL : S5_WB;
        break;
    case S5_WU:
    case S5_WB:
    case S5_WL:
        if (c == C5_U) {
            if (s == S5_WL || (s == S5_WB && (meta & PT5_LA))) break; // the word ends in front of this upper-case run
            return S5_WU;
        }
        if (c == C5_l) return S5_WL;
        if (c == C5_B || c == C5_M) return s == S5_WL ? S5_WL : S5_WB;
        if (aux & A5_CLEN) return ((aux & A5_CLEN) >> A5_CLEN_SHIFT) == 1 ? S5_SK1 : S5_SK2; // 's belongs to the word
        break;
    case S5_PUNCT:
        if (c == C5_O || c == C5_M) return S5_PUNCT;
        if (c == C5_R) return S5_PTAIL;
        break;
    case S5_PTAIL:
        if (c == C5_R || (c == C5_O && (meta & PT5_SUB) >> PT5_SUB_SHIFT == 1)) return S5_PTAIL;
        break;
    case S5_N:
        if (c == C5_N) return S5_N;
        break;
    default: break; // S5_S0
    }
    *start = true;
    return s5_boundary(meta, aux);
}

// the flag k_fn_apply writes: 0, 1, or GRP_INSIDE on the bytes of a taken special behind its first
YB_HD uint8_t s5_flag(uint8_t s, uint8_t meta, uint8_t aux) {
    bool start;
    (void)s5_step(s, meta, aux, &start);
    return start ? 1 : s == S5_INS ? GRP_INSIDE : 0;
}

// ---------------------------------------------------------------- functions over the states
typedef unsigned long long S5Fn; // nibble s: the state behind, for the state s in front
constexpr S5Fn S5_IDENTITY = 0xFEDCBA9876543210ull;

YB_HD uint8_t s5_apply(S5Fn f, uint8_t s) { return (uint8_t)((f >> (4 * s)) & 15u); }

// first f, then g
YB_HD S5Fn s5_then(S5Fn f, S5Fn g) {
    S5Fn r = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) r |= ((g >> (4 * ((f >> (4 * s)) & 15u))) & 15ull) << (4 * s);
    return r;
}

// one byte as a function (the nibbles past the last state keep themselves)
YB_HD S5Fn s5_fn(uint8_t meta, uint8_t aux) {
    S5Fn r = S5_IDENTITY & ~((1ull << (4 * S5_NSTATES)) - 1ull);
    bool start;
#pragma unroll
    for (int s = 0; s < S5_NSTATES; ++s) r |= (S5Fn)s5_step((uint8_t)s, meta, aux, &start) << (4 * s);
    return r;
}

// One piece of GRP_PIECE bytes: four words of meta and four of aux (bytes past the text: meta PT_O, aux 0), taken word by
// word.
YB_HD S5Fn s5_word_fn(S5Fn f, uint32_t m, uint32_t a) { // f, then the four bytes of (m, a) in order
#pragma unroll
    for (int b = 0; b < 4; ++b) f = s5_then(f, s5_fn((uint8_t)(m >> (8 * b)), (uint8_t)(a >> (8 * b))));
    return f;
}
// word w of four, without indexing (a dynamic index would move the words out of the registers)
YB_HD uint32_t s5_word(const uint32_t x[4], int w) { return w == 0 ? x[0] : w == 1 ? x[1] : w == 2 ? x[2] : x[3]; }
YB_HD S5Fn s5_piece_fn(const uint32_t m[4], const uint32_t a[4]) {
    S5Fn f = S5_IDENTITY;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) f = s5_word_fn(f, s5_word(m, w), s5_word(a, w)); // (rolled: four bytes are 52 transitions)
    return f;
}

// the flags of four bytes; *s: the state in front of them, then the state behind them
YB_HD uint32_t s5_word_flags(uint8_t *s, uint32_t m, uint32_t a) {
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint8_t mb = (uint8_t)(m >> (8 * b)), ab = (uint8_t)(a >> (8 * b));
        bool start;
        const uint8_t t = s5_step(*s, mb, ab, &start);
        o |= (uint32_t)(start ? 1 : *s == S5_INS ? GRP_INSIDE : 0) << (8 * b);
        *s = t;
    }
    return o;
}
// the piece's flags, over its aux words in place; before: the state in front of its first byte
YB_HD void s5_piece_flags(uint8_t before, const uint32_t m[4], uint32_t a[4]) {
    uint8_t s = before;
    a[0] = s5_word_flags(&s, m[0], a[0]);
    a[1] = s5_word_flags(&s, m[1], a[1]);
    a[2] = s5_word_flags(&s, m[2], a[2]);
    a[3] = s5_word_flags(&s, m[3], a[3]);
}

// ---------------------------------------------------------------- special tokens (training pattern)
// Occurrences must never overlap (a taken one is passed in the state INS, which ends at the next A5_LAST).  Refused therefore:
// a special that contains another one, and a special with a proper suffix that is a prefix of a special, itself included
// (equal specials are one special).  Returns 0 when the set is fine, else 1 (contains) or 2 (suffix / prefix) with the two
// specials in *a and *b.  Host code: the caller also refuses a first character of \s or \p{N}, as with cl100k.
inline int s5_specials_check(const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t *a, uint32_t *b) {
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j) {
            const uint8_t *x = bytes + off[i], *y = bytes + off[j];
            const uint32_t lx = off[i + 1] - off[i], ly = off[j + 1] - off[j];
            *a = i;
            *b = j;
            bool same = lx == ly;
            for (uint32_t k = 0; same && k < lx; ++k) same = x[k] == y[k];
            if (same) {
                if (i != j) continue;
            } else if (ly <= lx) { // y inside x
                for (uint32_t p = 0; p + ly <= lx; ++p) {
                    bool eq = true;
                    for (uint32_t k = 0; eq && k < ly; ++k) eq = x[p + k] == y[k];
                    if (eq) return 1;
                }
            }
            for (uint32_t len = 1; len < lx && len <= ly; ++len) { // the last len bytes of x begin y
                bool eq = true;
                for (uint32_t k = 0; eq && k < len; ++k) eq = x[lx - len + k] == y[k];
                if (eq) return 2;
            }
        }
    return 0;
}
