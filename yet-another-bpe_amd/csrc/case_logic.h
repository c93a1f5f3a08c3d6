// case_logic.h -- the rules of str.lower() on UTF-8 text cut into parts, shared by the HIP kernels (yabpe_case_kernels.h) and
// by the CPU unit-test model (tests/hostmodel/case_model.cpp).
//
//   map      one entry per code point (unicode_case.inc expanded by case_expand): the lowered code point, whether it is cased
//            or ignorable for the final-sigma rule, and whether U+0307 follows the lowered code point (U+0130 alone).
//   sigma    U+03A3 becomes U+03C2 iff the nearest code point in front of it that is not ignorable is cased and the nearest
//            one behind it that is not ignorable is not cased (or there is none); else U+03C3.  Both lengths are 2 bytes.
//            "The nearest one that is not ignorable" is a scan: a state of three values (nothing yet, cased, not cased) where
//            an ignorable code point is the identity and any other one overrides what was farther away.  A part's start (its
//            end, from behind) counts as "not cased": nothing reaches across it.
//   lengths  a lowered code point may be shorter or longer in UTF-8 than the code point (25 of them); a character belongs to
//            the piece and the window that hold its lead byte.
// Text is valid UTF-8 wherever a function says so: the check pass (case_check_piece) runs first and reports the rest.
// The part starts come as PT_CHUNK0 marks in an array of their own, as the pre-tokeniser's and the normaliser's do; a text
// that is one part comes without the array (case_part_start).
#pragma once
#include <stdint.h>

#include "pretok_logic.h"

constexpr int CASE_PIECE = 16;   // bytes one thread owns
constexpr int CASE_WIN = 4096;   // bytes per workgroup and iteration (SCAN_WIN)
constexpr uint32_t CASE_CP = 0x1FFFFFu, CASE_CASED = 1u << 21, CASE_IGNORABLE = 1u << 22, CASE_TWO = 1u << 23;  // table entry
constexpr uint32_t CASE_SIGMA = 0x3A3, CASE_SIGMA_FINAL = 0x3C2, CASE_SIGMA_SMALL = 0x3C3;
constexpr uint32_t CASE_TWO_CP = 0x130, CASE_TWO_SECOND = 0x307;  // (checked against YB_CASE_TWO by case_expand)
constexpr uint32_t CASE_NCP = 0x110000;

enum : uint32_t { CASE_ST_NONE = 0, CASE_ST_CASED = 1, CASE_ST_OTHER = 2 };  // the final-sigma state

struct CaseTables {
    const uint32_t *tab;  // CASE_NCP entries
};

// unicode_case.inc -> tab[CASE_NCP].  false: the tables do not fit the constants above.
inline bool case_expand(uint32_t *tab, const int (*lower)[4], unsigned n_lower, const unsigned *two, const unsigned (*cased)[2], unsigned n_cased,
                        const unsigned (*ign)[2], unsigned n_ign) {
    for (uint32_t cp = 0; cp < CASE_NCP; ++cp) tab[cp] = cp;
    for (unsigned r = 0; r < n_lower; ++r)
        for (int cp = lower[r][0]; cp <= lower[r][1]; cp += lower[r][2]) tab[cp] = (uint32_t)(cp + lower[r][3]);
    if (two[0] != CASE_TWO_CP || two[2] != CASE_TWO_SECOND || tab[two[0]] != two[0]) return false;
    tab[two[0]] = two[1] | CASE_TWO;
    for (unsigned r = 0; r < n_cased; ++r)
        for (unsigned cp = cased[r][0]; cp <= cased[r][1]; ++cp) tab[cp] |= CASE_CASED;
    for (unsigned r = 0; r < n_ign; ++r)
        for (unsigned cp = ign[r][0]; cp <= ign[r][1]; ++cp) tab[cp] |= CASE_IGNORABLE;
    return (tab[CASE_SIGMA] & CASE_CP) == CASE_SIGMA_SMALL;
}

// ---------------------------------------------------------------- code points
YB_HD uint32_t case_u8len(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }

// the UTF-8 bytes of cp, byte j in bits 8 j
YB_HD uint32_t case_u8pack(uint32_t cp) {
    if (cp < 0x80u) return cp;
    if (cp < 0x800u) return (0xC0u | (cp >> 6)) | (0x80u | (cp & 0x3Fu)) << 8;
    if (cp < 0x10000u) return (0xE0u | (cp >> 12)) | (0x80u | ((cp >> 6) & 0x3Fu)) << 8 | (0x80u | (cp & 0x3Fu)) << 16;
    return (0xF0u | (cp >> 18)) | (0x80u | ((cp >> 12) & 0x3Fu)) << 8 | (0x80u | ((cp >> 6) & 0x3Fu)) << 16 | (0x80u | (cp & 0x3Fu)) << 24;
}

YB_HD bool case_changes(uint32_t e, uint32_t cp) { return (e & (CASE_CP | CASE_TWO)) != cp; }

// output bytes of the code point with entry e (either sigma is 2 bytes)
YB_HD uint32_t case_out_len(uint32_t e) { return case_u8len(e & CASE_CP) + ((e & CASE_TWO) ? 2u : 0u); }

// the lowered character of cp (entry e) as packed bytes, *len of them (at most 4: U+0130 gives 3).  final: cp is a capital
// sigma that the rule makes a final one.
YB_HD uint32_t case_lower_pack(uint32_t e, uint32_t cp, bool final, uint32_t *len) {
    if (e & CASE_TWO) {
        *len = 3;
        return (e & 0x7Fu) | case_u8pack(CASE_TWO_SECOND) << 8;
    }
    const uint32_t low = cp == CASE_SIGMA && final ? CASE_SIGMA_FINAL : (e & CASE_CP);
    *len = case_u8len(low);
    return case_u8pack(low);
}

YB_HD uint32_t case_entry_state(uint32_t e) { return (e & CASE_CASED) ? CASE_ST_CASED : (e & CASE_IGNORABLE) ? CASE_ST_NONE : CASE_ST_OTHER; }

// the same for an ASCII byte without the table: letters are cased, ' . : ^ ` are ignorable (the model test holds it to the table)
YB_HD uint32_t case_ascii_state(uint32_t b) {
    if (((b | 0x20u) - 0x61u) < 26u) return CASE_ST_CASED;
    return (b == 0x27u || b == 0x2Eu || b == 0x3Au || b == 0x5Eu || b == 0x60u) ? CASE_ST_NONE : CASE_ST_OTHER;
}

// first a, then b: b is the nearer one in either direction
YB_HD uint32_t case_combine(uint32_t a, uint32_t b) { return b ? b : a; }

// SWAR over four ASCII bytes: 0x20 in every byte that is 'A'..'Z'
YB_HD uint32_t case_upper_bits4(uint32_t w) {
    const uint32_t ge_a = w + 0x3F3F3F3Fu, gt_z = w + 0x25252525u;  // bit 7 of a byte: >= 'A', > 'Z' (bytes < 0x80: no carry out)
    return ((ge_a & ~gt_z) & 0x80808080u) >> 2;
}

// ---------------------------------------------------------------- valid text: one character
// the character whose lead byte is at i: its code point, *len its bytes
YB_HD uint32_t case_char(const PtView &v, uint64_t i, uint32_t *len) {
    const uint8_t b0 = v.T(i);
    if (b0 < 0x80u) {
        *len = 1;
        return b0;
    }
    if (b0 < 0xE0u) {
        *len = 2;
        return (b0 & 0x1Fu) << 6 | (v.T(i + 1) & 0x3Fu);
    }
    if (b0 < 0xF0u) {
        *len = 3;
        return (b0 & 0x0Fu) << 12 | (v.T(i + 1) & 0x3Fu) << 6 | (v.T(i + 2) & 0x3Fu);
    }
    *len = 4;
    return (b0 & 0x07u) << 18 | (v.T(i + 1) & 0x3Fu) << 12 | (v.T(i + 2) & 0x3Fu) << 6 | (v.T(i + 3) & 0x3Fu);
}

YB_HD bool case_is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// a part starts at byte i.  A text that is one part comes without marks (v.meta == NULL): it starts at byte 0.
YB_HD bool case_part_start(const PtView &v, uint64_t i) { return v.meta ? (v.M(i) & PT_CHUNK0) != 0 : i == 0; }

YB_HD uint32_t case_char_state(const PtView &v, const CaseTables &T, uint64_t i) {
    const uint8_t b = v.T(i);
    if (b < 0x80u) return case_ascii_state(b);
    uint32_t len;
    return case_entry_state(T.tab[case_char(v, i, &len)]);
}

// ---------------------------------------------------------------- check: the piece [g, g + CASE_PIECE) of any text
struct CaseCounts {
    uint64_t bad;      // first malformed byte (~0: none)
    uint32_t changed;  // code points that change
    uint32_t resized;  // ... whose UTF-8 length changes
    uint32_t sigma;    // capital sigmas
    uint32_t out;      // bytes of the lowered characters whose lead byte is in the piece
};

// pt_classify's rule for a continuation byte, in a text that is one part: fine iff a lead byte at most 3 bytes back announces
// a sequence that reaches it.
YB_HD bool case_stray_cont(const PtView &v, uint64_t i) {
    for (int d = 1; d <= 3 && (uint64_t)d <= i; ++d) {
        const uint8_t p = v.T(i - d);
        if (!case_is_cont(p)) return pt_lead_len(p) <= d;
    }
    return true;
}

// v.meta: the PT_CHUNK0 marks (NULL: one part).  Malformed bytes are reported as yabpe_pretokenize reports them (pt_classify, pt_decode).
YB_HD void case_check_piece(const PtView &v, const CaseTables &T, uint64_t g, CaseCounts *c) {
    const uint64_t hi = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    for (uint64_t i = g; i < hi; ++i) {
        const uint8_t b = v.T(i);
        if (b < 0x80u) {
            c->changed += (uint32_t)(b - 0x41u) < 26u;
            ++c->out;
            continue;
        }
        uint64_t end = v.n;
        for (uint64_t q = i + 1; q < i + 4 && q < v.n; ++q)
            if (case_part_start(v, q)) {
                end = q;
                break;
            }
        bool bad = false;
        if (case_is_cont(b)) {
            if (v.meta) (void)pt_classify(v, i, end, nullptr, &bad);
            else bad = case_stray_cont(v, i);
        } else {
            uint32_t cp = 0;
            const int len = pt_decode(v, i, end, &cp);
            bad = len == 0;
            if (!bad) {
                const uint32_t e = T.tab[cp], ol = case_out_len(e);
                if (case_changes(e, cp)) {
                    ++c->changed;
                    c->sigma += cp == CASE_SIGMA;
                    c->resized += ol != (uint32_t)len;
                }
                c->out += ol;
            }
        }
        if (bad && i < c->bad) c->bad = i;
    }
}

// ---------------------------------------------------------------- same size: the piece's 16 output bytes (valid text,
// no code point changes length, no sigma).  Byte g + k of the output in bits 8 k of *lo (k < 8) or 8 (k - 8) of *hi.
YB_HD void case_same_piece(const PtView &v, const CaseTables &T, uint64_t g, uint64_t *lo, uint64_t *hi) {
    const uint64_t top = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    uint64_t i = g, l = 0, h = 0;
    for (int k = 0; k < 3 && i > 0 && case_is_cont(v.T(i)); ++k) --i;  // the character that reaches into the piece
    while (i < top) {
        uint32_t len, ol;
        const uint32_t cp = case_char(v, i, &len);
        const uint32_t pk = cp < 0x80u ? (cp | ((cp - 0x41u) < 26u ? 0x20u : 0u)) : case_lower_pack(T.tab[cp], cp, false, &ol);
        for (uint32_t j = 0; j < len; ++j) {
            const uint64_t p = i + j;
            if (p < g || p >= top) continue;
            const uint64_t x = (uint64_t)((pk >> (8 * j)) & 0xFFu);
            const uint32_t k = (uint32_t)(p - g);
            if (k < 8) l |= x << (8 * k);
            else h |= x << (8 * (k - 8));
        }
        i += len;
    }
    *lo = l;
    *hi = h;
}

// ---------------------------------------------------------------- final sigma (valid text)
// State of the piece [g, g + CASE_PIECE) for what lies behind it: its last code point that is not ignorable, a part start
// behind that code point overriding it.
YB_HD uint32_t case_piece_fwd(const PtView &v, const CaseTables &T, uint64_t g) {
    const uint64_t top = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    for (uint64_t i = top; i-- > g;) {
        if (!case_is_cont(v.T(i))) {
            const uint32_t s = case_char_state(v, T, i);
            if (s) return s;
        }
        if (case_part_start(v, i)) return CASE_ST_OTHER;
    }
    return CASE_ST_NONE;
}

// ... and for what lies in front of it: its first code point that is not ignorable, or a part start before that.
YB_HD uint32_t case_piece_bwd(const PtView &v, const CaseTables &T, uint64_t g) {
    const uint64_t top = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    for (uint64_t i = g; i < top; ++i) {
        if (case_part_start(v, i)) return CASE_ST_OTHER;
        if (!case_is_cont(v.T(i))) {
            const uint32_t s = case_char_state(v, T, i);
            if (s) return s;
        }
    }
    return CASE_ST_NONE;
}

YB_HD bool case_sigma_at(const PtView &v, uint64_t i) { return v.T(i) == 0xCEu && i + 1 < v.n && v.T(i + 1) == 0xA3u; }

// x: the state in front of the piece.  -> bit k: byte g + k leads a capital sigma with a cased code point in front of it.
YB_HD uint32_t case_piece_mark_fwd(const PtView &v, const CaseTables &T, uint64_t g, uint32_t x) {
    const uint64_t top = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    uint32_t mask = 0;
    for (uint64_t i = g; i < top; ++i) {
        if (case_part_start(v, i)) x = CASE_ST_OTHER;
        if (case_is_cont(v.T(i))) continue;
        if (x == CASE_ST_CASED && case_sigma_at(v, i)) mask |= 1u << (uint32_t)(i - g);
        x = case_combine(x, case_char_state(v, T, i));
    }
    return mask;
}

// x: the state behind the piece.  -> mask without the sigmas that a cased code point follows: the final ones.
YB_HD uint32_t case_piece_mark_bwd(const PtView &v, const CaseTables &T, uint64_t g, uint32_t x, uint32_t mask) {
    const uint64_t top = g + CASE_PIECE < v.n ? g + CASE_PIECE : v.n;
    for (uint64_t i = top; i-- > g;) {
        if (!case_is_cont(v.T(i))) {
            if (x == CASE_ST_CASED) mask &= ~(1u << (uint32_t)(i - g));
            x = case_combine(x, case_char_state(v, T, i));
        }
        if (case_part_start(v, i)) x = CASE_ST_OTHER;
    }
    return mask;
}

// ---------------------------------------------------------------- general write (valid text)
// Output bytes of byte i: those of its lowered character at a lead byte, 0 at a continuation byte.
YB_HD uint32_t case_byte_out_len(const PtView &v, const CaseTables &T, uint64_t i) {
    const uint8_t b = v.T(i);
    if (b < 0x80u) return 1;
    if (case_is_cont(b)) return 0;
    uint32_t len;
    return case_out_len(T.tab[case_char(v, i, &len)]);
}

// The lowered character at lead byte i into dst (*len bytes, at most 4).
YB_HD void case_emit(const PtView &v, const CaseTables &T, uint64_t i, bool final, uint8_t *dst, uint32_t *len) {
    uint32_t in_len;
    const uint32_t cp = case_char(v, i, &in_len);
    const uint32_t pk = cp < 0x80u ? (*len = 1, cp | ((cp - 0x41u) < 26u ? 0x20u : 0u)) : case_lower_pack(T.tab[cp], cp, final, len);
    for (uint32_t j = 0; j < *len; ++j) dst[j] = (uint8_t)(pk >> (8 * j));
}
