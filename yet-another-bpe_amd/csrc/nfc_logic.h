// nfc_logic.h -- Unicode NFC normalisation: the rules, shared by the HIP kernels (yabpe_norm_kernels.h) and by the CPU
// unit-test model (tests/hostmodel/nfc_model.cpp).  Reference: unicodedata.normalize("NFC", part) of CPython, whose tables
// tools/gen_unicode_norm.py writes into unicode_norm.inc.
//
// NFC has no bounded reach: a run of combining marks is reordered and composed as a whole.  What makes it parallel:
//   segment   starts at every code point with ccc = 0 and quick-check Yes, and at every part start.  NFC of a part is the
//             concatenation of the NFC of its segments: such a code point is a starter that no decomposition touches and that
//             never is the second operand of a composition, so nothing in front of it can reach past it.
//   clean     NFC leaves a segment as it is iff it holds no code point with quick-check No or Maybe and no adjacent pair with
//             ccc(prev) > ccc(cur) > 0 (UAX #15 section 9, the quick check).  Both tests look at one code point and the one
//             before it: "suspect" is a per-byte predicate (NFC_SUSPECT on lead bytes).
//   dirty     a segment that holds a suspect.  All of it is normalised as UAX #15 says, the tail behind its last suspect
//             included: canonical decomposition, a stable sort of every run of non-starters by ccc, canonical composition.
// The device finds for every suspect the start of its segment with an inclusive max-scan of the segment-start positions (a
// state per 16-byte piece and per window, the three steps of group_logic.h), so no lane ever walks a clean segment and none
// walks backwards; one lane (nfc_segment) then walks each dirty segment forward.
//
// Meta byte per text byte: NFC_CONT on continuation bytes; on lead bytes NFC_START (a segment starts here) and NFC_SUSPECT.
// The part starts come in an array of their own (NFC_PART0 marks), as the chunk marks of the pre-tokeniser do.
#pragma once
#include <stdint.h>

#include "pretok_logic.h"

enum : uint8_t { NFC_START = 1, NFC_SUSPECT = 2, NFC_CONT = PT_CONT, NFC_PART0 = PT_CHUNK0 };
enum : uint32_t { NFC_QC_YES = 0, NFC_QC_MAYBE = 1, NFC_QC_NO = 2 };

constexpr uint32_t NFC_FIRST = 0x300;        // every code point below it has ccc 0 and quick-check Yes (the table is not read)
constexpr uint32_t NFC_FIRST_DECOMP = 0xC0;  // ... and every one below this has no decomposition (both checked by the tests)
constexpr int NFC_PIECE = 16;           // bytes one thread owns in the scan passes
constexpr int NFC_WIN = 4096;           // bytes per workgroup and iteration (PT_WIN)
constexpr uint32_t NFC_SHORT = 32;      // decomposed code points a per-lane buffer holds; longer non-starter runs are counting-sorted
constexpr uint32_t NFC_CAP = 16384;     // input code points of one dirty segment: more is YABPE_E_CAPACITY
constexpr uint32_t NFC_MAX_DECOMP = 4;  // code points of the longest canonical decomposition

constexpr uint32_t NFC_SBASE = 0xAC00, NFC_LBASE = 0x1100, NFC_VBASE = 0x1161, NFC_TBASE = 0x11A7;
constexpr uint32_t NFC_LCOUNT = 19, NFC_VCOUNT = 21, NFC_TCOUNT = 28, NFC_NCOUNT = NFC_VCOUNT * NFC_TCOUNT, NFC_SCOUNT = NFC_LCOUNT * NFC_NCOUNT;

struct NfcTables {
    const uint16_t *prop;    // per code point (0x110000 entries): ccc | quick-check << 8
    const uint32_t *decomp;  // n_decomp rows {code point, d0, d1, d2, d3}, sorted
    const uint32_t *pairs;   // n_pairs rows {first, second, composite}, sorted
    uint32_t n_decomp, n_pairs;
};

YB_HD uint32_t nfc_prop(const NfcTables &T, uint32_t cp) { return cp < NFC_FIRST ? 0u : T.prop[cp]; }
YB_HD uint32_t nfc_ccc(uint32_t prop) { return prop & 0xFFu; }
YB_HD uint32_t nfc_qc(uint32_t prop) { return prop >> 8; }
YB_HD bool nfc_prop_starts(uint32_t prop) { return prop == 0; }  // ccc 0 and quick-check Yes

// ---------------------------------------------------------------- class pass
// One call per byte: the meta byte, and whether Python's decoder would stop here (pt_classify's rule).  v.meta holds the
// NFC_PART0 marks.  part_end: end of this byte's part when it is closer than 4 bytes, else any value >= i + 4.
YB_HD uint8_t nfc_classify(const PtView &v, uint64_t i, uint64_t part_end, const NfcTables &T, bool *bad) {
    if ((v.T(i) & 0xC0) == 0x80) {
        (void)pt_classify(v, i, part_end, nullptr, bad);  // (a continuation byte never reaches the class table)
        return NFC_CONT;
    }
    uint32_t cp = 0;
    *bad = pt_decode(v, i, part_end, &cp) == 0;
    if (*bad) return 0;
    if (cp < NFC_FIRST) return NFC_START;
    const bool part0 = (v.M(i) & NFC_PART0) != 0;
    const uint32_t p = T.prop[cp], cc = nfc_ccc(p);
    bool suspect = nfc_qc(p) != NFC_QC_YES;
    if (!suspect && cc && !part0) {  // the code point in front of it (malformed text is reported, not followed: 3 steps at most)
        uint64_t j = i - 1;
        for (int k = 0; k < 3 && j > 0 && (v.T(j) & 0xC0) == 0x80 && !(v.M(j) & NFC_PART0); ++k) --j;
        uint32_t pc = 0;
        if (pt_decode(v, j, i, &pc) != 0) suspect = nfc_ccc(nfc_prop(T, pc)) > cc;
    }
    return (uint8_t)((part0 || nfc_prop_starts(p) ? NFC_START : 0) | (suspect ? NFC_SUSPECT : 0));
}

// ---------------------------------------------------------------- suspects -> dirty segment starts
// State of a stretch of bytes: 1 + the position of its last segment start, 0 when it holds none.
typedef uint64_t NfcPos;
YB_HD NfcPos nfc_combine(NfcPos a, NfcPos b) { return b ? b : a; }  // first a, then b

// get(k) = meta of byte g + k (0 past the text)
template <class Get>
YB_HD NfcPos nfc_piece_state(Get get, uint64_t g) {
    NfcPos s = 0;
#pragma unroll
    for (int k = 0; k < NFC_PIECE; ++k)
        if (get(k) & NFC_START) s = g + (uint64_t)k + 1;
    return s;
}

// mark(p) for every suspect of the piece, p = the start of its segment; `before` = the state in front of the piece
template <class Get, class Mark>
YB_HD void nfc_piece_mark(NfcPos before, Get get, uint64_t g, Mark mark) {
    NfcPos s = before;
#pragma unroll
    for (int k = 0; k < NFC_PIECE; ++k) {
        const uint8_t m = get(k);
        if (m & NFC_START) s = g + (uint64_t)k + 1;
        if ((m & NFC_SUSPECT) && s) mark(s - 1);
    }
}

// ---------------------------------------------------------------- code points
// full canonical decomposition of cp into out (at most NFC_MAX_DECOMP code points); returns how many
YB_HD int nfc_decompose(const NfcTables &T, uint32_t cp, uint32_t *out) {
    out[0] = cp;
    if (cp < NFC_FIRST_DECOMP) return 1;
    if (cp - NFC_SBASE < NFC_SCOUNT) {
        const uint32_t s = cp - NFC_SBASE, t = s % NFC_TCOUNT;
        out[0] = NFC_LBASE + s / NFC_NCOUNT;
        out[1] = NFC_VBASE + (s % NFC_NCOUNT) / NFC_TCOUNT;
        out[2] = NFC_TBASE + t;
        return t ? 3 : 2;
    }
    uint32_t lo = 0, hi = T.n_decomp;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (T.decomp[mid * 5] < cp) lo = mid + 1;
        else hi = mid;
    }
    if (lo == T.n_decomp || T.decomp[lo * 5] != cp) return 1;
    int n = 0;
    for (; n < (int)NFC_MAX_DECOMP && T.decomp[lo * 5 + 1 + n]; ++n) out[n] = T.decomp[lo * 5 + 1 + n];
    return n;
}

// the primary composite of (a, b), 0 when there is none
YB_HD uint32_t nfc_compose_pair(const NfcTables &T, uint32_t a, uint32_t b) {
    if (a - NFC_LBASE < NFC_LCOUNT && b - NFC_VBASE < NFC_VCOUNT) return NFC_SBASE + ((a - NFC_LBASE) * NFC_VCOUNT + (b - NFC_VBASE)) * NFC_TCOUNT;
    if (a - NFC_SBASE < NFC_SCOUNT && (a - NFC_SBASE) % NFC_TCOUNT == 0 && b - (NFC_TBASE + 1) < NFC_TCOUNT - 1) return a + (b - NFC_TBASE);
    if (b < NFC_FIRST) return 0;  // (every second operand is Maybe)
    uint32_t lo = 0, hi = T.n_pairs;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        const uint32_t pa = T.pairs[mid * 3], pb = T.pairs[mid * 3 + 1];
        if (pa < a || (pa == a && pb < b)) lo = mid + 1;
        else hi = mid;
    }
    return lo < T.n_pairs && T.pairs[lo * 3] == a && T.pairs[lo * 3 + 1] == b ? T.pairs[lo * 3 + 2] : 0u;
}

YB_HD uint32_t nfc_utf8_len(uint32_t cp) { return cp < 0x80 ? 1u : cp < 0x800 ? 2u : cp < 0x10000 ? 3u : 4u; }
YB_HD uint32_t nfc_utf8_put(uint32_t cp, uint8_t *o) {
    if (cp < 0x80) {
        o[0] = (uint8_t)cp;
        return 1;
    }
    if (cp < 0x800) {
        o[0] = (uint8_t)(0xC0 | cp >> 6);
        o[1] = (uint8_t)(0x80 | (cp & 0x3F));
        return 2;
    }
    if (cp < 0x10000) {
        o[0] = (uint8_t)(0xE0 | cp >> 12);
        o[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
        o[2] = (uint8_t)(0x80 | (cp & 0x3F));
        return 3;
    }
    o[0] = (uint8_t)(0xF0 | cp >> 18);
    o[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
    o[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
    o[3] = (uint8_t)(0x80 | (cp & 0x3F));
    return 4;
}

// ---------------------------------------------------------------- one dirty segment
// A buffer entry is code point | ccc << 24.  Buf: get(i) / set(i, e) over `cap` entries -- a lane's slice of LDS (NfcLaneBuf in
// the kernels) or global scratch (a plain pointer wrapped the same way).
YB_HD uint32_t nfc_ent_ccc(uint32_t e) { return e >> 24; }
YB_HD uint32_t nfc_ent_cp(uint32_t e) { return e & 0xFFFFFFu; }

struct NfcSeg {
    uint64_t end;     // first byte behind the segment
    uint32_t in_cps;  // input code points walked (NFC_CAP + 1: the walk stopped there, the segment is over the cap)
    uint32_t n_ent;   // decomposed code points (all of them, also those that did not fit into the buffer)
};

// Walks the segment that starts at byte s forward to the next segment start or the end of the text, and leaves its canonical
// decomposition in buf (what fits into cap entries).  v.meta: the meta bytes (every part start carries NFC_START); valid UTF-8.
template <class Buf>
YB_HD NfcSeg nfc_seg_fill(const NfcTables &T, const PtView &v, uint64_t s, Buf &buf, uint32_t cap) {
    NfcSeg r{s, 0, 0};
    do {
        uint32_t cp = 0, d[NFC_MAX_DECOMP];
        const int len = pt_decode(v, r.end, v.n, &cp);
        const int nd = nfc_decompose(T, cp, d);
        for (int k = 0; k < nd; ++k) {
            if (r.n_ent < cap) buf.set(r.n_ent, d[k] | nfc_ccc(nfc_prop(T, d[k])) << 24);
            ++r.n_ent;
        }
        ++r.in_cps;
        r.end += (uint64_t)(len ? len : 1);
    } while (r.end < v.n && !(v.M(r.end) & NFC_START) && r.in_cps <= NFC_CAP);
    return r;
}

// stable insertion sort of entries [lo, hi) by ccc; a starter (ccc 0) is never passed, so runs of non-starters sort on their own
template <class Buf>
YB_HD void nfc_sort_insert(Buf &buf, uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo + 1; i < hi; ++i) {
        const uint32_t e = buf.get(i), cc = nfc_ent_ccc(e);
        if (!cc) continue;
        uint32_t j = i;
        for (; j > lo && nfc_ent_ccc(buf.get(j - 1)) > cc; --j) buf.set(j, buf.get(j - 1));
        if (j != i) buf.set(j, e);
    }
}

// The same order at any length in linear time: runs of non-starters of up to NFC_SHORT entries by insertion (a bounded number
// of steps per entry), longer ones by a counting sort over the 255 classes through tmp (n entries) and cnt (256 counters).
template <class Buf, class Tmp>
YB_HD void nfc_sort_long(Buf &buf, Tmp &tmp, uint32_t n, uint32_t *cnt) {
    uint32_t i = 0;
    while (i < n) {
        if (!nfc_ent_ccc(buf.get(i))) {
            ++i;
            continue;
        }
        uint32_t r = i;
        while (r < n && nfc_ent_ccc(buf.get(r))) ++r;
        if (r - i <= NFC_SHORT) {
            nfc_sort_insert(buf, i, r);
        } else {
            for (uint32_t k = 0; k < 256; ++k) cnt[k] = 0;
            for (uint32_t k = i; k < r; ++k) ++cnt[nfc_ent_ccc(buf.get(k))];
            uint32_t run = i;
            for (uint32_t k = 1; k < 256; ++k) {
                const uint32_t c = cnt[k];
                cnt[k] = run;
                run += c;
            }
            for (uint32_t k = i; k < r; ++k) {
                const uint32_t e = buf.get(k);
                tmp.set(cnt[nfc_ent_ccc(e)]++, e);
            }
            for (uint32_t k = i; k < r; ++k) buf.set(k, tmp.get(k));
        }
        i = r;
    }
}

// Canonical composition of the n sorted entries in place (UAX #15: a code point composes with the last starter unless a code
// point of equal or higher ccc stands uncomposed between them; adjacent starters compose too); returns how many are left.
template <class Buf>
YB_HD uint32_t nfc_compose(const NfcTables &T, Buf &buf, uint32_t n) {
    if (n == 0) return 0;
    uint32_t starter_pos = 0, starter = nfc_ent_cp(buf.get(0)), last_cc = nfc_ent_ccc(buf.get(0)), out = 1;
    if (last_cc) last_cc = 256;  // the segment begins with a mark (a part start): nothing composes with it
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t e = buf.get(i), cp = nfc_ent_cp(e), cc = nfc_ent_ccc(e);
        const uint32_t comp = (last_cc < cc || last_cc == 0) ? nfc_compose_pair(T, starter, cp) : 0u;
        if (comp) {
            starter = comp;
            buf.set(starter_pos, comp);  // (a primary composite of a starter is a starter: ccc 0)
        } else {
            if (cc == 0) {
                starter_pos = out;
                starter = cp;
            }
            last_cc = cc;
            buf.set(out++, e);
        }
    }
    return out;
}

// UTF-8 of the n entries: their length, written to out when it is not NULL
template <class Buf>
YB_HD uint64_t nfc_emit(Buf &buf, uint32_t n, uint8_t *out) {
    uint64_t len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t cp = nfc_ent_cp(buf.get(i));
        len += out ? nfc_utf8_put(cp, out + len) : nfc_utf8_len(cp);
    }
    return len;
}

// ---------------------------------------------------------------- copy pass
// first index in [lo, hi) with a[index] >= x (hi when there is none)
YB_HD uint64_t nfc_lower_bound(const unsigned long long *a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Where byte i of the input goes: *k = the number of dirty segments that start at or before i (the caller keeps it between
// calls with ascending i; it starts at any lower bound).  Returns false for a byte inside a dirty segment (the segment writes
// its own bytes), else true and *dst = i + shift[*k], shift[k] = what segments 0 .. k - 1 grew by (mod 2^64).
YB_HD bool nfc_copy_dst(const unsigned long long *dstart, const unsigned long long *dend, const unsigned long long *shift, uint64_t n_dirty,
                        uint64_t i, uint64_t *k, uint64_t *dst) {
    while (*k < n_dirty && dstart[*k] <= i) ++*k;
    if (*k && i < dend[*k - 1]) return false;
    *dst = i + shift[*k];
    return true;
}
