// utf8_logic.h -- the rules of bytes.decode("utf-8", errors="replace" | "ignore").encode() on raw text cut into parts, shared by
// the HIP kernels (yabpe_utf8_kernels.h) and by the CPU unit-test model (tests/hostmodel/utf8_model.cpp).
//
// The UTF-8 tables are decode_logic.h's and stay there: dec_out_len charges byte p of a document [ds, de) 1 (copied), 3 (it
// starts a maximal subpart of an ill-formed sequence) or 0 (a continuation byte inside such a subpart).  What this header adds:
//   mode     "replace" writes what dec_out_len charges (EF BF BD for every subpart); "ignore" charges 0 where it charges 3 --
//            the two handlers of CPython act on identical ranges.
//   parts    a part (a training chunk, an encode document) is a text of its own: the look-back and the look-ahead of a byte
//            are clipped to its part, so a sequence cut off by a part's end is ill-formed there and never joins the next part.
//            The part starts come as a mark per byte (non-zero at a part's first byte), as the chunk marks of the
//            pre-tokeniser do; the rules look 3 bytes each way, so the part of byte p is only known as far as that:
//            [max(its start, p - 3), min(its end, p + 4)) -- which is all dec_out_len asks about.
#pragma once
#include <stdint.h>

#include "decode_logic.h"

constexpr uint32_t U8_REPLACE = 1, U8_IGNORE = 2;  // YABPE_UTF8_REPLACE, YABPE_UTF8_IGNORE
constexpr int U8_PIECE = 16;                       // bytes a thread takes: an all-ASCII piece is one load and one compare
constexpr int U8_TILE = 4096;                      // bytes a workgroup takes at a time (BLOCK pieces)
constexpr int U8_HALO = 16;                        // bytes of the neighbours a tile keeps on either side (the rules look 3)
constexpr int U8_LOOK = 3;

// Text and part marks seen through an origin (the kernels read an LDS tile): T(j) = text[j - org], M(j) = mark[j - org].
struct U8View {
    const uint8_t *text;
    const uint8_t *mark;  // may be NULL when `marked` is false in the calls below
    uint64_t org;
    YB_HD uint8_t T(uint64_t j) const { return text[j - org]; }
    YB_HD uint8_t M(uint64_t j) const { return mark[j - org]; }
};

// The part of byte p of a text of n bytes as far as the rules look.  marked: some part starts within U8_LOOK bytes of p
// (false: the marks are not read at all).
YB_HD void u8_part(const U8View &v, uint64_t p, uint64_t n, bool marked, uint64_t *ps, uint64_t *pe) {
    const uint64_t lo = p >= (uint64_t)U8_LOOK ? p - U8_LOOK : 0, hi = p + U8_LOOK + 1 < n ? p + U8_LOOK + 1 : n;
    uint64_t s = lo, e = hi;
    if (marked) {
        for (uint64_t q = p;; --q) {
            if (v.M(q)) {
                s = q;
                break;
            }
            if (q == lo) break;
        }
        for (uint64_t q = p + 1; q < hi; ++q)
            if (v.M(q)) {
                e = q;
                break;
            }
    }
    *ps = s;
    *pe = e;
}

// What dec_out_len charges byte p inside its part: 1, 3 or 0 (3 = one subpart to replace or to drop), and in *run the bytes
// from p on that this settles: the lead of a well-formed sequence settles its continuation bytes with it (each is charged 1
// like the lead; a caller may skip them or ask again, the answer is the same), every other byte only itself.
YB_HD uint32_t u8_raw_len(const U8View &v, uint64_t p, uint64_t n, bool marked, uint32_t *run) {
    *run = 1;
    const uint8_t b = v.T(p);
    if (b < 0x80u) return 1;
    uint64_t ps, pe;
    u8_part(v, p, n, marked, &ps, &pe);
    const uint32_t raw = dec_out_len(DecView{v.text, v.org}, p, ps, pe);
    if (raw == 1u && !dec_cont(b)) *run = (uint32_t)dec_need(b);
    return raw;
}

// Output bytes of a byte that dec_out_len charged `raw`, under `mode`.
YB_HD uint32_t u8_charge(uint32_t raw, uint32_t mode) { return raw == 3u && mode == U8_IGNORE ? 0u : raw; }
