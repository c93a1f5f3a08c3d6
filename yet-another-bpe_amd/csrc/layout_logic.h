// layout_logic.h -- the index rules of BBPETokenizer.encode_batch_padded / encode_batch_packed (yet_another_bpe/tokenizer.py) on
// flat arrays, shared by the HIP kernels (yabpe_layout_kernels.h) and by the CPU unit-test model (tests/hostmodel/layout_model.cpp).
//
//   seq(d)    [bos] + the document's ids + [eos]; n_added = how many of the two are given; len(seq(d)) = n(d) + n_added.
//   padded    row d holds seq(d) cut to row_len: the content keeps its head (or, LAY_TRUNC_LEFT, its tail), BOS and EOS always
//             survive; the kept sequence sits at the row's left end (or, LAY_PAD_LEFT, at its right end), pad_id elsewhere.
//             Rule 1 (lay_pad_slot): which source id, if any, slot (row, col) holds.
//   packed    all seq(d) end to end, cut into rows of row_len.  The stream offset of document d is the exclusive scan of
//             len(seq(d)); the ids of a call are already laid end to end with their starts in doc_off, so that scan has the
//             closed form soff[d] = doc_off[d] + n_added * d (soff[n_docs] = n_ids + n_added * n_docs).
//             Rule 2 (lay_find_doc / lay_pack_slot): which (doc, pos) a stream position belongs to, given soff.  A document
//             with an empty seq has soff[d] == soff[d + 1] and owns no position: the search takes the LAST d with soff[d] <= g.
//   windows   (encode_batch_windows) with C = row_len - n_added content slots a row and step = C - stride: row k of document d
//             holds [bos] + ids[k * step : k * step + C] + [eos], padded like a padded row; the last row is the first one with
//             k * step + C >= n, so every document owns at least one row and only its last row can be short.
//             Rule 3 (lay_win_rows / lay_win_content / lay_win_slot): how many rows a document has, how many content ids row
//             k keeps, which source id a slot holds.  The first output row of document d is the exclusive scan of the row
//             counts; it ascends strictly, so the document of an output row is Rule 2's search (lay_find_doc) as it is.
//   pairs     (encode_batch_pairs) documents 2p and 2p + 1 are the two sides A, B of pair p; n_added = BOS + EOS + n_sep and C =
//             row_len - n_added content slots a row.  A row holds [bos] + A[:ka] + [sep] * n_sep + B[s : s + kb] + [eos], padded
//             like a padded row.  The three truncation modes give one row per pair (s = 0) and cut from the END of a side;
//             windows mode cuts the first side to ka = min(la, C - stride - 1) and windows the second as Rule 3 does with Cb =
//             C - ka content slots and step = Cb - stride.
//             Rule 4 (lay_pair_keep / lay_pair_first / lay_pair_rows / lay_pair_row / lay_pair_slot): how many ids each side
//             keeps, the rows of a pair, what row k keeps, which source id a slot holds and whether it belongs to the second.
#pragma once
#include <stdint.h>

#include "tile_logic.h" // YB_HD

// (the values of YABPE_LAYOUT_* in include/yabpe.h)
constexpr uint32_t LAY_BOS = 0x01u, LAY_EOS = 0x02u, LAY_TRUNC_LEFT = 0x04u, LAY_PAD_LEFT = 0x08u, LAY_DROP_LAST = 0x10u;
constexpr uint32_t LAY_PAD_FLAGS = LAY_BOS | LAY_EOS | LAY_TRUNC_LEFT | LAY_PAD_LEFT;
constexpr uint32_t LAY_PACK_FLAGS = LAY_BOS | LAY_EOS | LAY_DROP_LAST;
constexpr uint32_t LAY_WIN_FLAGS = LAY_BOS | LAY_EOS | LAY_PAD_LEFT;
constexpr uint32_t LAY_PAIR_FLAGS = LAY_WIN_FLAGS;
// (the values of YABPE_PAIRS_* in include/yabpe.h)
constexpr uint32_t LAY_PAIRS_LONGEST_FIRST = 0u, LAY_PAIRS_ONLY_FIRST = 1u, LAY_PAIRS_ONLY_SECOND = 2u, LAY_PAIRS_WINDOWS = 3u;
constexpr uint32_t LAY_PAIRS_MAX_SEP = 2u;                     // separators between the two sides at most
constexpr uint32_t LAY_NO_DOC = 0xFFFFFFFFu;                   // `doc` of a packed slot past the end of the stream
constexpr unsigned long long LAY_MAX_SLOTS = 1ull << 36;       // output slots one call addresses at most

// what a slot holds: a source id (index into ids), or one of the three constants
constexpr unsigned long long LAY_SLOT_PAD = ~0ull, LAY_SLOT_BOS = ~0ull - 1, LAY_SLOT_EOS = ~0ull - 2;
constexpr unsigned long long LAY_SLOT_SEP = ~0ull - 3;         // pairs only; a slot below it is a source id

YB_HD uint32_t lay_n_added(uint32_t flags) { return (flags & LAY_BOS ? 1u : 0u) + (flags & LAY_EOS ? 1u : 0u); }

// length of seq(d) after the cut to row_len (row_len >= n_added), n = the document's ids
YB_HD unsigned long long lay_kept(unsigned long long n, unsigned long long row_len, uint32_t flags) {
    const unsigned long long seq = n + lay_n_added(flags);
    return seq < row_len ? seq : row_len;
}

// Rule 1.  Slot `col` of the padded row of a document whose n ids start at ids[start]: the index of the id it holds, or
// LAY_SLOT_PAD / LAY_SLOT_BOS / LAY_SLOT_EOS.
YB_HD unsigned long long lay_pad_slot(unsigned long long start, unsigned long long n, uint32_t row_len, uint32_t flags, uint32_t col) {
    const uint32_t added = lay_n_added(flags), bos = flags & LAY_BOS ? 1u : 0u;
    const uint32_t kept = (uint32_t)lay_kept(n, row_len, flags);
    const uint32_t lead = flags & LAY_PAD_LEFT ? row_len - kept : 0u; // pad slots in front of the sequence
    if (col < lead || col - lead >= kept) return LAY_SLOT_PAD;
    const uint32_t p = col - lead; // index into the kept sequence
    if (bos && p == 0) return LAY_SLOT_BOS;
    if ((flags & LAY_EOS) && p == kept - 1) return LAY_SLOT_EOS;
    const unsigned long long kc = kept - added; // content ids kept: the head, or the tail
    return start + (flags & LAY_TRUNC_LEFT ? n - kc : 0ull) + (p - bos);
}

// Rule 2.  The document stream position g lies in: the largest d in [lo, hi] with soff[d - org] <= g (soff[lo - org] <= g is
// the caller's promise; hi = the last document that may own g).  org: the document soff[0] belongs to (an LDS window).
YB_HD uint32_t lay_find_doc(const unsigned long long *soff, uint32_t org, uint32_t lo, uint32_t hi, unsigned long long g) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (soff[mid - org] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Stream position g in document d (soff_d = soff[d], soff_next = soff[d + 1]): *pos = its index inside seq(d); returns the index
// of the id it holds, or LAY_SLOT_BOS / LAY_SLOT_EOS.  The document's ids start at soff_d - n_added * d.
YB_HD unsigned long long lay_pack_slot(unsigned long long g, uint32_t d, unsigned long long soff_d, unsigned long long soff_next, uint32_t flags,
                                       unsigned long long *pos) {
    const unsigned long long p = g - soff_d;
    *pos = p;
    if ((flags & LAY_BOS) && p == 0) return LAY_SLOT_BOS;
    if ((flags & LAY_EOS) && g + 1 == soff_next) return LAY_SLOT_EOS;
    return g - (unsigned long long)lay_n_added(flags) * d - (flags & LAY_BOS ? 1u : 0u);
}

// rows of a packed batch over a stream of `total` positions
YB_HD unsigned long long lay_pack_rows(unsigned long long total, uint32_t row_len, uint32_t flags) {
    return flags & LAY_DROP_LAST ? total / row_len : (total + row_len - 1) / row_len;
}

// Rule 3.  Rows of a document of n ids: C >= 1 content slots a row, consecutive rows step = C - stride >= 1 ids apart.
YB_HD unsigned long long lay_win_rows(unsigned long long n, unsigned long long C, unsigned long long step) {
    return n <= C ? 1ull : 1ull + (n - C + step - 1) / step;
}

// content ids row k of that document keeps (k < lay_win_rows(n, C, step), so k * step <= n): C, less only in the last row
YB_HD unsigned long long lay_win_content(unsigned long long n, unsigned long long k, unsigned long long C, unsigned long long step) {
    const unsigned long long left = n - k * step;
    return left < C ? left : C;
}

// Slot `col` of a window row whose `content` ids start at ids[first]: the index of the id it holds, or LAY_SLOT_PAD / _BOS /
// _EOS -- a padded row of exactly those ids (content <= C: nothing is cut).
YB_HD unsigned long long lay_win_row_slot(unsigned long long first, unsigned long long content, uint32_t row_len, uint32_t flags, uint32_t col) {
    return lay_pad_slot(first, content, row_len, flags & LAY_WIN_FLAGS, col);
}

// Slot `col` of row k of a document whose n ids start at ids[start].
YB_HD unsigned long long lay_win_slot(unsigned long long start, unsigned long long n, unsigned long long k, uint32_t row_len, uint32_t stride,
                                      uint32_t flags, uint32_t col) {
    const unsigned long long C = row_len - lay_n_added(flags), step = C - stride;
    return lay_win_row_slot(start + k * step, lay_win_content(n, k, C, step), row_len, flags, col);
}

// Rule 4.  What the two sides of a pair (la, lb ids) keep in a row of C >= 1 content slots, one of the truncation modes.  Ids
// leave from the end of a side.  longest_first is the closed form of "while ka + kb > C: drop the last id of the longer side,
// of the second when they are equally long": the longer side shrinks until the sides meet, then they alternate, the second
// first, so with h2 = C / 2 (what the second ends with when both are cut) and h1 = C - h2 a side at or below its half is never
// touched and the other side gives up the whole excess.
YB_HD void lay_pair_keep(unsigned long long la, unsigned long long lb, unsigned long long C, uint32_t mode, unsigned long long *ka,
                         unsigned long long *kb) {
    *ka = la;
    *kb = lb;
    if (la + lb <= C) return;
    if (mode == LAY_PAIRS_LONGEST_FIRST) {
        const unsigned long long h2 = C / 2, h1 = C - h2;
        if (lb <= h2) {
            *ka = C - lb;
        } else if (la <= h1) {
            *kb = C - la;
        } else {
            *ka = h1;
            *kb = h2;
        }
        return;
    }
    // only_first / only_second: one side gives up the excess, down to zero ids; the other alone may still be longer than C
    const unsigned long long e = la + lb - C;
    if (mode == LAY_PAIRS_ONLY_FIRST) {
        *ka = la > e ? la - e : 0ull;
        *kb = lb < C ? lb : C;
    } else {
        *kb = lb > e ? lb - e : 0ull;
        *ka = la < C ? la : C;
    }
}

// windows mode: the ids the first side keeps in every row of its pair -- at least stride + 1 slots stay for the second
// (stride <= C - 1)
YB_HD unsigned long long lay_pair_first(unsigned long long la, unsigned long long C, unsigned long long stride) {
    const unsigned long long most = C - stride - 1;
    return la < most ? la : most;
}

// rows of a pair: one in the truncation modes
YB_HD unsigned long long lay_pair_rows(unsigned long long la, unsigned long long lb, unsigned long long C, uint32_t mode, unsigned long long stride) {
    if (mode != LAY_PAIRS_WINDOWS) return 1ull;
    const unsigned long long Cb = C - lay_pair_first(la, C, stride);
    return lay_win_rows(lb, Cb, Cb - stride);
}

// row k of a pair (k < lay_pair_rows): the ids it keeps of the first side (from its start) and of the second (from its id *s on)
YB_HD void lay_pair_row(unsigned long long la, unsigned long long lb, unsigned long long k, unsigned long long C, uint32_t mode,
                        unsigned long long stride, unsigned long long *ka, unsigned long long *s, unsigned long long *kb) {
    if (mode != LAY_PAIRS_WINDOWS) {
        *s = 0;
        lay_pair_keep(la, lb, C, mode, ka, kb);
        return;
    }
    *ka = lay_pair_first(la, C, stride);
    const unsigned long long Cb = C - *ka, step = Cb - stride;
    *s = k * step;
    *kb = lay_win_content(lb, k, Cb, step);
}

// Slot `col` of a pair row that keeps ka ids from ids[a0] on and kb ids from ids[b0] on: the index of the id it holds, or
// LAY_SLOT_PAD / _BOS / _SEP / _EOS.  *type = 1 in the second side and in EOS, else 0.
YB_HD unsigned long long lay_pair_slot(unsigned long long a0, uint32_t ka, unsigned long long b0, uint32_t kb, uint32_t n_sep, uint32_t row_len,
                                       uint32_t flags, uint32_t col, uint32_t *type) {
    const uint32_t bos = flags & LAY_BOS ? 1u : 0u, eos = flags & LAY_EOS ? 1u : 0u;
    const uint32_t kept = bos + ka + n_sep + kb + eos;
    const uint32_t lead = flags & LAY_PAD_LEFT ? row_len - kept : 0u; // pad slots in front of the sequence
    *type = 0u;
    if (col < lead || col - lead >= kept) return LAY_SLOT_PAD;
    uint32_t p = col - lead; // index into the kept sequence
    if (bos && p == 0) return LAY_SLOT_BOS;
    p -= bos;
    if (p < ka) return a0 + p;
    p -= ka;
    if (p < n_sep) return LAY_SLOT_SEP;
    p -= n_sep;
    *type = 1u;
    return p < kb ? b0 + p : LAY_SLOT_EOS;
}
