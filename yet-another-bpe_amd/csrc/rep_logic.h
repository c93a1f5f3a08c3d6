// rep_logic.h -- the repetition signals (BBPETokenizer.repetition_stats, yet_another_bpe/tokenizer.py), host- and device-
// callable: yabpe_rep_kernels.h and yabpe_repetition (yabpe.hip) call the same functions.
//
// Inputs ids u32[n_ids], n_docs document starts, up to 16 lengths n in [1, 64], strictly ascending.  All of it integer, and
// all of it PER DOCUMENT: equal windows of two different documents never meet.  For a document d of L ids and a length n:
//   window      n consecutive ids of d: L - n + 1 of them, none when L < n.  Windows never cross a document seam.
//   count(w)    the number of windows of d that hold the same n ids as w; overlapping windows count (a run of one id of
//               length L has one class of L - n + 1 windows).
//   top         the largest count in d: 0 without windows, 1 when nothing repeats.
//   distinct    the number of classes of equal windows in d (n = 1: the unique ids).
//   covered     the number of ids of d inside at least one window with count >= 2, every id once.
// Two forms on the device.  A document of at most REP_DOC ids is counted in a table in LDS, sized to the document, one slot a
// u32 of (position of the class's representative, count); a longer one in a table in HBM over the windows of all long
// documents, a slot the global position of the representative, the count in an array beside it.  Either way the window hash
// (dup_logic.h: Horner prefix, H(p) = P[p + n] - P[p] * B^n) only chooses the home slot and never decides equality; the global
// table mixes the document into the home slot, and a resident of another document is never equal.
#pragma once
#include <stdint.h>

#include "dup_logic.h"

constexpr uint32_t REP_MAX_NGRAMS = 16, REP_MAX_LEN = 64;
constexpr uint32_t REP_DOC = 2 * DUP_TILE;                 // ids of a short-form document at most: one Horner scan of 2,048 elements
constexpr uint32_t REP_SHORT_SLOTS = 2 * REP_DOC;          // slots of the LDS table at most
constexpr uint32_t REP_CNT_BITS = 12;                      // slot of the LDS table: position << 12 | count (count <= 2,048, position < 2,048)
constexpr uint32_t REP_CNT_MASK = (1u << REP_CNT_BITS) - 1;
constexpr uint32_t REP_EMPTY = DUP_EMPTY;
static_assert(REP_DOC <= REP_CNT_MASK && ((REP_DOC - 1) << REP_CNT_BITS | REP_DOC) < REP_EMPTY, "a packed slot never equals REP_EMPTY");
static_assert(REP_MAX_LEN <= DUP_TILE, "the mark's halo stays within one tile");

// the rule's argument checks (yabpe_repetition and BBPETokenizer._rep_ngrams refuse the same things)
YB_HD bool rep_rule_valid(uint32_t n_ngrams, const uint32_t *ngram, uint32_t flags) {
    if (n_ngrams < 1 || n_ngrams > REP_MAX_NGRAMS || flags) return false;
    for (uint32_t k = 0; k < n_ngrams; ++k)
        if (ngram[k] < 1 || ngram[k] > REP_MAX_LEN || (k && ngram[k] <= ngram[k - 1])) return false;
    return true;
}

// the short/long boundary: option rep_doc_max, 0 = REP_DOC.  A document of more ids takes the long form.
YB_HD bool rep_doc_max_valid(long long opt) { return opt >= 0 && opt <= (long long)REP_DOC; }
YB_HD uint32_t rep_boundary(long long opt) { return opt ? (uint32_t)opt : REP_DOC; }
YB_HD bool rep_is_long(unsigned long long L, uint32_t boundary) { return L > boundary; }

// the LDS table of a document with W >= 1 windows: the smallest power of two >= 2 W, two slots at least (W <= 2,048: 2^12 at most)
YB_HD uint32_t rep_short_slots_log2(uint32_t W) {
    uint32_t lg = 1;
    while ((1u << lg) < 2 * W) ++lg;
    return lg;
}
YB_HD uint32_t rep_pack(uint32_t pos, uint32_t count) { return pos << REP_CNT_BITS | count; }
YB_HD uint32_t rep_pos(uint32_t slot) { return slot >> REP_CNT_BITS; }
YB_HD uint32_t rep_count(uint32_t slot) { return slot & REP_CNT_MASK; }

// the home slot of the global table: the document is part of the key
YB_HD uint32_t rep_home(unsigned long long H, uint32_t d, uint32_t slots_log2) { return dup_home(H + ENC_RND_G * ((unsigned long long)d + 1), slots_log2); }

// id i is covered iff the last window with count >= 2 that starts at or before i (last1 = its start + 1, 0: none) reaches it
YB_HD bool rep_is_covered(uint32_t last1, uint32_t i, uint32_t n) { return last1 != 0 && i + 1 - last1 < n; }
