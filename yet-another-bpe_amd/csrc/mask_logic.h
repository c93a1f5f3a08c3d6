// mask_logic.h -- the masked-language-model rule (BBPETokenizer.mask_tokens, yet_another_bpe/tokenizer.py), host- and
// device-callable: yabpe_mask_kernels.h and the CPU model of tests/hostmodel/mask_model.cpp call the same functions.
//
// With rnd(seed, stream, i) of yet_another_bpe/synth.py (enc_rnd of encode_logic.h) and T(x) = min(2^32, int(x * 2^32)):
// document d of the batch has the key Kd = rnd(seed, 0x6d, first_doc + d).  Token j of the document (0-based, counted before
// any cut) belongs to the unit u = j, with whole-word masking u = the index of the piece it was made from.  A token of a
// special occurrence is never selected and draws nothing.  Otherwise r = rnd(Kd, 0x73, u); the token is selected iff
// (r >> 32) < Ts, and then x = r & 0xFFFFFFFF says what replaces it: x < Tm the mask id, Tm <= x < Tm + Tr the id
// rnd(Kd, 0x72, j) % n_random (drawn per token in whole-word mode too), else the id stays.  The label of a selected token is
// its original id, that of every other one the ignore value.  Every draw is a function of (seed, first_doc + d, u or j)
// alone: the tokens of a word are selected together and replaced in the same way without talking to each other.
#pragma once
#include <stdint.h>

#include "encode_logic.h"

constexpr unsigned long long MASK_STREAM_DOC = 0x6d, MASK_STREAM_SELECT = 0x73, MASK_STREAM_RANDOM = 0x72;
constexpr unsigned long long MASK_T_ONE = 1ull << 32;  // T of 1.0
constexpr uint32_t MASK_WORD_SPECIAL = ENC_WORD_SPECIAL;  // words[k]: bit 31 = a special occurrence, the rest the piece index
constexpr uint32_t MASK_BLOCK = 256;                   // ids a workgroup of k_mask takes

// what became of a token (the order of the counters of k_mask, MASK_UNSELECTED aside)
enum MaskKind : uint32_t { MASK_PROTECTED = 0, MASK_MASKED = 1, MASK_RANDOM = 2, MASK_KEPT = 3, MASK_KINDS = 4, MASK_UNSELECTED = 4 };

struct MaskRule {
    unsigned long long select, mask, random;  // Ts, Tm, Tr: each <= 2^32, Tm + Tr <= 2^32
    uint32_t mask_id, n_random;               // n_random >= 1 when Tr > 0
};

// the rule's argument checks (yabpe_mask and the model refuse the same things)
YB_HD bool mask_rule_valid(const MaskRule &R) {
    return R.select <= MASK_T_ONE && R.mask <= MASK_T_ONE && R.random <= MASK_T_ONE && R.mask + R.random <= MASK_T_ONE &&
           (R.random == 0 || R.n_random != 0);
}

YB_HD unsigned long long mask_doc_key(unsigned long long seed, unsigned long long first_doc, unsigned long long d) {
    return enc_rnd(seed, MASK_STREAM_DOC, first_doc + d);
}

// An unprotected token of unit u at index j of its document, id `id`: -> its kind; *new_id = what the inputs hold there.
YB_HD uint32_t mask_decide(unsigned long long kd, unsigned long long u, unsigned long long j, const MaskRule &R, uint32_t id, uint32_t *new_id) {
    *new_id = id;
    const unsigned long long r = enc_rnd(kd, MASK_STREAM_SELECT, u);
    if ((r >> 32) >= R.select) return MASK_UNSELECTED;
    const unsigned long long x = r & 0xFFFFFFFFull;
    if (x < R.mask) {
        *new_id = R.mask_id;
        return MASK_MASKED;
    }
    if (x < R.mask + R.random) {
        *new_id = (uint32_t)(enc_rnd(kd, MASK_STREAM_RANDOM, j) % R.n_random);
        return MASK_RANDOM;
    }
    return MASK_KEPT;
}

// The document of id i: the last d in [lo, hi] with doc_off[d] <= i (doc_off: the n_docs starts, ascending from 0; an empty
// document shares its start with its successor and is never the answer while a later one starts there too).
YB_HD uint32_t mask_doc_of(const unsigned long long *doc_off, unsigned long long i, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (doc_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One id in full: the words entry w (0 without a words array), whole-word mode or not -> its kind; *new_id, *label.
YB_HD uint32_t mask_token(unsigned long long seed, unsigned long long first_doc, uint32_t d, unsigned long long j, uint32_t w, bool whole_word,
                          const MaskRule &R, uint32_t ignore, uint32_t id, uint32_t *new_id, uint32_t *label) {
    *new_id = id;
    *label = ignore;
    if (w & MASK_WORD_SPECIAL) return MASK_PROTECTED;
    const uint32_t kind = mask_decide(mask_doc_key(seed, first_doc, d), whole_word ? (unsigned long long)(w & ~MASK_WORD_SPECIAL) : j, j, R, id, new_id);
    if (kind != MASK_UNSELECTED) *label = id;
    return kind;
}
