// span_logic.h -- the span-corruption rule (BBPETokenizer.corrupt_spans, yet_another_bpe/tokenizer.py), host- and
// device-callable: yabpe_span_kernels.h and the CPU model of tests/hostmodel/span_model.cpp call the same functions.
//
// With rnd(seed, stream, i) of yet_another_bpe/synth.py (enc_rnd of encode_logic.h): document d of the batch has the key Kd =
// rnd(seed, 0x63, first_doc + d) -- not the mask's 0x6d, so one seed gives unrelated mask and span draws.  Token j of the
// document (0-based, counted before any cut) belongs to the unit u = j, in whole-word mode u = the index of the piece it was
// made from.  Per unit r = rnd(Kd, 0x6f, u): the unit opens a span iff (r >> 32) < To, and the span covers len(u) = 1 +
// #{k < Lmax - 1 : (r & 0xFFFFFFFF) < C[k]} units from u on (C non-increasing, so len(u) >= L iff L == 1 or x < C[L - 2]: no
// loop).  Unit v is noise iff some u in [max(0, v - Lmax + 1), v] opens with u + len(u) > v: at most Lmax draws, none of which
// reads protection, the cut or the batch.  A token is noise iff its unit is noise and it is no special occurrence.
//
// Per id the passes keep one byte (SPAN_F_*).  A run is a maximal stretch of consecutive kept noise ids of one document; runs
// are numbered per document, and those past the sentinel cap stay in the inputs (span_place clears their bits).
#pragma once
#include <stdint.h>

#include "encode_logic.h"
#include "mask_logic.h"  // mask_doc_of, MASK_WORD_SPECIAL

constexpr unsigned long long SPAN_STREAM_DOC = 0x63, SPAN_STREAM_DRAW = 0x6f;
constexpr unsigned long long SPAN_T_ONE = 1ull << 32;  // T of 1.0
constexpr uint32_t SPAN_MAX_LEN = 32;                  // Lmax at most (YABPE_SPAN_MAX_LEN)
constexpr uint32_t SPAN_BLOCK = 256;                   // ids a workgroup of every pass takes

// the byte of an id: after the flags pass KEPT, NOISE, START; after the place pass NOISE and START only on runs below the cap,
// and LAST on the id that carries its document's final sentinel
constexpr uint8_t SPAN_F_KEPT = 1, SPAN_F_NOISE = 2, SPAN_F_START = 4, SPAN_F_LAST = 8;

struct SpanRule {
    unsigned long long open;         // To <= 2^32
    const unsigned long long *len;   // C[0 .. max_len - 2], each <= 2^32, non-increasing (memory of the side that calls)
    uint32_t max_len;                // Lmax in 1 .. SPAN_MAX_LEN
};

// the rule's argument checks (yabpe_span_corrupt and the model refuse the same things); len: host memory here
YB_HD bool span_rule_valid(unsigned long long open, const unsigned long long *len, uint32_t max_len) {
    if (open > SPAN_T_ONE || max_len < 1 || max_len > SPAN_MAX_LEN) return false;
    for (uint32_t k = 0; k + 1 < max_len; ++k)
        if (len[k] > SPAN_T_ONE || (k && len[k] > len[k - 1])) return false;
    return true;
}

YB_HD unsigned long long span_doc_key(unsigned long long seed, unsigned long long first_doc, unsigned long long d) {
    return enc_rnd(seed, SPAN_STREAM_DOC, first_doc + d);
}

// Is unit v of the document with key kd noise?  Nearest opener first: it is the likeliest to reach v.
YB_HD bool span_unit_noise(unsigned long long kd, unsigned long long v, const SpanRule &R) {
    const unsigned long long lo = v >= R.max_len - 1 ? v - (R.max_len - 1) : 0;
    for (unsigned long long u = v;; --u) {
        const unsigned long long r = enc_rnd(kd, SPAN_STREAM_DRAW, u);
        if ((r >> 32) < R.open) {
            const unsigned long long need = v - u + 1;  // len(u) >= need?  (need <= Lmax)
            if (need == 1 || (r & 0xFFFFFFFFull) < R.len[need - 2]) return true;
        }
        if (u == lo) return false;
    }
}

// One id: index j in its document, words entry w (0 without a words array) -> noise or not
YB_HD bool span_token_noise(unsigned long long kd, unsigned long long j, uint32_t w, bool whole_word, const SpanRule &R) {
    if (w & MASK_WORD_SPECIAL) return false;
    return span_unit_noise(kd, whole_word ? (unsigned long long)(w & ~MASK_WORD_SPECIAL) : j, R);
}

YB_HD bool span_kept(unsigned long long j, unsigned long long max_doc_ids) { return max_doc_ids == 0 || j < max_doc_ids; }

// flags pass: the byte of an id from its own noise and its predecessor's (prev_noise: of id j - 1 of the same document)
YB_HD uint8_t span_flags(bool kept, bool noise, unsigned long long j, bool prev_noise) {
    if (!kept) return 0;
    if (!noise) return SPAN_F_KEPT;
    return (uint8_t)(SPAN_F_KEPT | SPAN_F_NOISE | ((j == 0 || !prev_noise) ? SPAN_F_START : 0));
}

// place pass.  f: the flags pass's byte; k: the run's number in its document (meaningful with NOISE); K: runs that get a
// sentinel; is_last: the document's last kept id, and a final sentinel is asked for.  -> the final byte; *c_in / *c_tgt: the
// slots the id takes in the inputs and the targets (the final sentinel is charged to the last kept id); *over: the id starts a
// run past the cap.
YB_HD uint8_t span_place(uint8_t f, unsigned long long k, unsigned long long K, bool is_last, uint8_t *c_in, uint8_t *c_tgt, bool *over) {
    *over = false;
    if ((f & SPAN_F_NOISE) && k >= K) {
        *over = (f & SPAN_F_START) != 0;
        f = SPAN_F_KEPT;
    }
    const bool kept = (f & SPAN_F_KEPT) != 0, noise = (f & SPAN_F_NOISE) != 0, start = (f & SPAN_F_START) != 0;
    if (kept && is_last) f |= SPAN_F_LAST;
    *c_in = (uint8_t)(kept ? (noise ? (start ? 1 : 0) : 1) : 0);
    *c_tgt = (uint8_t)((noise ? 1 + (start ? 1 : 0) : 0) + ((f & SPAN_F_LAST) ? 1 : 0));
    return f;
}

// write pass: one id's stores.  ip / tp: its first slot in the inputs / targets; k: its run's number (read with START only);
// n_runs: the runs of its document (read with LAST only).
YB_HD void span_write(uint8_t f, uint32_t id, unsigned long long ip, unsigned long long tp, unsigned long long k, unsigned long long n_runs,
                      unsigned long long K, const uint32_t *sentinels, uint32_t *out_in, uint32_t *out_tgt) {
    if (!(f & SPAN_F_KEPT)) return;
    if (f & SPAN_F_NOISE) {
        if (f & SPAN_F_START) {
            const uint32_t s = sentinels[k];
            out_in[ip] = s;
            out_tgt[tp++] = s;
        }
        out_tgt[tp++] = id;
    } else {
        out_in[ip] = id;
    }
    if (f & SPAN_F_LAST) out_tgt[tp] = sentinels[n_runs < K ? n_runs : K];
}
