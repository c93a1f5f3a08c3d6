// decode_logic.h -- the rules of BBPETokenizer.decode (yet_another_bpe/tokenizer.py) on flat arrays, shared by the HIP kernels
// (yabpe_decode_kernels.h) and by the CPU unit-test model (tests/hostmodel/decode_model.cpp).
//
//   ids -> bytes   _vocab_inv = {i: t for t, i in vocab.items()}: a dense table id -> (offset into the byte pool, length);
//                  when two byte strings share an id the LAST one in vocab order wins.  Ids outside the table and ids no
//                  vocab entry names have no bytes (DEC_UNKNOWN): decode skips them.
//   UTF-8          bytes.decode("utf-8", errors="replace") per document: every maximal subpart of an ill-formed sequence
//                  becomes one U+FFFD (EF BF BD).  Each byte of a document is charged 0, 1 or 3 output bytes
//                  (dec_out_len): 1 = it is ASCII or part of a well-formed character and is copied; 3 = it starts a maximal
//                  subpart (a lead byte whose sequence does not complete, a byte that can never start one, a stray
//                  continuation byte); 0 = a continuation byte inside such a subpart.  The role of byte p needs at most 3
//                  bytes before it (its lead) and 3 after it (whether that lead's sequence completes), bounded by the
//                  document [ds, de): a sequence cut off at a document's end is replaced there.
#pragma once
#include <stdint.h>

#include "tile_logic.h" // YB_HD

constexpr uint32_t DEC_UNKNOWN = 0xFFFFFFFFu;       // table offset of an id that maps to no bytes
constexpr uint32_t DEC_MAX_ID = (1u << 24) - 1;     // largest id the table holds
constexpr unsigned long long DEC_MAX_POOL = (1ull << 32) - 1; // bytes the pool holds at most (u32 offsets)

// A byte buffer seen through an origin: T(j) = text[j - org] (the kernels read an LDS tile of the gathered text).
struct DecView {
    const uint8_t *text;
    uint64_t org;
    YB_HD uint8_t T(uint64_t j) const { return text[j - org]; }
};

YB_HD bool dec_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// length of the well-formed sequence that starts with b (1 ASCII, 2..4 a lead byte), 0 when b cannot start one
YB_HD int dec_need(uint8_t b) {
    if (b < 0x80u) return 1;
    if (b >= 0xC2u && b <= 0xDFu) return 2;
    if (b >= 0xE0u && b <= 0xEFu) return 3;
    if (b >= 0xF0u && b <= 0xF4u) return 4;
    return 0;
}

// the range of the byte after a lead (Unicode Table 3-7: no overlongs, no surrogates, nothing past U+10FFFF)
YB_HD bool dec_second_ok(uint8_t lead, uint8_t b) {
    uint8_t lo = 0x80u, hi = 0xBFu;
    if (lead == 0xE0u) lo = 0xA0u;
    else if (lead == 0xEDu) hi = 0x9Fu;
    else if (lead == 0xF0u) lo = 0x90u;
    else if (lead == 0xF4u) hi = 0x8Fu;
    return b >= lo && b <= hi;
}

// continuation bytes the byte at s takes (its maximal subpart is 1 + this many bytes); the sequence is complete iff the result
// is dec_need(t[s]) - 1.  0 for ASCII and for bytes that cannot start a sequence.
YB_HD int dec_take(const DecView &v, uint64_t s, uint64_t de) {
    const uint8_t lead = v.T(s);
    const int n = dec_need(lead);
    int k = 0;
    while (k + 1 < n && s + 1 + k < de) {
        const uint8_t b = v.T(s + 1 + k);
        if (k == 0 ? !dec_second_ok(lead, b) : !dec_cont(b)) break;
        ++k;
    }
    return k;
}

// Output bytes charged to byte p of the document [ds, de) (ds <= p < de): 1, 3 (U+FFFD) or 0 (see the header).
YB_HD uint32_t dec_out_len(const DecView &v, uint64_t p, uint64_t ds, uint64_t de) {
    const uint8_t b = v.T(p);
    if (b < 0x80u) return 1;
    if (!dec_cont(b)) {
        const int n = dec_need(b);
        return n && dec_take(v, p, de) == n - 1 ? 1u : 3u;
    }
    // a continuation byte: taken by the nearest byte before it that is not one (at most 3 back, inside the document) when
    // that byte's subpart reaches p; otherwise it stands alone
    for (uint64_t k = 1; k <= 3 && p - ds >= k; ++k) {
        const uint8_t c = v.T(p - k);
        if (dec_cont(c)) continue;
        const int t = dec_take(v, p - k, de);
        if ((uint64_t)t < k) return 3u;
        return t == dec_need(c) - 1 ? 1u : 0u;
    }
    return 3u;
}

// Writes the bytes dec_out_len charged to p (len = its result) at out.
YB_HD void dec_emit(uint8_t b, uint32_t len, uint8_t *out) {
    if (len == 1) {
        out[0] = b;
    } else if (len == 3) {
        out[0] = 0xEFu;
        out[1] = 0xBFu;
        out[2] = 0xBDu;
    }
}

// ---------------------------------------------------------------- the id table, built on the host
#include <vector>

struct DecTableHost {
    std::vector<uint32_t> ent; // 2 per id: offset into vocab_bytes (DEC_UNKNOWN: no bytes), length
};

// 0 on success; -1 when an id exceeds DEC_MAX_ID, -2 when the byte pool holds DEC_MAX_POOL bytes or more.  vocab entry i =
// vocab_bytes[vocab_off[i], vocab_off[i + 1]) with id vocab_ids[i]; the pool the offsets point into is vocab_bytes itself.
inline int dec_build_table(const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab, DecTableHost *t) {
    if (n_vocab && vocab_off[n_vocab] >= DEC_MAX_POOL) return -2;
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_vocab; ++i) {
        if (vocab_ids[i] > DEC_MAX_ID) return -1;
        n = vocab_ids[i] + 1 > n ? vocab_ids[i] + 1 : n;
    }
    t->ent.assign(2ull * n, 0);
    for (uint32_t i = 0; i < 2 * n; i += 2) t->ent[i] = DEC_UNKNOWN;
    for (uint32_t i = 0; i < n_vocab; ++i) { // in vocab order: the last entry of an id wins
        const uint64_t len = vocab_off[i + 1] - vocab_off[i];
        t->ent[2ull * vocab_ids[i]] = len ? (uint32_t)vocab_off[i] : 0u;
        t->ent[2ull * vocab_ids[i] + 1] = (uint32_t)len;
    }
    return 0;
}
