// encode_logic.h -- the rules of BBPETokenizer.encode (yet_another_bpe/tokenizer.py) on ids, shared by the HIP kernels
// (yabpe_encode_kernels.h) and by the CPU unit-test models (tests/hostmodel/encode_model.cpp, spans_model.cpp).
//
//   specials   regex.split("(s1|s2|...)") with the specials in the tokenizer's order (longest first, stable): leftmost
//              occurrence, first alternative at that position, no overlaps.  Occurrences that overlap form a CHAIN, resolved
//              left to right by the thread of its first occurrence (enc_special_walk); chains are independent.  The result
//              is one byte per position: 0 text, 1 + index at the first byte of a taken special, ENC_INSIDE on its other
//              bytes.  Every special span and every text between two spans is a text of its own for the GPT-2 pattern
//              (pretok_logic.h with a PT_CHUNK0 mark at each span's first byte and right after it).
//   merges     per pre-token, repeatedly the adjacent pair with the lowest rank, leftmost on ties (rank = LAST index of the
//              pair in `merges`).  Pairs are keyed by bytes; the host interns every byte string that can be a token of a
//              word (the 256 single bytes, both operands and the concatenation of every merge) to a dense internal id, so
//              a lookup on the pair of internal ids is exactly a lookup on the pair of byte strings.
//   ids        internal id -> vocab.get(bytes, unk); a special -> vocab[special] if present, else nothing.
#pragma once
#include <stdint.h>

#include "pretok_logic.h" // PtView, PtSpecials, pt_special_at, PT_CHUNK0; YB_HD

constexpr uint32_t ENC_NONE = 0xFFFFFFFFu;        // no rank / no token
constexpr unsigned long long ENC_EMPTY = ~0ull;   // free slot of the pair table
constexpr uint8_t ENC_INSIDE = 0xFF;              // a byte inside a taken special (not its first)
constexpr uint32_t ENC_MAX_SPECIALS = 254;        // 1 + index must fit below ENC_INSIDE
constexpr uint32_t ENC_SHORT = 64;                // words of at most this many bytes: one lane per byte
constexpr uint32_t ENC_WORD_SPECIAL = 0x80000000u; // yabpe_encode_words: the piece of this id is a special occurrence

// ---------------------------------------------------------------- pair table: (a, b) -> (rank, result)
struct EncTable {
    const unsigned long long *keys; // (a << 32) | b, ENC_EMPTY = free
    const uint32_t *vals;           // 2 per slot: rank, internal id of the concatenation
    unsigned long long mask;        // capacity - 1 (a power of two, load <= 1/2)
};

YB_HD unsigned long long enc_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

YB_HD bool enc_lookup(const EncTable &t, uint32_t a, uint32_t b, uint32_t *rank, uint32_t *res) {
    const unsigned long long key = ((unsigned long long)a << 32) | b;
    unsigned long long s = enc_mix(key) & t.mask;
    while (true) {
        const unsigned long long k = t.keys[s];
        if (k == key) {
            *rank = t.vals[2 * s];
            *res = t.vals[2 * s + 1];
            return true;
        }
        if (k == ENC_EMPTY) return false;
        s = (s + 1) & t.mask;
    }
}

// ---------------------------------------------------------------- special split (v.meta holds the document marks only)
// An occurrence at i heads its chain iff no earlier occurrence of the same document covers i.
template <class OccF>
YB_HD bool enc_special_is_head(const PtView &v, const PtSpecials &sp, OccF occ, uint64_t i) {
    if (v.M(i) & PT_CHUNK0) return true;
    for (uint64_t d = 1; d < sp.max_len && d <= i; ++d) {
        const uint64_t q = i - d;
        const uint32_t o = occ(q);
        if (o && (uint64_t)pt_special_len(sp, o) > d) return false;
        if (v.M(q) & PT_CHUNK0) break;
    }
    return true;
}

// Resolves the chain headed by the occurrence o0 at i: sflag[q] = o for every taken occurrence q, ENC_INSIDE on its other bytes.
template <class OccF>
YB_HD void enc_special_walk(const PtView &v, const PtSpecials &sp, OccF occ, uint8_t *sflag, uint64_t i, uint32_t o0) {
    uint64_t cover = 0, reach = 0, q = i;
    uint32_t oq = o0;
    while (true) {
        const uint32_t len = pt_special_len(sp, oq);
        if (q >= cover) { // leftmost, first alternative (occ() returns the first special in order that stands at q)
            sflag[q] = (uint8_t)oq;
            for (uint32_t k = 1; k < len; ++k) sflag[q + k] = ENC_INSIDE;
            cover = q + len;
        }
        if (q + len > reach) reach = q + len;
        uint64_t nq = q + 1;
        uint32_t no = 0;
        for (; nq < reach; ++nq) { // (an occurrence never crosses a document start, so neither does reach)
            no = occ(nq);
            if (no) break;
        }
        if (!no) return;
        q = nq;
        oq = no;
    }
}

// Does a text of its own (for the GPT-2 pattern) start at i?  A special's first byte, and the byte right after a special.
YB_HD bool enc_segment_start(const uint8_t *sflag, uint64_t i) {
    const uint8_t f = sflag[i];
    if (f != 0 && f != ENC_INSIDE) return true;
    return i > 0 && f == 0 && sflag[i - 1] != 0;
}

// ---------------------------------------------------------------- checksum of one word's segmentation
// The fold of k_stream_checksum (yabpe_kernels.h): FNV-1a over each token's bytes followed by the 0x1ff boundary, then mixed,
// summed over the words whose segmentation has at least 2 tokens -- the words a flat training stream still holds (a word
// of one byte is never loaded there, and one that becomes a single token leaves it), so that the two folds can be compared.
YB_HD unsigned long long enc_fnv_init() { return 1469598103934665603ull; }
YB_HD unsigned long long enc_fnv_byte(unsigned long long h, uint8_t b) { return (h ^ b) * 1099511628211ull; }
YB_HD unsigned long long enc_fnv_mark(unsigned long long h) { return (h ^ 0x1ffull) * 1099511628211ull; }
YB_HD unsigned long long enc_fnv_final(unsigned long long h) {
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h;
}

// ---------------------------------------------------------------- one word, sequentially (any length)
// A binary min-heap of (rank << 32 | position) with lazy invalidation: an entry is current iff its position still starts
// a token that has a right neighbour and the pair there still has that rank.  Positions of token starts keep their left-to-
// right order, so the smallest entry is the lowest rank, leftmost on ties.  O(L log L).
// Scratch: tok, nxt, prv of L entries, heap of 3 L entries.  Returns the number of tokens; tok[0..count) = their internal
// ids, nxt[0..count) = their first bytes.
YB_HD void enc_heap_push(unsigned long long *heap, uint32_t &hn, unsigned long long v) {
    uint32_t k = hn++;
    while (k > 0) {
        const uint32_t p = (k - 1) >> 1;
        if (heap[p] <= v) break;
        heap[k] = heap[p];
        k = p;
    }
    heap[k] = v;
}

YB_HD unsigned long long enc_heap_pop(unsigned long long *heap, uint32_t &hn) {
    const unsigned long long top = heap[0];
    const unsigned long long v = heap[--hn];
    uint32_t k = 0;
    while (true) {
        uint32_t c = 2 * k + 1;
        if (c >= hn) break;
        if (c + 1 < hn && heap[c + 1] < heap[c]) ++c;
        if (v <= heap[c]) break;
        heap[k] = heap[c];
        k = c;
    }
    if (hn) heap[k] = v;
    return top;
}

YB_HD uint32_t enc_merge_heap(const uint8_t *w, uint32_t L, const EncTable &t, uint32_t *tok, uint32_t *nxt, uint32_t *prv,
                              unsigned long long *heap) {
    for (uint32_t p = 0; p < L; ++p) {
        tok[p] = w[p]; // internal ids 0..255 are the single bytes
        nxt[p] = p + 1 < L ? p + 1 : ENC_NONE;
        prv[p] = p ? p - 1 : ENC_NONE;
    }
    uint32_t hn = 0, r = 0, res = 0;
    for (uint32_t p = 0; p + 1 < L; ++p)
        if (enc_lookup(t, tok[p], tok[p + 1], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
    while (hn) {
        const unsigned long long e = enc_heap_pop(heap, hn);
        const uint32_t p = (uint32_t)e, er = (uint32_t)(e >> 32);
        if (tok[p] == ENC_NONE) continue;           // no longer a token start
        const uint32_t q = nxt[p];
        if (q == ENC_NONE) continue;
        if (!enc_lookup(t, tok[p], tok[q], &r, &res) || r != er) continue; // the pair there changed
        tok[p] = res;
        tok[q] = ENC_NONE;
        nxt[p] = nxt[q];
        if (nxt[q] != ENC_NONE) prv[nxt[q]] = p;
        if (nxt[p] != ENC_NONE && enc_lookup(t, tok[p], tok[nxt[p]], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
        const uint32_t a = prv[p];
        if (a != ENC_NONE && enc_lookup(t, tok[a], tok[p], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | a);
    }
    // compact: tok[k] = id, nxt[k] = byte offset of token k (k <= p: only entries already read are overwritten)
    uint32_t k = 0, p = L ? 0 : ENC_NONE;
    while (p != ENC_NONE) {
        const uint32_t np = nxt[p];
        nxt[k] = p;
        tok[k++] = tok[p];
        p = np;
    }
    return k;
}

// ---------------------------------------------------------------- BPE-dropout (BBPETokenizer.encode_dropout)
// rnd(seed, stream, i) of yet_another_bpe/synth.py (synth_rnd of yabpe_aux_kernels.h: the same mix), u64 with wraparound.
// Document key Kd = rnd(seed, 0x64, doc); word key Kw = rnd(Kd, 0x77, s), s = the pre-token's byte offset in its document.
// At merge step t (merges performed so far) the candidate whose left part starts at byte q of the word is dropped iff
// rnd(Kw, t, q) >> 32 < T, T = min(2^32, int(p * 2^32)); the surviving candidate of lowest rank, leftmost on ties, merges.
constexpr unsigned long long ENC_RND_G = 0x9E3779B97F4A7C15ull, ENC_RND_S = 0xD1B54A32D192ED03ull;
constexpr unsigned long long ENC_DROP_DOC = 0x64, ENC_DROP_WORD = 0x77;
constexpr unsigned long long ENC_DROP_ALL = 1ull << 32; // T of p = 1

YB_HD unsigned long long enc_rnd(unsigned long long seed, unsigned long long stream, unsigned long long i) {
    return enc_mix(seed + ENC_RND_G * (i + 1) + ENC_RND_S * stream);
}
YB_HD unsigned long long enc_drop_doc_key(unsigned long long seed, unsigned long long doc) { return enc_rnd(seed, ENC_DROP_DOC, doc); }
YB_HD unsigned long long enc_drop_word_key(unsigned long long kd, unsigned long long s) { return enc_rnd(kd, ENC_DROP_WORD, s); }
// The draw in two halves, so that a lane keeps what does not change from step to step: lane = enc_drop_lane(Kw, q) once,
// then enc_dropped(lane + ENC_RND_S * t, T) at step t.
YB_HD unsigned long long enc_drop_lane(unsigned long long kw, uint32_t q) { return kw + ENC_RND_G * ((unsigned long long)q + 1); }
YB_HD bool enc_dropped(unsigned long long lane_t, unsigned long long T) { return (enc_mix(lane_t) >> 32) < T; }
YB_HD bool enc_drop_draw(unsigned long long kw, uint32_t t, uint32_t q, unsigned long long T) {
    return enc_dropped(enc_drop_lane(kw, q) + ENC_RND_S * t, T);
}

// enc_merge_heap with dropout: the draws are evaluated lazily.  The smallest current entry is popped; dropped at (t, q), it
// is set aside and the next one popped, so the first entry that survives is the smallest candidate not dropped at step t.
// After its merge the entries set aside go back to the heap (their draws at t + 1 are new ones); when the heap runs empty
// without a survivor the word is finished.  Expected pops per step 1 / (1 - p); T = 2^32 drains the heap once.
// The entries set aside live at the top end of `heap`, growing down: heap and set-aside together only ever hold entries
// that were pushed and not yet discarded, at most 3 (L - 1).  Scratch and result as enc_merge_heap.
YB_HD uint32_t enc_merge_heap_dropout(const uint8_t *w, uint32_t L, const EncTable &t, unsigned long long kw, unsigned long long T,
                                      uint32_t *tok, uint32_t *nxt, uint32_t *prv, unsigned long long *heap) {
    for (uint32_t p = 0; p < L; ++p) {
        tok[p] = w[p];
        nxt[p] = p + 1 < L ? p + 1 : ENC_NONE;
        prv[p] = p ? p - 1 : ENC_NONE;
    }
    uint32_t hn = 0, r = 0, res = 0, step = 0, aside = 3 * L; // set aside: heap[aside .. 3 L)
    for (uint32_t p = 0; p + 1 < L; ++p)
        if (enc_lookup(t, tok[p], tok[p + 1], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
    while (hn) {
        const unsigned long long e = enc_heap_pop(heap, hn);
        const uint32_t p = (uint32_t)e, er = (uint32_t)(e >> 32);
        if (tok[p] == ENC_NONE) continue;
        const uint32_t q = nxt[p];
        if (q == ENC_NONE) continue;
        if (!enc_lookup(t, tok[p], tok[q], &r, &res) || r != er) continue;
        if (enc_drop_draw(kw, step, p, T)) {
            heap[--aside] = e;
            continue;
        }
        tok[p] = res;
        tok[q] = ENC_NONE;
        nxt[p] = nxt[q];
        if (nxt[q] != ENC_NONE) prv[nxt[q]] = p;
        ++step;
        while (aside < 3 * L) enc_heap_push(heap, hn, heap[aside++]); // (hn < aside here: the push never overwrites what it reads)
        if (nxt[p] != ENC_NONE && enc_lookup(t, tok[p], tok[nxt[p]], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | p);
        const uint32_t a = prv[p];
        if (a != ENC_NONE && enc_lookup(t, tok[a], tok[p], &r, &res)) enc_heap_push(heap, hn, ((unsigned long long)r << 32) | a);
    }
    uint32_t k = 0, p = L ? 0 : ENC_NONE;
    while (p != ENC_NONE) {
        const uint32_t np = nxt[p];
        nxt[k] = p;
        tok[k++] = tok[p];
        p = np;
    }
    return k;
}

// The checksum hash of a word whose tokens start at starts[0..count) (byte offsets into w, ascending).
YB_HD unsigned long long enc_word_hash(const uint8_t *w, uint32_t L, const uint32_t *starts, uint32_t count) {
    unsigned long long h = enc_fnv_init();
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t e = k + 1 < count ? starts[k + 1] : L;
        for (uint32_t p = starts[k]; p < e; ++p) h = enc_fnv_byte(h, w[p]);
        h = enc_fnv_mark(h);
    }
    return enc_fnv_final(h);
}

// ---------------------------------------------------------------- spans: which bytes / characters each token covers
// Byte unit: token k of a word covers [start_k, start_{k+1}) of it, the last one up to the word's end.  The starts are the
// alive lanes of the lane form and, on the long path, what enc_merge_heap leaves in nxt[0..count).
YB_HD uint32_t enc_heap_start(const uint32_t *nxt, uint32_t k) { return nxt[k]; }
YB_HD uint32_t enc_token_end(const uint32_t *starts, uint32_t count, uint32_t L, uint32_t k) { return k + 1 < count ? starts[k + 1] : L; }

// Char unit: with lead(p) = the number of non-continuation bytes below p, the smallest run of whole characters that covers
// the bytes [s, e) is [lead(s + 1) - 1, lead(e)).  (A token may begin or end inside a character.)
YB_HD bool enc_is_lead(uint8_t b) { return (b & 0xC0) != 0x80; }
template <class LeadF>
YB_HD unsigned long long enc_char_start(LeadF lead, unsigned long long s) { return lead(s + 1) - 1ull; }
template <class LeadF>
YB_HD unsigned long long enc_char_end(LeadF lead, unsigned long long e) { return lead(e); }

// lead() from a prefix every ENC_GRANULE bytes: table[g] = lead(g * ENC_GRANULE), then at most four 16-byte chunks of the
// text.  `text` must be 16-byte aligned; a chunk that would reach past n is read byte by byte.
constexpr uint32_t ENC_GRANULE = 64;
struct alignas(16) EncChunk {
    unsigned long long lo, hi;
};

// the continuation bytes (10xxxxxx) among the low `bytes` bytes of x (bytes in 1..8)
YB_HD uint32_t enc_cont_count(unsigned long long x, uint32_t bytes) {
    unsigned long long c = x & ~(x << 1) & 0x8080808080808080ull;
    if (bytes < 8) c &= (1ull << (8 * bytes)) - 1ull;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(c);
#else
    return (uint32_t)__builtin_popcountll(c);
#endif
}

// non-continuation bytes in [c, c + m), c a multiple of 16, 1 <= m <= 16
YB_HD uint32_t enc_lead_chunk(const uint8_t *text, unsigned long long n, unsigned long long c, uint32_t m) {
    uint32_t cont = 0;
    if (c + 16 <= n) {
        const EncChunk v = *(const EncChunk *)(text + c);
        cont = enc_cont_count(v.lo, m < 8 ? m : 8);
        if (m > 8) cont += enc_cont_count(v.hi, m - 8);
    } else {
        for (uint32_t k = 0; k < m; ++k) cont += enc_is_lead(text[c + k]) ? 0u : 1u;
    }
    return m - cont;
}

YB_HD unsigned long long enc_lead(const uint8_t *text, unsigned long long n, const unsigned long long *table, unsigned long long p) {
    const unsigned long long g = p / ENC_GRANULE;
    unsigned long long r = table[g];
    for (unsigned long long c = g * ENC_GRANULE; c < p; c += 16) r += enc_lead_chunk(text, n, c, p - c < 16 ? (uint32_t)(p - c) : 16u);
    return r;
}

// ---------------------------------------------------------------- the model, built on the host
#include <string>
#include <unordered_map>
#include <vector>

struct EncModelHost {
    std::vector<unsigned long long> keys;
    std::vector<uint32_t> vals;
    std::vector<uint32_t> out_id;   // internal id -> output id
    std::vector<uint32_t> sp_id;    // special index -> output id ...
    std::vector<uint8_t> sp_has;    // ... when present in the vocab (else the special emits nothing)
    uint32_t n_internal = 0;
    uint64_t n_pairs = 0;
    EncTable table() const { return EncTable{keys.data(), vals.data(), keys.size() - 1}; }
};

// 0 on success, -1 (YABPE_E_INVALID) for an empty special, -4 (YABPE_E_CAPACITY) past the id range or the special count.
inline int enc_build_model(const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab,
                           const uint8_t *merge_bytes, const uint64_t *merge_off, uint32_t n_merges, const uint8_t *special_bytes,
                           const uint32_t *special_off, uint32_t n_special, uint32_t unk_id, EncModelHost *m) {
    if (n_special > ENC_MAX_SPECIALS) return -4;
    for (uint32_t s = 0; s < n_special; ++s)
        if (special_off[s + 1] <= special_off[s]) return -1;
    std::unordered_map<std::string, uint32_t> vocab;
    vocab.reserve(n_vocab * 2 + 1);
    for (uint32_t i = 0; i < n_vocab; ++i)
        vocab.emplace(std::string((const char *)vocab_bytes + vocab_off[i], vocab_off[i + 1] - vocab_off[i]), vocab_ids[i]);
    std::unordered_map<std::string, uint32_t> intern;
    intern.reserve(256 + 3ull * n_merges);
    std::vector<std::string> names;
    auto id_of = [&](std::string s) -> uint32_t {
        auto it = intern.find(s);
        if (it != intern.end()) return it->second;
        const uint32_t id = (uint32_t)names.size();
        intern.emplace(s, id);
        names.push_back(std::move(s));
        return id;
    };
    for (int b = 0; b < 256; ++b) id_of(std::string(1, (char)b));
    if (256ull + 3ull * n_merges >= ENC_NONE) return -4;
    std::unordered_map<unsigned long long, uint64_t> pairs; // key -> (rank << 32 | result); a later duplicate overwrites
    pairs.reserve(n_merges * 2 + 1);
    for (uint32_t i = 0; i < n_merges; ++i) {
        std::string l((const char *)merge_bytes + merge_off[2 * i], merge_off[2 * i + 1] - merge_off[2 * i]);
        std::string r((const char *)merge_bytes + merge_off[2 * i + 1], merge_off[2 * i + 2] - merge_off[2 * i + 1]);
        const uint32_t a = id_of(l), b = id_of(r), c = id_of(l + r);
        pairs[((unsigned long long)a << 32) | b] = ((uint64_t)i << 32) | c;
    }
    m->n_internal = (uint32_t)names.size();
    m->n_pairs = pairs.size();
    uint64_t cap = 16;
    while (cap < 2 * pairs.size()) cap <<= 1;
    m->keys.assign(cap, ENC_EMPTY);
    m->vals.assign(2 * cap, 0);
    for (const auto &kv : pairs) {
        unsigned long long s = enc_mix(kv.first) & (cap - 1);
        while (m->keys[s] != ENC_EMPTY) s = (s + 1) & (cap - 1);
        m->keys[s] = kv.first;
        m->vals[2 * s] = (uint32_t)(kv.second >> 32);
        m->vals[2 * s + 1] = (uint32_t)kv.second;
    }
    m->out_id.resize(names.size());
    for (size_t i = 0; i < names.size(); ++i) {
        auto it = vocab.find(names[i]);
        m->out_id[i] = it == vocab.end() ? unk_id : it->second;
    }
    m->sp_id.assign(n_special, 0);
    m->sp_has.assign(n_special, 0);
    for (uint32_t s = 0; s < n_special; ++s) {
        auto it = vocab.find(std::string((const char *)special_bytes + special_off[s], special_off[s + 1] - special_off[s]));
        if (it != vocab.end()) {
            m->sp_id[s] = it->second;
            m->sp_has[s] = 1;
        }
    }
    return 0;
}
