// yabpe_encode_kernels.h -- BBPETokenizer.encode on the device (yet_another_bpe/tokenizer.py; rules in encode_logic.h).
//
// Passes (host orchestration: yabpe_encode in yabpe.hip):
//   split     k_pt_mark_chunks (document starts) -> k_enc_special (sflag: the tokenizer's special split) -> k_enc_segments
//             (every special span and every text between spans becomes a text of its own) -> k_pt_fused (classes, UTF-8,
//             pre-token starts) -> k_enc_clear (no start inside a special) -> with the option "digit_group": k_grp_windows /
//             k_grp_carry / k_grp_apply (digit runs cut into groups, yabpe_pretok_kernels.h)
//   pretok    k_pt_count / exclusive_scan / k_pt_scatter: starts -> u64 pre-token offsets into the text
//   pool      k_word_hash / k_word_dedup / k_dedup_flags + scans: each pre-token's representative (unique word), then
//             k_enc_compact lists the unique words and the scratch each long one needs
//   words     k_enc_words: one wave per unique word -- the ids of its tokens, their number and the checksum fold
//   emit      k_enc_count / exclusive_scan / k_enc_emit: per pre-token count -> id offsets -> u32 ids; k_enc_docs: the
//             per-document offsets into the ids
// With words (yabpe_encode_words): k_enc_docs also writes every document's first pre-token, and k_enc_emit_words takes
// k_enc_emit's place: beside each id, the index of its pre-token in its document and whether it is a special occurrence.
// With spans (yabpe_encode_spans): k_enc_words<true> also writes every token's byte offset inside its word, and
// k_enc_emit_spans writes (start, end) per id, relative to its document; in characters after k_enc_lead_count /
// exclusive_scan built the lead-byte prefix of the text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_logic.h"
#include "yabpe_pretok_kernels.h"

namespace yb {

// The tokenizer's special split: sflag[i] = 1 + special index at a taken special's first byte, ENC_INSIDE on its other
// bytes, 0 elsewhere (sflag zeroed by the caller).  meta holds the document marks only.  A 256-bit set of the specials'
// first bytes keeps nearly every thread out of the compare.
__global__ __launch_bounds__(BLOCK) void k_enc_special(const uint8_t *text, const uint8_t *meta, unsigned long long n, PtSpecials sp,
                                                       uint8_t *sflag) {
    __shared__ uint32_t s_first[8];
    if (threadIdx.x < 8) s_first[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < sp.n; s += BLOCK) atomicOr(&s_first[sp.bytes[sp.off[s]] >> 5], 1u << (sp.bytes[sp.off[s]] & 31));
    __syncthreads();
    const PtView v{text, meta, n, 0};
    const uint32_t *first = s_first;
    auto occ = [&](unsigned long long q) -> uint32_t {
        const uint8_t b = v.T(q);
        return ((first[b >> 5] >> (b & 31)) & 1u) ? pt_special_at(v, sp, q) : 0u;
    };
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) {
        const uint32_t o = occ(i);
        if (o && enc_special_is_head(v, sp, occ, i)) enc_special_walk(v, sp, occ, sflag, i, o);
    }
}

__global__ __launch_bounds__(BLOCK) void k_enc_segments(const uint8_t *sflag, unsigned long long n, uint8_t *meta) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK)
        if (enc_segment_start(sflag, i)) meta[i] |= PT_CHUNK0;
}

// (inside: 0, or GRP_INSIDE when the grouping pass follows -- it turns the mark into 0, group_logic.h)
__global__ __launch_bounds__(BLOCK) void k_enc_clear(const uint8_t *sflag, unsigned long long n, uint8_t *flags, uint8_t inside) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK)
        if (sflag[i] == ENC_INSIDE) flags[i] = inside;
}

// ulist[u] = the pre-token that represents unique word u; llen[u] = its length when it takes the sequential (long) path
__global__ void k_enc_compact(const uint32_t *flag, const unsigned long long *uidx, const unsigned long long *off, unsigned long long n,
                              uint32_t *ulist, uint32_t *llen) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n || !flag[w]) return;
    const unsigned long long u = uidx[w], L = off[w + 1] - off[w];
    ulist[u] = (uint32_t)w;
    llen[u] = L > ENC_SHORT ? (uint32_t)L : 0u;
}

struct EncWordsParams {
    const uint8_t *text;
    const unsigned long long *off;    // pre-token offsets
    const uint32_t *ulist;            // unique word -> representative pre-token
    unsigned long long n_unique;
    const unsigned long long *uoff;   // per representative: first slot of its ids in uids
    const unsigned long long *lbase;  // per unique word: first slot of its long-path scratch
    const unsigned long long *count;  // per representative: occurrences (k_word_dedup)
    const uint8_t *sflag;             // nullptr without specials
    EncTable tab;
    const uint32_t *out_id;           // internal id -> output id
    const uint32_t *sp_id;
    const uint8_t *sp_has;
    uint32_t *wcnt;                   // out, per representative: number of ids
    uint32_t *uids;                   // out: the ids of every unique word
    uint32_t *upos;                   // out (SPANS): per slot of uids, the token's byte offset inside its word
    uint32_t *ltok, *lnxt, *lprv;     // long-path scratch
    unsigned long long *lheap;
    unsigned long long *sums;         // [0] checksum [1] words [2] tokens: over the words of >= 2 tokens (encode_logic.h); [3] specials
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o);
        x = y < x ? y : x;
    }
    return x;
}

// One wave per unique word.  Words of at most 64 bytes: lane p holds the token that starts at byte p (while one does) and
// the rank of the pair it begins; each step takes the smallest (rank, position) by a wave reduction, and only the two lanes
// whose pair changed look the table up again.  Longer words: lane 0 runs the heap walk of encode_logic.h in global scratch.
// SPANS: beside each id, the byte offset of its token inside the word (the lane; on the long path the walk's list).
template <bool SPANS>
__global__ __launch_bounds__(BLOCK) void k_enc_words(EncWordsParams P) {
    const int lane = threadIdx.x & 63;
    const unsigned long long wave0 = (unsigned long long)blockIdx.x * WPB + (threadIdx.x >> 6), waves = (unsigned long long)gridDim.x * WPB;
    unsigned long long sum = 0, words = 0, tokens = 0; // (lane 0's)
    for (unsigned long long u = wave0; u < P.n_unique; u += waves) {
        const uint32_t w = P.ulist[u];
        const unsigned long long s = P.off[w], base = P.uoff[w];
        const uint32_t L = (uint32_t)(P.off[w + 1] - s);
        const uint8_t sf = P.sflag ? P.sflag[s] : 0;
        if (sf) { // a special (its own pre-token): its id, or nothing
            if (lane == 0) {
                const uint32_t k = sf - 1u;
                P.wcnt[w] = P.sp_has[k] ? 1u : 0u;
                if (P.sp_has[k]) P.uids[base] = P.sp_id[k];
                if (SPANS && P.sp_has[k]) P.upos[base] = 0u;
                atomicAdd(&P.sums[3], P.count[w]);
            }
            continue;
        }
        const unsigned long long f = P.count[w];
        if (L > ENC_SHORT) {
            if (lane == 0) {
                const unsigned long long lb = P.lbase[u];
                uint32_t *tok = P.ltok + lb, *nxt = P.lnxt + lb;
                const uint32_t cnt = enc_merge_heap(P.text + s, L, P.tab, tok, nxt, P.lprv + lb, P.lheap + 3 * lb);
                for (uint32_t k = 0; k < cnt; ++k) P.uids[base + k] = P.out_id[tok[k]];
                if (SPANS)
                    for (uint32_t k = 0; k < cnt; ++k) P.upos[base + k] = enc_heap_start(nxt, k);
                P.wcnt[w] = cnt;
                if (cnt >= 2) {
                    sum += f * enc_word_hash(P.text + s, L, nxt, cnt);
                    words += f;
                    tokens += f * cnt;
                }
            }
            continue;
        }
        uint32_t tok = lane < (int)L ? P.text[s + lane] : 0u;
        bool alive = lane < (int)L, dirty = true;
        uint32_t rk = ENC_NONE, res = 0;
        unsigned long long am = __ballot(alive);
        while (true) {
            const unsigned long long above = am & ~((2ull << lane) - 1ull);
            const int nx = above ? __ffsll((long long)above) - 1 : -1;
            const uint32_t ntok = __shfl(tok, nx < 0 ? lane : nx);
            if (dirty) {
                rk = ENC_NONE;
                if (alive && nx >= 0 && !enc_lookup(P.tab, tok, ntok, &rk, &res)) rk = ENC_NONE;
                dirty = false;
            }
            const unsigned long long key = (alive && rk != ENC_NONE) ? (((unsigned long long)rk << 6) | (unsigned)lane) : ~0ull;
            const unsigned long long m = wave_min_u64(key);
            if (m == ~0ull) break;
            const int win = (int)(m & 63);
            const int right = __shfl(nx, win);
            const unsigned long long below = am & ((1ull << win) - 1ull);
            const int pv = below ? 63 - __clzll((long long)below) : -1;
            if (lane == win) {
                tok = res;
                dirty = true;
            }
            if (lane == right) alive = false;
            if (lane == pv) dirty = true;
            am &= ~(1ull << right);
        }
        const uint32_t cnt = (uint32_t)__popcll(am);
        if (alive) P.uids[base + __popcll(am & ((1ull << lane) - 1ull))] = P.out_id[tok];
        if (SPANS && alive) P.upos[base + __popcll(am & ((1ull << lane) - 1ull))] = (uint32_t)lane;
        // the checksum fold: every lane walks the word's bytes with the token boundaries of the alive mask (same value in all)
        unsigned long long h = enc_fnv_init();
        for (uint32_t p = 0; p < L; ++p) {
            h = enc_fnv_byte(h, P.text[s + p]);
            if (p + 1 == L || ((am >> (p + 1)) & 1ull)) h = enc_fnv_mark(h);
        }
        if (lane == 0) {
            P.wcnt[w] = cnt;
            if (cnt >= 2) {
                sum += f * enc_fnv_final(h);
                words += f;
                tokens += f * cnt;
            }
        }
    }
    if (lane == 0 && words) {
        atomicAdd(&P.sums[0], sum);
        atomicAdd(&P.sums[1], words);
        atomicAdd(&P.sums[2], tokens);
    }
}

// per pre-token: the number of ids of its unique word
__global__ void k_enc_count(const uint32_t *rep, const uint32_t *wcnt, unsigned long long n, uint32_t *cnt) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n) cnt[w] = wcnt[rep[w]];
}

__global__ void k_enc_emit(const uint32_t *rep, const unsigned long long *uoff, const uint32_t *uids, const unsigned long long *id_off,
                           unsigned long long n, uint32_t *ids) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const unsigned long long a = id_off[w], e = id_off[w + 1];
    const uint32_t *src = uids + uoff[rep[w]];
    for (unsigned long long k = a; k < e; ++k) ids[k] = src[k - a];
}

// k_enc_emit that also says which piece of its document every id was made from (yabpe_encode_words): words[k] = the index of
// pre-token w among the pre-tokens of its document, with ENC_WORD_SPECIAL set when w is a special occurrence.  doc_pre[d] =
// the first pre-token of document d (k_enc_docs; n_docs + 1 entries, ascending): the document of w is the last d with
// doc_pre[d] <= w, searched between the documents of the block's first and last pre-token as k_enc_emit_spans does.  A
// pre-token without ids (a special the vocab lacks) writes nothing and still counts: the indices of its document have a gap.
__global__ __launch_bounds__(256) void k_enc_emit_words(const uint32_t *rep, const unsigned long long *uoff, const uint32_t *uids,
                                                        const unsigned long long *id_off, const unsigned long long *off, unsigned long long n,
                                                        const uint32_t *doc_pre, uint32_t n_docs, const uint8_t *sflag, uint32_t *ids,
                                                        uint32_t *words) {
    __shared__ uint32_t s_doc[2];
    auto doc_of = [&](unsigned long long w, uint32_t lo, uint32_t hi) -> uint32_t { // last d in [lo, hi] with doc_pre[d] <= w
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (doc_pre[mid] <= w) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    const unsigned long long w0 = (unsigned long long)blockIdx.x * blockDim.x, w = w0 + threadIdx.x;
    if (threadIdx.x < 2) {
        const unsigned long long wl = w0 + blockDim.x - 1 < n ? w0 + blockDim.x - 1 : n - 1;
        s_doc[threadIdx.x] = doc_of(threadIdx.x ? wl : w0, 0, n_docs - 1);
    }
    __syncthreads();
    if (w >= n) return;
    const unsigned long long a = id_off[w], e = id_off[w + 1];
    if (a == e) return;
    const uint32_t word = (uint32_t)(w - doc_pre[doc_of(w, s_doc[0], s_doc[1])]) | ((sflag && sflag[off[w]]) ? ENC_WORD_SPECIAL : 0u);
    const uint32_t *src = uids + uoff[rep[w]];
    for (unsigned long long k = a; k < e; ++k) {
        ids[k] = src[k - a];
        words[k] = word;
    }
}

// cnt[g] = the non-continuation bytes of granule g (ENC_GRANULE bytes of text, 16-byte aligned): one 16-byte chunk per
// thread, four neighbouring lanes make a granule.  Its exclusive scan is enc_lead's table.
__global__ __launch_bounds__(BLOCK) void k_enc_lead_count(const uint8_t *text, unsigned long long n, uint8_t *cnt) {
    const unsigned long long t = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, c = t * 16; // (whole waves run: the shuffles below)
    uint32_t v = c < n ? enc_lead_chunk(text, n, c, n - c < 16 ? (uint32_t)(n - c) : 16u) : 0u;
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    if ((threadIdx.x & 3) == 0 && c < n) cnt[t >> 2] = (uint8_t)v;
}

// The spans of every id: (start, end) relative to the id's document, one 16-byte store each.  Bytes: start = pre-token
// offset + in-word offset - document start, end = the next token's start or the pre-token's end.  CHARS: both ends by the
// lead rule of encode_logic.h.  A pre-token never crosses a document start; its document is searched between the documents
// of the block's first and last pre-token (nearly always the same one: no search).
template <bool CHARS>
__global__ __launch_bounds__(256) void k_enc_emit_spans(const uint32_t *rep, const unsigned long long *uoff, const uint32_t *upos,
                                                        const unsigned long long *id_off, const unsigned long long *off, unsigned long long n,
                                                        const unsigned long long *doc_start, uint32_t n_docs, const uint8_t *text,
                                                        unsigned long long n_bytes, const unsigned long long *lead_table, ulonglong2 *spans) {
    __shared__ uint32_t s_doc[2];
    auto doc_of = [&](unsigned long long pos, uint32_t lo, uint32_t hi) -> uint32_t { // last d in [lo, hi] with doc_start[d] <= pos
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (doc_start[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    const unsigned long long w0 = (unsigned long long)blockIdx.x * blockDim.x, w = w0 + threadIdx.x;
    if (threadIdx.x < 2) {
        const unsigned long long wl = w0 + blockDim.x - 1 < n ? w0 + blockDim.x - 1 : n - 1;
        s_doc[threadIdx.x] = doc_of(off[threadIdx.x ? wl : w0], 0, n_docs - 1);
    }
    __syncthreads();
    if (w >= n) return;
    const unsigned long long a = id_off[w], e = id_off[w + 1];
    if (a == e) return;
    const unsigned long long ws = off[w], we = off[w + 1];
    const unsigned long long ds = doc_start[doc_of(ws, s_doc[0], s_doc[1])];
    const uint32_t *src = upos + uoff[rep[w]];
    auto lead = [&](unsigned long long p) { return enc_lead(text, n_bytes, lead_table, p); };
    const unsigned long long dl = CHARS ? lead(ds) : 0ull;
    unsigned long long st = ws + src[0], ls = CHARS ? lead(st) : 0ull; // ls = lead(st): the previous token's lead(end)
    for (unsigned long long k = a; k < e; ++k) {
        const unsigned long long en = k + 1 < e ? ws + src[k + 1 - a] : we;
        if (CHARS) {
            auto lead_next = [&](unsigned long long p) { return ls + (enc_is_lead(text[p - 1]) ? 1ull : 0ull); }; // lead(st + 1)
            const unsigned long long le = enc_char_end(lead, en);
            spans[k] = make_ulonglong2(enc_char_start(lead_next, st) - dl, le - dl);
            ls = le;
        } else {
            spans[k] = make_ulonglong2(st - ds, en - ds);
        }
        st = en;
    }
}

// doc_ids[d] = id offset of the first pre-token at or after document d's start (d == n_docs: the total); doc_pre (nullptr:
// not wanted) [d] = that pre-token's index
__global__ void k_enc_docs(const unsigned long long *doc_start, uint32_t n_docs, unsigned long long n_bytes, const unsigned long long *off,
                           unsigned long long n_pre, const unsigned long long *id_off, unsigned long long *doc_ids, uint32_t *doc_pre) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    const unsigned long long pos = d < n_docs ? doc_start[d] : n_bytes;
    unsigned long long lo = 0, hi = n_pre; // first w with off[w] >= pos (off[n_pre] = n_bytes)
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (off[mid] >= pos) hi = mid; else lo = mid + 1;
    }
    doc_ids[d] = id_off[lo];
    if (doc_pre) doc_pre[d] = (uint32_t)lo;
}

} // namespace yb
