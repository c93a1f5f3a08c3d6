// yabpe_layout_kernels.h -- ragged ids + document starts -> the two fixed shapes a model consumes (rules in layout_logic.h;
// contract: BBPETokenizer.encode_batch_padded / encode_batch_packed, yet_another_bpe/tokenizer.py).
//
// Passes (host orchestration: yabpe_layout_pad / yabpe_layout_pack in yabpe.hip):
//   lengths   k_lay_lengths: one thread per document.  Padded: the kept length of every row, and per call the longest
//             sequence, the truncated documents, the ids dropped and the slots kept (one atomic per counter and workgroup).
//             Packed: the stream offsets soff[n_docs + 1] in their closed form doc_off[d] + n_added * d (layout_logic.h: the ids
//             already lie end to end, so the exclusive scan of len(seq(d)) needs no scan pass), and the longest sequence.
//   write     k_lay_pad_write / k_lay_pack_write: the output is indexed flat; a thread owns 4 consecutive slots per step,
//             resolves each of them and stores 16 bytes (output buffers are 256-B aligned, so a store at a flat index that is a
//             multiple of 4 is aligned whatever row_len is).  A workgroup owns LAY_PIECE consecutive slots.  The packed form
//             finds the piece's first and last document by binary search in soff and stages that window in LDS; a window of
//             more than LAY_STAGE offsets (many tiny documents in one piece) is searched in global memory instead.  The pad
//             tail of the last packed row is written by the same kernel.
//
// Windows (yabpe_layout_windows; contract: BBPETokenizer.encode_batch_windows): a document becomes lay_win_rows rows, so the
// first row of a document has no closed form:
//   count     k_lay_win_count: one thread per document writes its row count; per call the longest document, the documents of
//             more than one row and the slots kept (one atomic per counter and workgroup).  exclusive_scan -> row_off.
//   rows      k_lay_win_rows: one thread per output row searches row_off once and writes row_doc, row_start, row_len and the
//             row's record (first source id, content ids kept).
//   write     k_lay_rows_write<LayWinRow, SPANS>: k_lay_pad_write's shape with one record read per row touched.
//
// Pairs (yabpe_layout_pairs; contract: BBPETokenizer.encode_batch_pairs): documents 2p and 2p + 1 share a row, cut by one of
// three truncation rules (one row a pair) or with the second side windowed behind the whole first (Rule 4 of layout_logic.h):
//   count     k_lay_pair_count: one thread per pair: the call's counters and, in windows mode only, its row count.  The
//             truncation modes have one row a pair, so their row_off is the identity and no scan runs.
//   rows      k_lay_pair_rows: one thread per output row (windows mode: one search in row_off) writes row_pair, row_start,
//             first_len, second_len and the row's record (where each side's kept ids start, how many they are).
//   write     k_lay_rows_write<LayPairRow, SPANS>: next to the 16 bytes of ids a thread stores its 4 slots' type bytes as one
//             aligned u32.
// Windows and pairs share the write kernel: a row policy (LayWinRow / LayPairRow) names the record of a row, the rule that
// resolves a slot of it and the id a resolved slot holds; SPANS also stores the 16-byte span of every slot.  The three count
// kernels (k_lay_lengths, k_lay_win_count, k_lay_pair_count) end in lay_commit.
// No workgroup waits for another; every loop runs over LAY_VPT steps or a search in an array whose length is given.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout_logic.h"
#include "yabpe_kernels.h" // BLOCK, WPB

namespace yb {

constexpr int LAY_VPT = 4;                     // 16-byte stores per thread (and output array)
constexpr int LAY_PIECE = BLOCK * 4 * LAY_VPT; // output slots per workgroup
constexpr int LAY_STAGE = 2048;                // stream offsets the packed write stages in LDS (16 KiB)

struct LayLenParams {
    const unsigned long long *doc;  // n_docs document starts (ids), ascending, doc[0] = 0
    uint32_t n_docs;
    unsigned long long n_ids;
    uint32_t row_len, flags;        // padded: row_len 0 = no cut (the longest sequence becomes the row length)
    uint32_t *len;                  // out, padded: kept length per document
    unsigned long long *soff;       // out, packed: n_docs + 1 stream offsets
    unsigned long long *counters;   // [0] longest sequence; padded also [1] truncated documents [2] ids dropped [3] slots kept
};

// How a count kernel ends.  The call's counters over a workgroup: v[0] by maximum, v[1..3] by sum; thread 0 then commits the
// maximum and (SUMS) the sums that are not zero: one atomic per counter and workgroup.
template <bool SUMS>
__device__ __forceinline__ void lay_commit(unsigned long long (&v)[4], unsigned long long *counters) {
    __shared__ unsigned long long s_red[WPB][4];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long m = __shfl_xor(v[0], o);
        v[0] = m > v[0] ? m : v[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) v[k] += __shfl_xor(v[k], o);
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k) s_red[wib][k] = v[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < WPB; ++w) {
        v[0] = s_red[w][0] > v[0] ? s_red[w][0] : v[0];
        for (int k = 1; k < 4; ++k) v[k] += s_red[w][k];
    }
    atomicMax(&counters[0], v[0]);
    if (SUMS)
        for (int k = 1; k < 4; ++k)
            if (v[k]) atomicAdd(&counters[k], v[k]);
}

template <bool PACK>
__global__ __launch_bounds__(BLOCK) void k_lay_lengths(LayLenParams P) {
    const unsigned long long d = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t added = lay_n_added(P.flags);
    unsigned long long v[4] = {0, 0, 0, 0}; // max, truncated, dropped, kept
    if (d < P.n_docs) {
        const unsigned long long a = P.doc[d], b = d + 1 < P.n_docs ? P.doc[d + 1] : P.n_ids;
        const unsigned long long seq = b - a + added;
        v[0] = seq;
        if (PACK) {
            P.soff[d] = a + added * d;
            if (d + 1 == P.n_docs) P.soff[d + 1] = P.n_ids + (unsigned long long)added * P.n_docs;
        } else {
            const unsigned long long kept = P.row_len ? lay_kept(b - a, P.row_len, P.flags) : seq;
            P.len[d] = (uint32_t)kept;
            v[1] = seq > kept ? 1u : 0u;
            v[2] = seq - kept;
            v[3] = kept;
        }
    }
    lay_commit<!PACK>(v, P.counters);
}

struct LayConst {
    uint32_t pad_id, bos_id, eos_id;
};

// the id a resolved slot holds (slot: an index into ids or one of LAY_SLOT_*)
__device__ __forceinline__ uint32_t lay_value(const uint32_t *ids, unsigned long long slot, const LayConst &K) {
    if (slot == LAY_SLOT_PAD) return K.pad_id;
    if (slot == LAY_SLOT_BOS) return K.bos_id;
    if (slot == LAY_SLOT_EOS) return K.eos_id;
    return ids[slot];
}

// 4 slots at flat index f (a multiple of 4) of an array of n_slots: one 16-B store, or the last 1..3 slots one by one
__device__ __forceinline__ void lay_store4(uint32_t *out, unsigned long long f, unsigned long long n_slots, const uint32_t (&v)[4]) {
    if (f + 4 <= n_slots) {
        *reinterpret_cast<uint4 *>(out + f) = make_uint4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int k = 0; k < 4; ++k)
        if (f + k < n_slots) out[f + k] = v[k];
}

// (row, col) of flat slot f; narrow (uniform): the 32-bit division
__device__ __forceinline__ void lay_row_col(unsigned long long f, uint32_t row_len, bool narrow, unsigned long long *row, uint32_t *col) {
    if (narrow) {
        *row = (uint32_t)f / row_len;
        *col = (uint32_t)f % row_len;
    } else {
        *row = f / row_len;
        *col = (uint32_t)(f % row_len);
    }
}

struct LayPadParams {
    const uint32_t *ids;
    const unsigned long long *doc;  // n_docs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    uint32_t row_len, flags;        // row_len >= 1
    LayConst K;
    uint32_t *rows;                 // out: n_docs * row_len slots
    unsigned long long n_slots;
};

__global__ __launch_bounds__(BLOCK) void k_lay_pad_write(LayPadParams P) {
    const unsigned long long f0 = (unsigned long long)blockIdx.x * LAY_PIECE;
    const bool narrow = P.n_slots <= 0xFFFFFFFFull; // (uniform: the 32-bit division then)
#pragma unroll
    for (int s = 0; s < LAY_VPT; ++s) {
        const unsigned long long f = f0 + ((unsigned long long)s * BLOCK + threadIdx.x) * 4;
        if (f >= P.n_slots) break;
        unsigned long long row;
        uint32_t col;
        lay_row_col(f, P.row_len, narrow, &row, &col);
        unsigned long long a = P.doc[row], b = row + 1 < P.n_docs ? P.doc[row + 1] : P.n_ids;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (f + k >= P.n_slots) break;
            v[k] = lay_value(P.ids, lay_pad_slot(a, b - a, P.row_len, P.flags, col), P.K);
            if (++col == P.row_len && row + 1 < P.n_docs) { // the next slot opens the next row
                col = 0;
                ++row;
                a = b;
                b = row + 1 < P.n_docs ? P.doc[row + 1] : P.n_ids;
            }
        }
        lay_store4(P.rows, f, P.n_slots, v);
    }
}

struct LayPackParams {
    const uint32_t *ids;
    const unsigned long long *soff; // n_docs + 1 stream offsets (k_lay_lengths<true>)
    uint32_t n_docs;
    unsigned long long total;       // stream positions: soff[n_docs]
    unsigned long long n_slots;     // n_rows * row_len: slots at or past `total` are the pad tail
    uint32_t flags;
    LayConst K;
    uint32_t *out_ids, *out_doc, *out_pos;
};

// The slots of one lane: w = the stream offsets of the documents [d0, d1 + 1] seen through the origin org (w[d - org]).
__device__ __forceinline__ void lay_pack_lane(const LayPackParams &P, const unsigned long long *w, uint32_t org, uint32_t d0, uint32_t d1,
                                              unsigned long long g0, unsigned long long g1) {
#pragma unroll
    for (int s = 0; s < LAY_VPT; ++s) {
        const unsigned long long g = g0 + ((unsigned long long)s * BLOCK + threadIdx.x) * 4;
        if (g >= g1) break;
        uint32_t vi[4] = {0, 0, 0, 0}, vd[4] = {0, 0, 0, 0}, vp[4] = {0, 0, 0, 0};
        uint32_t d = d0;
        unsigned long long sd = 0, next = 0; // soff[d], soff[d + 1]; next = 0: not looked up yet
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long gg = g + k;
            if (gg >= g1) break; // (the last vector of the output: slots that do not exist; [d0, d1] does not cover them)
            if (gg >= P.total) { // the pad tail
                vi[k] = P.K.pad_id;
                vd[k] = LAY_NO_DOC;
                continue;
            }
            if (gg >= next) { // the first slot, or the document ended: the last document that starts at or before gg
                d = lay_find_doc(w, org, next ? d + 1 : d0, d1, gg);
                sd = w[d - org];
                next = w[d + 1 - org];
            }
            unsigned long long pos;
            vi[k] = lay_value(P.ids, lay_pack_slot(gg, d, sd, next, P.flags, &pos), P.K);
            vd[k] = d;
            vp[k] = (uint32_t)pos;
        }
        lay_store4(P.out_ids, g, P.n_slots, vi);
        lay_store4(P.out_doc, g, P.n_slots, vd);
        lay_store4(P.out_pos, g, P.n_slots, vp);
    }
}

__global__ __launch_bounds__(BLOCK) void k_lay_pack_write(LayPackParams P) {
    __shared__ unsigned long long s_off[LAY_STAGE];
    __shared__ uint32_t s_d[2];
    const unsigned long long g0 = (unsigned long long)blockIdx.x * LAY_PIECE;
    const unsigned long long g1 = g0 + LAY_PIECE < P.n_slots ? g0 + LAY_PIECE : P.n_slots;
    const unsigned long long e = g1 < P.total ? g1 : P.total; // end of the piece's part of the stream
    uint32_t d0 = 0, d1 = 0;
    bool staged = false;
    if (g0 < e) { // (uniform)
        if (threadIdx.x == 0) {
            s_d[0] = lay_find_doc(P.soff, 0, 0, P.n_docs - 1, g0);
            s_d[1] = lay_find_doc(P.soff, 0, s_d[0], P.n_docs - 1, e - 1);
        }
        __syncthreads();
        d0 = s_d[0];
        d1 = s_d[1];
        staged = d1 - d0 + 2 <= (uint32_t)LAY_STAGE;
        if (staged) {
            for (uint32_t i = threadIdx.x; i < d1 - d0 + 2; i += BLOCK) s_off[i] = P.soff[d0 + i];
            __syncthreads();
        }
    }
    if (staged)
        lay_pack_lane(P, s_off, d0, d0, d1, g0, g1);
    else
        lay_pack_lane(P, P.soff, 0, d0, d1, g0, g1);
}

// ---- windows (yabpe_layout_windows): C content slots a row, consecutive rows of a document step ids apart
struct LayWinCountParams {
    const unsigned long long *doc;  // n_docs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    uint32_t C, step, added;
    unsigned long long *rows;       // out: rows per document (their exclusive scan is row_off)
    unsigned long long *counters;   // [0] longest document (ids) [1] documents of more than one row [3] slots kept
};

__global__ __launch_bounds__(BLOCK) void k_lay_win_count(LayWinCountParams P) {
    const unsigned long long d = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long v[4] = {0, 0, 0, 0}; // max, more than one row, (unused), kept
    if (d < P.n_docs) {
        const unsigned long long a = P.doc[d], b = d + 1 < P.n_docs ? P.doc[d + 1] : P.n_ids;
        const unsigned long long n = b - a, rows = lay_win_rows(n, P.C, P.step);
        P.rows[d] = rows;
        v[0] = n;
        v[1] = rows > 1 ? 1u : 0u;
        v[3] = rows * P.added + (rows - 1) * P.C + lay_win_content(n, rows - 1, P.C, P.step); // every row but the last is full
    }
    lay_commit<true>(v, P.counters);
}

struct LayWinRowsParams {
    const unsigned long long *doc;      // n_docs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    const unsigned long long *row_off;  // n_docs + 1: the first output row of every document
    unsigned long long n_rows;          // row_off[n_docs]
    uint32_t C, step, added;
    uint32_t *row_doc, *row_start, *row_len; // out, per output row
    ulonglong2 *rec;                    // out, per output row: (index into ids of its first content id, content ids it keeps)
};

__global__ __launch_bounds__(BLOCK) void k_lay_win_rows(LayWinRowsParams P) {
    const unsigned long long r = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= P.n_rows) return;
    const uint32_t d = lay_find_doc(P.row_off, 0, 0, P.n_docs - 1, r);
    const unsigned long long k = r - P.row_off[d];
    const unsigned long long a = P.doc[d], b = d + 1 < P.n_docs ? P.doc[d + 1] : P.n_ids;
    const unsigned long long content = lay_win_content(b - a, k, P.C, P.step);
    P.row_doc[r] = d;
    P.row_start[r] = (uint32_t)(k * P.step);
    P.row_len[r] = (uint32_t)content + P.added;
    P.rec[r] = make_ulonglong2(a + k * P.step, content);
}

// ---- pairs (yabpe_layout_pairs): documents 2p and 2p + 1 share rows of C content slots (Rule 4 of layout_logic.h)
struct LayPairShape {
    uint32_t C, mode, stride, n_sep, added; // added = BOS + EOS + n_sep
};

// the ids of pair p: the first side is ids[*a, *b), the second ids[*b, *e)
__device__ __forceinline__ void lay_pair_docs(const unsigned long long *doc, uint32_t n_docs, unsigned long long n_ids, unsigned long long p,
                                              unsigned long long *a, unsigned long long *b, unsigned long long *e) {
    *a = doc[2 * p];
    *b = doc[2 * p + 1];
    *e = 2 * p + 2 < n_docs ? doc[2 * p + 2] : n_ids;
}

struct LayPairCountParams {
    const unsigned long long *doc;  // n_docs = 2 * n_pairs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    LayPairShape S;
    unsigned long long *rows;       // out, windows mode: rows per pair (their exclusive scan is row_off); else NULL
    unsigned long long *counters;   // [0] longest document (ids) [1] pairs that lost an id or took several rows [2] ids dropped [3] slots kept
};

__global__ __launch_bounds__(BLOCK) void k_lay_pair_count(LayPairCountParams P) {
    const unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long v[4] = {0, 0, 0, 0}; // max, cut, dropped, kept
    if (2 * p < P.n_docs) {
        unsigned long long a, b, e;
        lay_pair_docs(P.doc, P.n_docs, P.n_ids, p, &a, &b, &e);
        const unsigned long long la = b - a, lb = e - b;
        v[0] = la > lb ? la : lb;
        if (P.S.mode == LAY_PAIRS_WINDOWS) {
            const unsigned long long ka = lay_pair_first(la, P.S.C, P.S.stride), Cb = P.S.C - ka, step = Cb - P.S.stride;
            const unsigned long long rows = lay_win_rows(lb, Cb, step);
            P.rows[p] = rows;
            v[1] = rows > 1 || ka < la ? 1u : 0u;
            v[3] = rows * (P.S.added + ka) + (rows - 1) * Cb + lay_win_content(lb, rows - 1, Cb, step); // every row but the last is full
        } else {
            unsigned long long ka, kb;
            lay_pair_keep(la, lb, P.S.C, P.S.mode, &ka, &kb);
            v[1] = ka + kb < la + lb ? 1u : 0u;
            v[2] = la + lb - ka - kb;
            v[3] = P.S.added + ka + kb;
        }
    }
    lay_commit<true>(v, P.counters);
}

// what the write pass needs of an output row
struct LayPairRec {
    unsigned long long a0, b0;      // index into ids of the first id it keeps of the first side, of the second side
    uint32_t ka, kb;                // ids kept of each
};

struct LayPairRowsParams {
    const unsigned long long *doc;      // n_docs document starts
    uint32_t n_docs;
    unsigned long long n_ids;
    const unsigned long long *row_off;  // windows mode: n_pairs + 1, the first output row of every pair; else NULL (row p = pair p)
    unsigned long long n_rows;
    LayPairShape S;
    uint32_t *row_pair, *row_start, *first_len, *second_len; // out, per output row
    LayPairRec *rec;                    // out, per output row
};

__global__ __launch_bounds__(BLOCK) void k_lay_pair_rows(LayPairRowsParams P) {
    const unsigned long long r = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= P.n_rows) return;
    unsigned long long p = r, k = 0;
    if (P.row_off) {
        p = lay_find_doc(P.row_off, 0, 0, P.n_docs / 2 - 1, r);
        k = r - P.row_off[p];
    }
    unsigned long long a, b, e, ka, s, kb;
    lay_pair_docs(P.doc, P.n_docs, P.n_ids, p, &a, &b, &e);
    lay_pair_row(b - a, e - b, k, P.S.C, P.S.mode, P.S.stride, &ka, &s, &kb);
    P.row_pair[r] = (uint32_t)p;
    P.row_start[r] = (uint32_t)s;
    P.first_len[r] = (uint32_t)ka;
    P.second_len[r] = (uint32_t)kb;
    P.rec[r] = LayPairRec{a, b + s, (uint32_t)ka, (uint32_t)kb};
}

// ---- the write pass of windows and pairs: one record per output row
// A row policy has: Rec, the record of a row; TYPES, whether a type byte a slot is stored; slot(), the rule of layout_logic.h that
// resolves slot `col` of a row; value(), the id a resolved slot holds.
struct LayWinRow {
    using Rec = ulonglong2;         // (index into ids of the row's first content id, content ids it keeps)
    static constexpr bool TYPES = false;
    __device__ __forceinline__ unsigned long long slot(const Rec &rec, uint32_t row_len, uint32_t flags, uint32_t col, uint32_t *) const {
        return lay_win_row_slot(rec.x, rec.y, row_len, flags, col);
    }
    __device__ __forceinline__ uint32_t value(const uint32_t *ids, unsigned long long slot, const LayConst &K) const {
        return lay_value(ids, slot, K);
    }
};

struct LayPairRow {
    using Rec = LayPairRec;
    static constexpr bool TYPES = true;
    uint32_t n_sep, sep_id;
    __device__ __forceinline__ unsigned long long slot(const Rec &rec, uint32_t row_len, uint32_t flags, uint32_t col, uint32_t *type) const {
        return lay_pair_slot(rec.a0, rec.ka, rec.b0, rec.kb, n_sep, row_len, flags, col, type);
    }
    __device__ __forceinline__ uint32_t value(const uint32_t *ids, unsigned long long slot, const LayConst &K) const {
        return slot == LAY_SLOT_SEP ? sep_id : lay_value(ids, slot, K);
    }
};

template <class Row>
struct LayRowsParams {
    const uint32_t *ids;
    const typename Row::Rec *rec;   // n_rows row records (k_lay_win_rows / k_lay_pair_rows)
    unsigned long long n_rows;
    uint32_t row_len, flags;
    Row R;
    LayConst K;
    uint32_t *rows;                 // out: n_rows * row_len slots
    uint8_t *types;                 // out, Row::TYPES: one byte per slot
    unsigned long long n_slots;
    const ulonglong2 *spans;        // SPANS: one (start, end) per id ...
    ulonglong2 *out_spans;          // ... and per output slot
};

// k_lay_pad_write's shape: a row's ids are those of its record instead of a whole document.  The 4 slots a thread owns per step
// are 16 bytes of ids and (Row::TYPES) 4 bytes of types: the flat index of the first is a multiple of 4, so both stores are aligned
// whatever row_len is, and a wave's type bytes lie end to end (256 B a step).  The last 1..3 slots of the output are stored one by
// one.  SPANS: also the span of every slot, in a pass of its own over the same 256 slots of a wave and step: lane l takes the
// slots l, 64 + l, 128 + l and 192 + l, so the 16-byte loads and stores of a wave lie end to end (4 consecutive slots a lane would
// put 64 bytes between neighbouring lanes).  A slot below LAY_SLOT_SEP, the lowest of the constants, is a source id and has a span.
template <class Row, bool SPANS>
__global__ __launch_bounds__(BLOCK) void k_lay_rows_write(LayRowsParams<Row> P) {
    using Rec = typename Row::Rec;
    const unsigned long long f0 = (unsigned long long)blockIdx.x * LAY_PIECE;
    const bool narrow = P.n_slots <= 0xFFFFFFFFull; // (uniform: the 32-bit division then)
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < LAY_VPT; ++s) {
        const unsigned long long f = f0 + ((unsigned long long)s * BLOCK + threadIdx.x) * 4;
        const unsigned long long fw = f - 4ull * lane; // the wave's first slot
        if ((SPANS ? fw : f) >= P.n_slots) break;
        if (!SPANS || f < P.n_slots) {
            unsigned long long row;
            uint32_t col;
            lay_row_col(f, P.row_len, narrow, &row, &col);
            Rec rec = P.rec[row];
            uint32_t v[4] = {0, 0, 0, 0}, t[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) { // (past the last slot col runs on past the row's end: a pad slot that is never stored)
                v[k] = P.R.value(P.ids, P.R.slot(rec, P.row_len, P.flags, col, &t[k]), P.K);
                if (++col == P.row_len && row + 1 < P.n_rows) { // the next slot opens the next row
                    col = 0;
                    rec = P.rec[++row];
                }
            }
            lay_store4(P.rows, f, P.n_slots, v);
            if (Row::TYPES) {
                if (f + 4 <= P.n_slots) {
                    *reinterpret_cast<uint32_t *>(P.types + f) = t[0] | t[1] << 8 | t[2] << 16 | t[3] << 24;
                } else {
                    for (int k = 0; k < 4; ++k)
                        if (f + k < P.n_slots) P.types[f + k] = (uint8_t)t[k];
                }
            }
        }
        if (SPANS) {
            unsigned long long sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0}; // the slots' (start, end)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long g = fw + 64 * k + lane;
                if (g < P.n_slots) {
                    unsigned long long row;
                    uint32_t col, type;
                    lay_row_col(g, P.row_len, narrow, &row, &col);
                    const Rec rec = P.rec[row];
                    const unsigned long long slot = P.R.slot(rec, P.row_len, P.flags, col, &type);
                    if (slot < LAY_SLOT_SEP) {
                        const ulonglong2 sp = P.spans[slot];
                        sa[k] = sp.x;
                        sb[k] = sp.y;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (fw + 64 * k + lane < P.n_slots) P.out_spans[fw + 64 * k + lane] = make_ulonglong2(sa[k], sb[k]);
        }
    }
}

} // namespace yb
