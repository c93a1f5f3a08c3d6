// yabpe_decrows_kernels.h -- BBPETokenizer.decode_rows / decode_rows_with_offsets on the device (yet_another_bpe/tokenizer.py; the
// rules: DESIGN.md "Decoding id rows", the character-start rule in decode_logic.h).
//
// A [n_rows, row_len] matrix of ids comes in.  A wave owns a row and walks it in chunks of DROW_CHUNK columns, 16 bytes of ids a
// lane; rows start wherever n_rows * row_len puts them, so a chunk starts at the row's first id rounded down to 4 ids and the
// columns outside [0, row_len) are masked.  The stop and skip ids of the call are two sorted lists that every workgroup stages
// in LDS; a 64-bit filter in SGPRs (bit id & 63) answers for nearly every id without touching the lists.
//
// Passes (host orchestration: yabpe_decode_rows in yabpe.hip):
//   select    k_drow_select: the first stop column at or after the window's start (a ballot per chunk; the loop ends with the
//             chunk that holds it), the columns that remain tested against the skip list and the id table -> per row the
//             considered columns, the kept count and the kept byte length.  exclusive_scan of the counts -> where every row's
//             kept ids go (the document starts of the decoder); of the byte lengths -> every row's first byte in the text
//   compact   k_drow_compact: the kept ids of every row, in order, back to back.  yabpe_decode's lengths, gather, check and
//             repair passes run on them unchanged
//   chars     (offsets, or a row of 2^32 - 1 bytes or more) k_drow_chars: per DEC_TILE bytes of the gathered, unrepaired text,
//             tile and halo in LDS as in k_dec_check, a bit per byte that starts a character of the replace-mode decoding, the
//             count in front of every 64-byte word, the tile's count; exclusive_scan of the tile counts.  Row bounds are bits
//             in LDS set from the row byte offsets (one search per tile for the first row that starts in it)
//   spans     k_drow_spans: a wave per row again: the exclusive scan of the kept byte lengths along the row, carried across its
//             chunks, and per column nchars = tile prefix + word prefix + popcount of the mask below its byte, minus the row's
//             -> [n_rows, row_len, 2] u32, 8 bytes a column
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_logic.h"
#include "yabpe_decode_kernels.h"

namespace yb {

constexpr uint32_t DROW_MAX_STOP = 64;      // stop ids of one call (YABPE_DECODE_ROWS_MAX_STOP)
constexpr uint32_t DROW_MAX_SKIP = 1024;    // skip ids of one call (YABPE_DECODE_ROWS_MAX_SKIP)
constexpr int DROW_CHUNK = 64 * 4;          // columns a wave takes at a time: 16 bytes of ids a lane
constexpr int DROW_WORDS = DEC_TILE / 64;   // 64-byte mask words per text tile
constexpr uint32_t DROW_INCLUDE_STOP = 1u;  // flags (YABPE_DECODE_ROWS_INCLUDE_STOP)
constexpr uint32_t DROW_E_WINDOW = 1u, DROW_E_CHARS = 2u, DROW_BIG_ROW = 4u;  // bits of the call's status word
constexpr unsigned long long DROW_MAX_CHARS = 0xFFFFFFFFull;  // a row's text holds fewer characters (and spans are u32)

// The stop ids ([0, n_stop)) and skip ids ([n_stop, n_stop + n_skip)) of a call: each list sorted and unique, and its filter.
struct DrowSets {
    const uint32_t *ids;
    uint32_t n_stop, n_skip;
    unsigned long long f_stop, f_skip;  // bit (id & 63) set for every id of the list
};

__device__ __forceinline__ void drow_stage_sets(const DrowSets &S, uint32_t *s_set) {
    for (uint32_t i = threadIdx.x; i < S.n_stop + S.n_skip; i += BLOCK) s_set[i] = S.ids[i];
    __syncthreads();
}

// id is one of the n sorted ids at s (LDS)
__device__ __forceinline__ bool drow_has(const uint32_t *s, uint32_t n, unsigned long long filter, uint32_t id) {
    if (!((filter >> (id & 63u)) & 1ull)) return false;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && s[lo] == id;
}

// A row of the matrix as its wave sees it: lane l of chunk k holds the ids at g(k) .. g(k) + 3, columns col(k) .. col(k) + 3
// (the first chunk may start up to 3 columns in front of the row, the last one end behind it).
struct DrowRow {
    unsigned long long g0, a0, n;  // the row's first id, that rounded down to 4 ids, ids in the matrix
    __device__ DrowRow(uint32_t r, uint32_t row_len, uint32_t n_rows)
        : g0((unsigned long long)r * row_len), a0(g0 & ~3ull), n((unsigned long long)n_rows * row_len) {}
    __device__ unsigned long long g(unsigned long long k) const { return a0 + k * DROW_CHUNK + 4ull * (threadIdx.x & 63); }
    __device__ long long col(unsigned long long k) const { return (long long)(g(k) - a0) - (long long)(g0 - a0); }
    __device__ unsigned long long chunk_of(unsigned long long c) const { return (g0 + c - a0) / DROW_CHUNK; }  // the chunk of column c
    __device__ bool before(unsigned long long k, unsigned long long c) const { return a0 + k * DROW_CHUNK < g0 + c; }  // chunk k starts before column c
    __device__ void load(const uint32_t *ids, unsigned long long k, uint32_t (&id)[4]) const {
        const unsigned long long x = g(k);
        if (x + 4 <= n) {
            const uint4 a = *reinterpret_cast<const uint4 *>(ids + x);
            id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w;
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = x + j < n ? ids[x + j] : 0u;
    }
};

__device__ __forceinline__ unsigned long long drow_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// inclusive prefix of v over the wave
__device__ __forceinline__ unsigned long long drow_wave_scan(unsigned long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

struct DrowSelectParams {
    const uint32_t *ids;               // n_rows * row_len, 16-B aligned
    uint32_t n_rows, row_len;
    const uint32_t *row_start, *row_end;  // nullptr: 0 / row_len
    DrowSets sets;
    uint32_t flags;
    DecTable tab;
    uint2 *win;                        // out, per row: the considered columns [x, y)
    uint32_t *kept;                    // out, per row: kept ids
    unsigned long long *rbytes;        // out, per row: bytes of the kept ids' tokens
    uint32_t *status;                  // |= DROW_E_WINDOW for a bad window, DROW_BIG_ROW for a row of DROW_MAX_CHARS bytes or more
};

__global__ __launch_bounds__(BLOCK) void k_drow_select(DrowSelectParams P) {
    __shared__ uint32_t s_set[DROW_MAX_STOP + DROW_MAX_SKIP];
    drow_stage_sets(P.sets, s_set);
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= P.n_rows) return;
    uint32_t lo = P.row_start ? P.row_start[r] : 0u, hi = P.row_end ? P.row_end[r] : P.row_len;
    if (lo > hi || hi > P.row_len) {
        if (lane == 0) atomicOr(P.status, DROW_E_WINDOW);
        lo = hi = 0;
    }
    const DrowRow R(r, P.row_len, P.n_rows);
    long long end = hi;  // the first column that is not considered
    unsigned long long kept = 0, bytes = 0;
    for (unsigned long long k = R.chunk_of(lo); R.before(k, (unsigned long long)end); ++k) {
        uint32_t id[4];
        R.load(P.ids, k, id);
        const long long c = R.col(k);
        if (P.sets.n_stop) {  // the first stop of this chunk ends the row (and the loop)
            long long first = -1;
#pragma unroll
            for (int j = 3; j >= 0; --j)
                if (c + j >= (long long)lo && c + j < end && drow_has(s_set, P.sets.n_stop, P.sets.f_stop, id[j])) first = c + j;
            const unsigned long long hit = __ballot(first >= 0);
            if (hit) end = __shfl(first, __ffsll((long long)hit) - 1) + ((P.flags & DROW_INCLUDE_STOP) ? 1 : 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j >= (long long)lo && c + j < end && !drow_has(s_set + P.sets.n_stop, P.sets.n_skip, P.sets.f_skip, id[j])) {
                ++kept;
                bytes += dec_entry(P.tab, id[j]).y;
            }
    }
    kept = drow_wave_sum(kept);
    bytes = drow_wave_sum(bytes);
    if (lane == 0) {
        P.win[r] = make_uint2(lo, (uint32_t)(end > (long long)lo ? end : (long long)lo));
        P.kept[r] = (uint32_t)kept;
        P.rbytes[r] = bytes;
        if (bytes >= DROW_MAX_CHARS) atomicOr(P.status, DROW_BIG_ROW);
    }
}

struct DrowCompactParams {
    const uint32_t *ids;
    uint32_t n_rows, row_len;
    DrowSets sets;
    const uint2 *win;                  // per row: the considered columns
    const unsigned long long *koff;    // per row: its first slot in kids
    uint32_t *kids;                    // out: the kept ids of all rows
};

__global__ __launch_bounds__(BLOCK) void k_drow_compact(DrowCompactParams P) {
    __shared__ uint32_t s_set[DROW_MAX_STOP + DROW_MAX_SKIP];
    drow_stage_sets(P.sets, s_set);
    const uint32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= P.n_rows) return;
    const uint2 w = P.win[r];
    const DrowRow R(r, P.row_len, P.n_rows);
    unsigned long long o = P.koff[r];
    for (unsigned long long k = R.chunk_of(w.x); R.before(k, w.y); ++k) {
        uint32_t id[4];
        R.load(P.ids, k, id);
        const long long c = R.col(k);
        uint32_t keep = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j >= (long long)w.x && c + j < (long long)w.y && !drow_has(s_set + P.sets.n_stop, P.sets.n_skip, P.sets.f_skip, id[j]))
                keep |= 1u << j;
        const unsigned long long inc = drow_wave_scan(__popc(keep));
        unsigned long long x = o + inc - __popc(keep);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (keep >> j & 1u) P.kids[x++] = id[j];
        o += __shfl(inc, 63);
    }
}

// What k_drow_chars leaves and k_drow_spans reads: nchars(b) of the whole gathered text, for any byte offset b into it.
struct DrowChars {
    unsigned long long *mask;   // per 64 bytes: bit i = byte i starts a character
    uint16_t *wpre;             // per 64 bytes: character starts in its tile in front of it
    unsigned long long *tpre;   // per tile: character starts in front of it ([n_tiles] = all)
};

__device__ __forceinline__ unsigned long long drow_nchars(const DrowChars &C, unsigned long long b) {
    const unsigned long long t = b / DEC_TILE;
    const uint32_t w = (uint32_t)(b % DEC_TILE);
    unsigned long long n = C.tpre[t];
    if (w) {  // (b = the end of the text on a tile edge: there is no word to read)
        const unsigned long long word = t * DROW_WORDS + (w >> 6);
        n += C.wpre[word];
        if (w & 63u) n += __popcll(C.mask[word] & ((1ull << (w & 63u)) - 1));
    }
    return n;
}

struct DrowCharsParams {
    const uint8_t *g;                   // gathered text
    unsigned long long n;               // its bytes
    const unsigned long long *rbase;    // n_rows + 1 row offsets into it, ascending, [0] = 0, [n_rows] = n
    uint32_t n_rows;
    DrowChars out;
    uint32_t *tcount;                   // out, per tile: character starts
};

__global__ __launch_bounds__(BLOCK) void k_drow_chars(DrowCharsParams P) {
    constexpr int SPAN = DEC_TILE + 2 * DEC_HALO;
    __shared__ __attribute__((aligned(16))) uint8_t s_t[SPAN];
    __shared__ uint32_t s_b[(SPAN + 31) / 32];  // bit q: a row starts (or the text ends) at byte org + q
    __shared__ unsigned long long s_w[WPB];
    __shared__ uint32_t s_d0;
    const unsigned long long T0 = (unsigned long long)blockIdx.x * DEC_TILE, p0 = T0 + (unsigned long long)threadIdx.x * DEC_TPT;
    const long long org = (long long)T0 - DEC_HALO;
    for (int i = threadIdx.x; i < (SPAN + 31) / 32; i += BLOCK) s_b[i] = 0;
    if (threadIdx.x == 0) {  // the first row offset at or after the span's first byte
        uint32_t lo = 0, hi = P.n_rows + 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((long long)P.rbase[mid] >= org) hi = mid; else lo = mid + 1;
        }
        s_d0 = lo;
    }
    __syncthreads();
    for (unsigned long long d = (unsigned long long)s_d0 + threadIdx.x; d <= P.n_rows; d += BLOCK) {
        const long long q = (long long)P.rbase[d] - org;
        if (q >= SPAN) break;
        atomicOr(&s_b[q >> 5], 1u << (q & 31));
    }
    const uint4 w = dec_load_tile(P.g, P.n, T0, s_t);  // (ends with a barrier: the bits are set, too)
    uint32_t bits = 0;
    if (p0 < P.n) {
        const unsigned long long p1 = p0 + DEC_TPT < P.n ? p0 + DEC_TPT : P.n;
        if (p1 - p0 == DEC_TPT && !((w.x | w.y | w.z | w.w) & 0x80808080u)) {
            bits = 0xFFFFu;  // ASCII: every byte is a character
        } else {
            const DecView v{s_t, (uint64_t)org};
            auto edge = [&](unsigned long long x) { const long long q = (long long)x - org; return (s_b[q >> 5] >> (q & 31)) & 1u; };
            for (unsigned long long p = p0; p < p1; ++p) {
                bool st = !dec_cont(v.T(p));
                if (!st) {  // the row's bounds as far as dec_out_len looks: 3 bytes either way
                    unsigned long long ds = p >= 3 ? p - 3 : 0, de = p + 4 < P.n ? p + 4 : P.n;
                    for (int k = 0; k <= 3 && (unsigned long long)k <= p; ++k)
                        if (edge(p - k)) { ds = p - k; break; }
                    for (int k = 1; k <= 3 && p + k <= P.n; ++k)
                        if (edge(p + k)) { de = p + k; break; }
                    st = dec_char_start(v, p, ds, de);
                }
                bits |= (st ? 1u : 0u) << (p - p0);
            }
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long m = (unsigned long long)bits << (16 * (lane & 3));
    m |= __shfl_xor(m, 1);
    m |= __shfl_xor(m, 2);
    unsigned long long total;
    const unsigned long long pre = dec_block_scan(__popc(bits), s_w, &total);
    if ((lane & 3) == 0) {
        const unsigned long long word = (unsigned long long)blockIdx.x * DROW_WORDS + (threadIdx.x >> 2);
        P.out.mask[word] = m;
        P.out.wpre[word] = (uint16_t)pre;
    }
    if (threadIdx.x == 0) P.tcount[blockIdx.x] = (uint32_t)total;
}

struct DrowSpansParams {
    const uint32_t *ids;
    uint32_t n_rows, row_len;
    DrowSets sets;
    DecTable tab;
    const uint2 *win;                   // per row: the considered columns
    const unsigned long long *rbase;    // n_rows + 1 row offsets into the gathered text
    DrowChars chars;
    uint2 *spans;                       // out: (start, end) in characters of the row's text for every column; nullptr: not wanted
    uint32_t *status;                   // |= DROW_E_CHARS for a row of DROW_MAX_CHARS characters or more
};

__global__ __launch_bounds__(BLOCK) void k_drow_spans(DrowSpansParams P) {
    __shared__ uint32_t s_set[DROW_MAX_STOP + DROW_MAX_SKIP];
    drow_stage_sets(P.sets, s_set);
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= P.n_rows) return;
    const unsigned long long base = P.rbase[r], n0 = drow_nchars(P.chars, base);
    if (drow_nchars(P.chars, P.rbase[r + 1]) - n0 >= DROW_MAX_CHARS) {
        if (lane == 0) atomicOr(P.status, DROW_E_CHARS);
        return;
    }
    if (!P.spans) return;
    const uint2 w = P.win[r];
    const DrowRow R(r, P.row_len, P.n_rows);
    unsigned long long carry = 0;  // kept bytes of the row in front of this chunk
    for (unsigned long long k = 0; R.before(k, P.row_len); ++k) {
        const long long c = R.col(k);
        uint32_t len[4] = {0u, 0u, 0u, 0u};
        unsigned long long pre = 0, total = 0;  // kept bytes of this chunk in front of the lane's columns, and in all of it
        if (R.before(k, w.y) && !R.before(k + 1, (unsigned long long)w.x + 1)) {  // the chunk holds considered columns
            uint32_t id[4];
            R.load(P.ids, k, id);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j >= (long long)w.x && c + j < (long long)w.y && !drow_has(s_set + P.sets.n_stop, P.sets.n_skip, P.sets.f_skip, id[j]))
                    len[j] = dec_entry(P.tab, id[j]).y;
            const unsigned long long mine = (unsigned long long)len[0] + len[1] + len[2] + len[3], inc = drow_wave_scan(mine);
            pre = inc - mine;
            total = __shfl(inc, 63);
        }
        unsigned long long p = base + carry + pre;
        carry += total;
        uint32_t s = (uint32_t)(drow_nchars(P.chars, p) - n0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p += len[j];
            const uint32_t e = len[j] ? (uint32_t)(drow_nchars(P.chars, p) - n0) : s;
            if (c + j >= 0 && c + j < (long long)P.row_len) P.spans[R.g0 + (unsigned long long)(c + j)] = make_uint2(s, e);
            s = e;
        }
    }
}

} // namespace yb
