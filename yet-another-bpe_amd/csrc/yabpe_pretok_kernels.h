// yabpe_pretok_kernels.h -- the pre-tokeniser on the device (reference trainer.py:136-214).
//
// Input: the UTF-8 bytes of the corpus, resident in HBM, cut into chunks (every chunk is a text of its own).
// Output: u64 word offsets INTO THAT BUFFER (no copy of the text): word i = text[off[i], off[i+1]).  Pre-tokens partition
// each chunk, so one flag per byte ("a pre-token starts here") describes the result; the flags are compacted into the
// offsets array by a two-level prefix sum.  All rules live in pretok_logic.h (shared with the CPU model the tests run
// against regex.findall); the kernels only map bytes to threads.
//
// Passes over the text:
//               k_pt_fused     text -> meta (class, continuation, UTF-8 validation: first malformed byte by atomicMin)
//                                      and flags, through an LDS window per workgroup
//               k_pt_special   text, meta -> corrected flags (only when special tokens are configured)
//               k_grp_windows / k_grp_carry / k_grp_apply   meta, flags -> flags with digit runs cut into groups (only with
//                                      the option "digit_group" >= 1; group_logic.h)
//               k_pt_count / k_pt_scatter   flags -> offsets
// With the option "split_pattern" = 1 (the cl100k pattern, split4_logic.h) the first two are k_pt4_fused / k_pt4_special,
// and k_nl_windows / k_nl_carry / k_nl_apply (the newline rules: two segmented scans) run in front of the digit groups.
// With "split_pattern" = 3 (the o200k_base pattern, split5_logic.h) pt_split5 takes the place of all of them: classes, a
// backward scan of two look-ahead bits, a forward scan of state-transition functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "group_logic.h"
#include "pretok_logic.h"
#include "split4_logic.h"
#include "split5_logic.h"
#include "yabpe_aux_kernels.h"
#include "yabpe_scan_kernels.h"

namespace yb {

constexpr int PT_PER_BLOCK = BLOCK * 8; // bytes per workgroup in the count / scatter passes

struct PretokParams {
    const uint8_t *text;
    uint8_t *meta;
    uint8_t *flags;
    unsigned long long n;
    const uint8_t *cls;       // class per code point (0x110000 entries)
    unsigned long long *err;  // smallest malformed byte position (atomicMin), ~0 = none
    PtSpecials sp;
    uint8_t inside;           // what k_pt_special writes on the bytes of a taken special after its first: 0, or GRP_INSIDE
                              // when the grouping pass follows (it has to tell them from the digits of a digit run)
};

__global__ __launch_bounds__(BLOCK) void k_pt_mark_chunks(uint8_t *meta, const unsigned long long *chunk_off, uint32_t n_chunks,
                                                          unsigned long long n) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < n_chunks && chunk_off[c] < n) meta[chunk_off[c]] = PT_CHUNK0; // (meta was zeroed)
}

// classify + starts in one pass: a workgroup stages a window of the text (and the chunk marks) in LDS with a halo on both
// sides, classifies every byte of window + halo there (neighbouring workgroups redo each other's halo: 16 bytes of 4 KiB),
// then decides the start flag of every byte of the window from LDS.  The text is read from HBM once, meta and flags are
// written once, 16 B per lane.  The rules are the same functions the CPU model runs, on an LDS view (PtView::org).
constexpr int PT_WIN = BLOCK * 16; // bytes per workgroup and iteration
constexpr int PT_HALO = 16;        // >= reach of the rules: 7 bytes back (contraction + previous character; cl100k: 11), 4 ahead
constexpr int PT_LDS = PT_HALO + PT_WIN + PT_HALO;
// PAT 0: the GPT-2 rules; PAT 1: the cl100k rules (split4_logic.h; they look 11 bytes back, meta gets PT4_NL, a flag can
// be PT4_PENDING).
template <int PAT>
__device__ __forceinline__ void pt_fused_body(const PretokParams &P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[PT_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_meta[PT_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_tmp[PT_LDS]; // classes, then flags
    const unsigned long long n_win = (P.n + PT_WIN - 1) / PT_WIN;
    const bool wide = (reinterpret_cast<uintptr_t>(P.text) & 15u) == 0; // 16-B loads need an aligned text buffer
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long base = w * PT_WIN;      // first byte of the window
        const long long org = (long long)base - PT_HALO; // position of s_text[0] (negative for window 0)
        // ---- stage: the window as 16-B pieces, the halos byte by byte
        {
            const unsigned long long g = base + (unsigned long long)threadIdx.x * 16;
            uint8_t *dt = s_text + PT_HALO + threadIdx.x * 16, *dm = s_meta + PT_HALO + threadIdx.x * 16;
            if (g + 16 <= P.n) {
                if (wide) {
                    *reinterpret_cast<uint4 *>(dt) = *reinterpret_cast<const uint4 *>(P.text + g);
                } else {
                    for (int k = 0; k < 16; ++k) dt[k] = P.text[g + k];
                }
                *reinterpret_cast<uint4 *>(dm) = *reinterpret_cast<const uint4 *>(P.meta + g);
            } else {
                for (int k = 0; k < 16; ++k) {
                    dt[k] = g + k < P.n ? P.text[g + k] : 0;
                    dm[k] = g + k < P.n ? P.meta[g + k] : 0;
                }
            }
            if (threadIdx.x < 2 * PT_HALO) {
                const int k = threadIdx.x < PT_HALO ? threadIdx.x : PT_WIN + threadIdx.x; // slot in s_text
                const long long pos = org + k;
                const bool in = pos >= 0 && (unsigned long long)pos < P.n;
                s_text[k] = in ? P.text[pos] : 0;
                s_meta[k] = in ? P.meta[pos] : 0;
            }
        }
        __syncthreads();
        // A view whose position `org` is s_text[0].  For window 0 the halo before the text does not exist: the view then
        // starts at position 0 (s_text + PT_HALO) -- no rule looks before a chunk start, and position 0 is one.
        const bool first = org < 0;
        const unsigned long long vorg = first ? 0ull : (unsigned long long)org;
        const PtView v{first ? s_text + PT_HALO : s_text, first ? s_meta + PT_HALO : s_meta, P.n, vorg};
        uint8_t *tmp = first ? s_tmp + PT_HALO : s_tmp;   // tmp[pos - vorg]
        uint8_t *meta_w = first ? s_meta + PT_HALO : s_meta;
        // ---- classify the window + 8 bytes on each side (cl100k: 12 in front): what the start rules can look at
        const long long c_lo = (long long)base - (PAT ? 12 : 8), c_hi = (long long)base + PT_WIN + 8; // [c_lo, c_hi)
        {
            unsigned long long bad_pos = ~0ull;
            for (long long pos = c_lo + threadIdx.x; pos < c_hi; pos += BLOCK) { // (consecutive lanes, consecutive bytes)
                if (pos < 0 || (unsigned long long)pos >= P.n) continue;
                const unsigned long long i = (unsigned long long)pos;
                unsigned long long end = P.n;
                for (unsigned long long q = i + 1; q < i + 4 && q < P.n; ++q)
                    if (v.M(q) & PT_CHUNK0) {
                        end = q;
                        break;
                    }
                bool bad = false;
                tmp[i - vorg] = pt_classify(v, i, end, P.cls, &bad);
                if (bad && i >= base && i < base + PT_WIN && i < bad_pos) bad_pos = i; // (a halo byte is reported by its own window)
            }
            if (bad_pos != ~0ull) atomicMin(P.err, bad_pos);
        }
        __syncthreads(); // every chunk mark has been read; now the class bits are added
        for (long long pos = c_lo + threadIdx.x; pos < c_hi; pos += BLOCK) {
            if (pos < 0 || (unsigned long long)pos >= P.n) continue;
            const unsigned long long k = (unsigned long long)pos - vorg;
            meta_w[k] = (uint8_t)((meta_w[k] & PT_CHUNK0) | tmp[k]);
            if (PAT && pt4_is_nl(v.T((unsigned long long)pos))) meta_w[k] |= PT4_NL;
        }
        __syncthreads();
        // ---- start flags of the window (tmp is free again), then meta and flags go out as 16-B pieces
        for (int k = threadIdx.x; k < PT_WIN; k += BLOCK) {
            const unsigned long long j = base + k;
            if (PAT) tmp[j - vorg] = j < P.n ? pt4_is_start(v, j, -1) : 0;
            else tmp[j - vorg] = j < P.n ? (pt_is_start(v, j, -1) ? 1 : 0) : 0;
        }
        __syncthreads();
        {
            const unsigned long long g = base + (unsigned long long)threadIdx.x * 16;
            const uint8_t *fm = s_meta + PT_HALO + threadIdx.x * 16, *ff = s_tmp + PT_HALO + threadIdx.x * 16;
            if (g + 16 <= P.n) {
                *reinterpret_cast<uint4 *>(P.flags + g) = *reinterpret_cast<const uint4 *>(ff);
                *reinterpret_cast<uint4 *>(P.meta + g) = *reinterpret_cast<const uint4 *>(fm);
            } else {
                for (int k = 0; k < 16 && g + k < P.n; ++k) {
                    P.flags[g + k] = ff[k];
                    P.meta[g + k] = fm[k];
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BLOCK) void k_pt_fused(PretokParams P) { pt_fused_body<0>(P); }
__global__ __launch_bounds__(BLOCK) void k_pt4_fused(PretokParams P) { pt_fused_body<1>(P); }

// Special tokens: one pass.  A 256-bit set of the specials' first bytes keeps nearly every thread out of the compare;
// a thread that finds an occurrence checks whether it heads its chain (occurrences before it are looked up on demand,
// through the same filter) and, if so, resolves the whole chain (pretok_logic.h).
template <int PAT>
__device__ __forceinline__ void pt_special_body(const PretokParams &P) {
    __shared__ uint32_t s_first[8];
    if (threadIdx.x < 8) s_first[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x < P.sp.n) {
        const uint32_t o = P.sp.off[threadIdx.x];
        if (P.sp.off[threadIdx.x + 1] > o) atomicOr(&s_first[P.sp.bytes[o] >> 5], 1u << (P.sp.bytes[o] & 31));
    }
    __syncthreads();
    const PtView v{P.text, P.meta, P.n, 0};
    const PtSpecials sp = P.sp;
    const uint32_t *first = s_first;
    auto occ = [&](unsigned long long q) -> uint32_t {
        const uint8_t b = v.T(q);
        return ((first[b >> 5] >> (b & 31)) & 1u) ? pt_special_at(v, sp, q) : 0u;
    };
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < P.n; i += (unsigned long long)gridDim.x * BLOCK) {
        const uint32_t o = occ(i);
        if (PAT) {
            if (o && pt4_special_is_head(v, sp, occ, i)) pt4_special_walk(v, sp, occ, P.flags, i, o);
        } else {
            if (o && pt_special_is_head(v, sp, occ, i)) pt_special_walk(v, sp, occ, P.flags, i, o, P.inside);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_pt_special(PretokParams P) { pt_special_body<0>(P); }
__global__ __launch_bounds__(BLOCK) void k_pt4_special(PretokParams P) { pt_special_body<1>(P); }

// ---------------------------------------------------------------- digit groups (rules and states: group_logic.h)
// Whether a pre-token starts at a digit depends on how many digits of its run stand in front of it, however many that
// is: a segmented scan over the text, forward, in the three launches of yabpe_scan_kernels.h.
//   k_grp_windows   per window: the combined state of its bytes (does it hold a start; digits counted after the last one)
//   k_grp_carry     the state in front of every window
//   k_grp_apply     per piece the state in front of it, then every thread walks its piece and writes its 16 final flags
// Every read of the flags as k_pt_fused / k_pt_special / k_enc_clear left them happens in the first two kernels or, in
// k_grp_apply, by the one thread that afterwards writes those same 16 bytes: a start this pass adds is never taken for
// one it should count from.
static_assert(PT_WIN == SCAN_WIN && PT_WIN == GRP_WIN && GRP_PIECE == SCAN_PIECE, "one piece per thread, one window per workgroup");

struct GrpPiece {
    uint32_t m[4], f[4]; // 16 meta bytes, 16 flag bytes
    __device__ __forceinline__ void get(int k, uint8_t *meta, uint8_t *flag) const {
        *meta = (uint8_t)(m[k >> 2] >> ((k & 3) * 8));
        *flag = (uint8_t)(f[k >> 2] >> ((k & 3) * 8));
    }
};

// The piece at byte g (a multiple of 16); bytes past the text read as meta PT_O, flag 0.  (scan_load for two arrays under one
// tail guard.  Two calls of scan_load, or one loader for N arrays, cost k_nl_apply 3 VGPRs and the tail twice the branches.)
__device__ __forceinline__ GrpPiece grp_load(const uint8_t *meta, const uint8_t *flags, unsigned long long g, unsigned long long n) {
    GrpPiece p;
    if (g + GRP_PIECE <= n) {
        const uint4 a = *reinterpret_cast<const uint4 *>(meta + g), b = *reinterpret_cast<const uint4 *>(flags + g);
        p.m[0] = a.x; p.m[1] = a.y; p.m[2] = a.z; p.m[3] = a.w;
        p.f[0] = b.x; p.f[1] = b.y; p.f[2] = b.z; p.f[3] = b.w;
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            p.m[w] = PT_O * 0x01010101u;
            p.f[w] = 0u;
        }
#pragma unroll
        for (int k = 0; k < GRP_PIECE; ++k)
            if (g + k < n) {
                const int sh = (k & 3) * 8;
                p.m[k >> 2] = (p.m[k >> 2] & ~(0xFFu << sh)) | ((uint32_t)meta[g + k] << sh);
                p.f[k >> 2] |= (uint32_t)flags[g + k] << sh;
            }
    }
    return p;
}

struct GrpOp {
    typedef GrpState State;
    uint32_t G;
    __device__ __forceinline__ State identity() const { return 0; }
    __device__ __forceinline__ State combine(State a, State b) const { return grp_combine(a, b, G); }
};

struct GrpPass { // (no finish: k_grp_apply has a loop of its own)
    const uint8_t *meta, *flags;
    unsigned long long n;
    uint32_t G;
    __device__ __forceinline__ GrpPiece load(unsigned long long g) const { return grp_load(meta, flags, g, n); }
    __device__ __forceinline__ GrpState state(const GrpPiece &p, unsigned long long) const {
        return grp_piece_state([&](int k, uint8_t *m, uint8_t *f) { p.get(k, m, f); }, G);
    }
};

__global__ __launch_bounds__(BLOCK) void k_grp_windows(const uint8_t *meta, const uint8_t *flags, unsigned long long n, uint32_t G,
                                                       GrpState *win) {
    scan_windows_body<SCAN_FWD>(GrpOp{G}, GrpPass{meta, flags, n, G}, n, win);
}
__global__ __launch_bounds__(BLOCK) void k_grp_carry(GrpState *win, unsigned long long n_win, uint32_t G) {
    scan_carry_body<SCAN_FWD, SCAN_WHOLE>(GrpOp{G}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_grp_apply(const uint8_t *meta, uint8_t *flags, unsigned long long n, uint32_t G,
                                                     const GrpState *win) {
    __shared__ GrpState s_w[WPB];
    const GrpOp op{G};
    const unsigned long long n_win = (n + PT_WIN - 1) / PT_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * PT_WIN + (unsigned long long)threadIdx.x * GRP_PIECE;
        const GrpPiece p = grp_load(meta, flags, g, n);
        auto get = [&](int k, uint8_t *m, uint8_t *f) { p.get(k, m, f); };
        GrpState total;
        const GrpState before = op.combine(win[w], scan_block<SCAN_FWD>(op, grp_piece_state(get, G), s_w, &total));
        uint32_t o[4] = {0u, 0u, 0u, 0u};
        grp_piece_flags(before, get, [&](int k, uint8_t f) { o[k >> 2] |= (uint32_t)f << ((k & 3) * 8); }, G);
        if (g + GRP_PIECE <= n) { // (scan_store, written out: the call costs this kernel 2 VGPRs, 36 for 34)
            *reinterpret_cast<uint4 *>(flags + g) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < GRP_PIECE; ++k)
                if (g + k < n) flags[g + k] = (uint8_t)(o[k >> 2] >> ((k & 3) * 8));
        }
        __syncthreads();
    }
}

// The three steps on meta / flags of n > 0 bytes, left in flight on s.  G in [1, GRP_MAX].  The window states belong to S.
inline int pt_group(hipStream_t s, Scratch &S, const uint8_t *meta, uint8_t *flags, unsigned long long n, uint32_t G) {
    GrpState *win = nullptr;
    YB_RET(scan_launch(
        S, n, &win, [&](dim3 grid, GrpState *w) { hipLaunchKernelGGL(k_grp_windows, grid, dim3(BLOCK), 0, s, meta, (const uint8_t *)flags, n, G, w); },
        [&](GrpState *w, unsigned long long n_win) { hipLaunchKernelGGL(k_grp_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win, G); },
        [&](dim3 grid, const GrpState *w) { hipLaunchKernelGGL(k_grp_apply, grid, dim3(BLOCK), 0, s, meta, flags, n, G, w); }));
    return 0;
}

// ---------------------------------------------------------------- newline rules of the cl100k pattern (split4_logic.h)
// Whether a whitespace character behind a newline starts a pre-token (PT4_PENDING) depends on the whole whitespace run around
// it, however long: two segmented scans, one in each direction, packed in one word and one set of launches.
//   k_nl_windows   per window: one word with both summaries (what the window does to B behind it, to F in front of it)
//   k_nl_carry     the forward summaries scanned left to right, then the backward ones right to left -> per window the value
//                  of everything in front of it (bits 0-1) and of everything behind it (bits 2-3)
//   k_nl_apply     per piece both values, then every thread resolves its 16 flags
struct NlOp {
    typedef NlState State;
    __device__ __forceinline__ State identity() const { return NL_KEEP; }
    __device__ __forceinline__ State combine(State a, State b) const { return nl_comb(a, b); }
    __device__ __forceinline__ State lo(State x) const { return x & NL_MASK; }
    __device__ __forceinline__ State hi(State x) const { return x >> NL_BWD; } // (a state has four bits)
    __device__ __forceinline__ State pack(State l, State h) const { return l | (h << NL_BWD); }
};

// The windows and the apply kernel keep a scan and loops of their own: both directions share every shuffle step and the one
// barrier.  Built from the halves of scan_block, k_nl_apply comes out 2 VGPRs above this form (49 for 47), so only the carry
// kernel, which scans one direction at a time, goes through the bodies of yabpe_scan_kernels.h (k_nl_apply takes its scan_store).
// Exclusive scans of one state per thread over the workgroup: bits 0-1 over the threads in front (thread order), bits 2-3
// over the threads behind (nearest last).  *total: all of them, in both senses.  s_w: 2 * WPB words.
__device__ __forceinline__ NlState nl_block_scan(NlState mine, uint32_t *s_w, NlState *total) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    uint32_t f = mine & NL_MASK, b = mine >> NL_BWD;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t uf = __shfl_up(f, o), ub = __shfl_down(b, o);
        if (lane >= o) f = nl_comb(uf, f);
        if (lane + o < 64) b = nl_comb(ub, b);
    }
    const uint32_t pf = __shfl_up(f, 1), pb = __shfl_down(b, 1);
    if (lane == 63) s_w[wib] = f;
    if (lane == 0) s_w[WPB + wib] = b;
    __syncthreads();
    uint32_t bf = NL_KEEP, af = NL_KEEP, bb = NL_KEEP, ab = NL_KEEP;
#pragma unroll
    for (int w = 0; w < WPB; ++w) {
        if (w == wib) bf = af;
        af = nl_comb(af, s_w[w]);
    }
#pragma unroll
    for (int w = WPB - 1; w >= 0; --w) {
        if (w == wib) bb = ab;
        ab = nl_comb(ab, s_w[WPB + w]);
    }
    *total = af | (ab << NL_BWD);
    const uint32_t ef = lane ? nl_comb(bf, pf) : bf, eb = lane < 63 ? nl_comb(bb, pb) : bb;
    return ef | (eb << NL_BWD);
}

__global__ __launch_bounds__(BLOCK) void k_nl_windows(const uint8_t *meta, const uint8_t *flags, unsigned long long n, NlState *win) {
    __shared__ uint32_t s_w[2 * WPB];
    const unsigned long long n_win = (n + PT_WIN - 1) / PT_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const GrpPiece p = grp_load(meta, flags, w * PT_WIN + (unsigned long long)threadIdx.x * GRP_PIECE, n);
        NlState total;
        (void)nl_block_scan(nl_piece_state(nl_piece(p.m, p.f)), s_w, &total);
        if (threadIdx.x == 0) win[w] = total;
        __syncthreads();
    }
}
__global__ __launch_bounds__(BLOCK) void k_nl_carry(NlState *win, unsigned long long n_win) {
    scan_carry_body<SCAN_FWD, SCAN_LO>(NlOp{}, win, n_win);
    scan_carry_body<SCAN_BWD, SCAN_HI>(NlOp{}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_nl_apply(const uint8_t *meta, uint8_t *flags, unsigned long long n, const NlState *win) {
    __shared__ uint32_t s_w[2 * WPB];
    const unsigned long long n_win = (n + PT_WIN - 1) / PT_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * PT_WIN + (unsigned long long)threadIdx.x * GRP_PIECE;
        const GrpPiece p = grp_load(meta, flags, g, n);
        const NlPiece q = nl_piece(p.m, p.f);
        NlState total;
        const NlState in = nl_block_scan(nl_piece_state(q), s_w, &total), edge = win[w];
        const uint32_t before = nl_comb(edge & NL_MASK, in & NL_MASK), after = nl_comb(edge >> NL_BWD, in >> NL_BWD);
        uint32_t o[4] = {p.f[0], p.f[1], p.f[2], p.f[3]};
        nl_piece_flags(before, after, q, o);
        scan_store(flags, g, n, o);
        __syncthreads();
    }
}

// The three steps on meta / flags of n > 0 bytes, left in flight on s.  The window states belong to S.
inline int pt_newlines(hipStream_t s, Scratch &S, const uint8_t *meta, uint8_t *flags, unsigned long long n) {
    NlState *win = nullptr;
    YB_RET(scan_launch(
        S, n, &win, [&](dim3 grid, NlState *w) { hipLaunchKernelGGL(k_nl_windows, grid, dim3(BLOCK), 0, s, meta, (const uint8_t *)flags, n, w); },
        [&](NlState *w, unsigned long long n_win) { hipLaunchKernelGGL(k_nl_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
        [&](dim3 grid, const NlState *w) { hipLaunchKernelGGL(k_nl_apply, grid, dim3(BLOCK), 0, s, meta, flags, n, w); }));
    return 0;
}

// ---------------------------------------------------------------- the o200k_base pattern (split5_logic.h; "split_pattern" = 3)
// No rule of this pattern has bounded reach, so nothing is decided locally: the text becomes classes, the classes become two
// look-ahead bits by one backward scan, and the characters -- functions over the scanner's 13 states -- are scanned forward.
//   k_s5_class     text, chunk marks -> meta (class, sub-class, continuation, chunk mark; UTF-8 validation as k_pt_fused does it).
//                  The marks are read from an array of their own, so no thread reads a byte another one writes.
//   k_la_windows / k_la_carry / k_la_apply   meta -> meta with PT5_LA: F and UE, scanned right to left
//   k_s5_aux       text, meta -> flags = the aux byte (class of the next character, contraction length)
//   k_s5_special   text, meta -> A5_HEAD / A5_LAST on every occurrence of a special (training pattern only)
//   k_fn_windows / k_fn_carry / k_fn_apply   meta, aux -> flags: per window the composed function; the functions in front of
//                  every window; per piece the state in front of it, then its 16 flags (0, 1, GRP_INSIDE)

__global__ __launch_bounds__(BLOCK) void k_s5_class(const uint8_t *text, const uint8_t *marks, uint8_t *meta, unsigned long long n,
                                                    const uint8_t *cls5, unsigned long long *err) {
    const PtView v{text, marks, n, 0};
    unsigned long long bad_pos = ~0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) {
        unsigned long long end = n;
        for (unsigned long long q = i + 1; q < i + 4 && q < n; ++q)
            if (marks[q] & PT_CHUNK0) {
                end = q;
                break;
            }
        bool bad = false;
        meta[i] = (uint8_t)((marks[i] & PT_CHUNK0) | pt_classify(v, i, end, cls5, &bad));
        if (bad && i < bad_pos) bad_pos = i;
    }
    if (bad_pos != ~0ull) atomicMin(err, bad_pos);
}

struct LaOp {
    typedef uint32_t State;
    __device__ __forceinline__ State identity() const { return LA_KEEP; }
    __device__ __forceinline__ State combine(State a, State b) const { return la_comb(a, b); }
};

struct LaPass {
    const uint8_t *meta;
    uint8_t *out; // the meta bytes again (k_la_apply)
    unsigned long long n;
    __device__ __forceinline__ ScanPiece load(unsigned long long g) const { return scan_load(meta, g, n, PT_O); }
    __device__ __forceinline__ uint32_t state(const ScanPiece &m, unsigned long long) const { return la_piece_state(m.w); }
    __device__ __forceinline__ void finish(uint32_t after, ScanPiece &m, unsigned long long g) const {
        la_piece_bits(after, m.w);
        scan_store(out, g, n, m.w);
    }
};

__global__ __launch_bounds__(BLOCK) void k_la_windows(const uint8_t *meta, unsigned long long n, uint32_t *win) {
    scan_windows_body<SCAN_BWD>(LaOp{}, LaPass{meta, nullptr, n}, n, win);
}
__global__ __launch_bounds__(BLOCK) void k_la_carry(uint32_t *win, unsigned long long n_win) {
    scan_carry_body<SCAN_BWD, SCAN_WHOLE>(LaOp{}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_la_apply(uint8_t *meta, unsigned long long n, const uint32_t *win) {
    scan_apply_body<SCAN_BWD>(LaOp{}, LaPass{meta, meta, n}, n, win);
}

// the aux byte of every byte: the rules look at most 4 bytes ahead (the next character; two suffix letters)
__global__ __launch_bounds__(BLOCK) void k_s5_aux(const uint8_t *text, const uint8_t *meta, uint8_t *aux, unsigned long long n) {
    const PtView v{text, meta, n, 0};
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK)
        aux[i] = s5_aux(v, i);
}

// every occurrence of a special gets A5_HEAD on its first and A5_LAST on its last byte (occurrences never overlap: the caller
// has refused the sets in which they could, so every byte is written by one thread at most)
__global__ __launch_bounds__(BLOCK) void k_s5_special(PretokParams P) {
    __shared__ uint32_t s_first[8];
    if (threadIdx.x < 8) s_first[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x < P.sp.n) {
        const uint32_t o = P.sp.off[threadIdx.x];
        if (P.sp.off[threadIdx.x + 1] > o) atomicOr(&s_first[P.sp.bytes[o] >> 5], 1u << (P.sp.bytes[o] & 31));
    }
    __syncthreads();
    const PtView v{P.text, P.meta, P.n, 0};
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < P.n; i += (unsigned long long)gridDim.x * BLOCK) {
        const uint8_t b = v.T(i);
        if (!((s_first[b >> 5] >> (b & 31)) & 1u)) continue;
        const uint32_t o = pt_special_at(v, P.sp, i);
        if (!o) continue;
        const uint32_t len = pt_special_len(P.sp, o);
        if (len == 1) {
            P.flags[i] |= A5_HEAD | A5_LAST;
        } else {
            P.flags[i] |= A5_HEAD;
            P.flags[i + len - 1] |= A5_LAST;
        }
    }
}

struct FnOp {
    typedef S5Fn State;
    __device__ __forceinline__ State identity() const { return S5_IDENTITY; }
    __device__ __forceinline__ State combine(State a, State b) const { return s5_then(a, b); }
};

struct FnPass {
    const uint8_t *meta, *aux;
    uint8_t *out; // the aux bytes become the flags (k_fn_apply)
    unsigned long long n;
    __device__ __forceinline__ GrpPiece load(unsigned long long g) const { return grp_load(meta, aux, g, n); }
    __device__ __forceinline__ S5Fn state(const GrpPiece &p, unsigned long long) const { return s5_piece_fn(p.m, p.f); }
    __device__ __forceinline__ void finish(S5Fn before, GrpPiece &p, unsigned long long g) const {
        s5_piece_flags(s5_apply(before, S5_S0), p.m, p.f); // (whatever stands in front of the text: its first byte is a constant)
        scan_store(out, g, n, p.f);
    }
};

__global__ __launch_bounds__(BLOCK) void k_fn_windows(const uint8_t *meta, const uint8_t *aux, unsigned long long n, S5Fn *win) {
    scan_windows_body<SCAN_FWD>(FnOp{}, FnPass{meta, aux, nullptr, n}, n, win);
}
__global__ __launch_bounds__(BLOCK) void k_fn_carry(S5Fn *win, unsigned long long n_win) {
    scan_carry_body<SCAN_FWD, SCAN_WHOLE>(FnOp{}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_fn_apply(const uint8_t *meta, uint8_t *flags, unsigned long long n, const S5Fn *win) {
    scan_apply_body<SCAN_FWD>(FnOp{}, FnPass{meta, flags, flags, n}, n, win);
}

// All passes of the pattern on the chunk marks `marks` (PT_CHUNK0 or 0 per byte) of n > 0 bytes: meta and flags (0, 1,
// GRP_INSIDE: what pt_group reads) are written, *err as by k_pt_fused; left in flight on s.  sp.n = 0: no special is looked for
// (encode: the pieces are texts of their own).  The window values belong to S.
inline int pt_split5(hipStream_t s, Scratch &S, const uint8_t *text, const uint8_t *marks, uint8_t *meta, uint8_t *flags, unsigned long long n,
                     const uint8_t *cls5, unsigned long long *err, const PtSpecials &sp) {
    uint32_t *la = nullptr;
    S5Fn *fn = nullptr;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>((n + BLOCK - 1) / BLOCK, 1u << 20);
    hipLaunchKernelGGL(k_s5_class, dim3(grid), dim3(BLOCK), 0, s, text, marks, meta, n, cls5, err);
    YB_RET(scan_launch(
            S, n, &la, [&](dim3 wgrid, uint32_t *w) { hipLaunchKernelGGL(k_la_windows, wgrid, dim3(BLOCK), 0, s, (const uint8_t *)meta, n, w); },
            [&](uint32_t *w, unsigned long long n_win) { hipLaunchKernelGGL(k_la_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
            [&](dim3 wgrid, const uint32_t *w) { hipLaunchKernelGGL(k_la_apply, wgrid, dim3(BLOCK), 0, s, meta, n, w); }));
    hipLaunchKernelGGL(k_s5_aux, dim3(grid), dim3(BLOCK), 0, s, text, (const uint8_t *)meta, flags, n);
    if (sp.n) {
        const PretokParams P{text, meta, flags, n, cls5, err, sp, 0};
        hipLaunchKernelGGL(k_s5_special, dim3(grid), dim3(BLOCK), 0, s, P);
    }
    YB_RET(scan_launch(
        S, n, &fn, [&](dim3 wgrid, S5Fn *w) { hipLaunchKernelGGL(k_fn_windows, wgrid, dim3(BLOCK), 0, s, (const uint8_t *)meta, (const uint8_t *)flags, n, w); },
        [&](S5Fn *w, unsigned long long n_win) { hipLaunchKernelGGL(k_fn_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
        [&](dim3 wgrid, const S5Fn *w) { hipLaunchKernelGGL(k_fn_apply, wgrid, dim3(BLOCK), 0, s, (const uint8_t *)meta, flags, n, w); }));
    return 0;
}

// flags -> offsets, pass 1: number of starts per workgroup of PT_PER_BLOCK bytes
__global__ __launch_bounds__(BLOCK) void k_pt_count(const uint8_t *flags, unsigned long long n, unsigned long long *block_sums) {
    __shared__ uint32_t s_w[WPB];
    const unsigned long long base = (unsigned long long)blockIdx.x * PT_PER_BLOCK + (unsigned long long)threadIdx.x * 8;
    uint32_t cnt = 0;
    if (base + 8 <= n) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long *>(flags + base); // eight 0/1 bytes
        cnt = (uint32_t)__popcll(w);
    } else {
        for (unsigned long long k = base; k < n; ++k) cnt += flags[k];
    }
    cnt = (uint32_t)wave_sum_u64(cnt);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < WPB; ++w) t += s_w[w];
        block_sums[blockIdx.x] = t;
    }
}

// pass 2: off[block_base + rank of the start inside the workgroup] = its byte position
__global__ __launch_bounds__(BLOCK) void k_pt_scatter(const uint8_t *flags, unsigned long long n, const unsigned long long *block_base,
                                                      unsigned long long *off) {
    __shared__ uint32_t s_w[WPB];
    const unsigned long long base = (unsigned long long)blockIdx.x * PT_PER_BLOCK + (unsigned long long)threadIdx.x * 8;
    uint8_t f[8];
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        f[k] = base + k < n ? flags[base + k] : 0;
        cnt += f[k];
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_sum(cnt);
    if (lane == 63) s_w[wib] = inc;
    __syncthreads();
    uint32_t woff = 0;
    for (int w = 0; w < wib; ++w) woff += s_w[w];
    unsigned long long idx = block_base[blockIdx.x] + woff + inc - cnt;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (f[k]) off[idx++] = base + k;
}

struct PretokOut {
    unsigned long long *off; // n_words + 1
    unsigned long long n_words;
    long long bad_pos;       // first malformed UTF-8 byte, -1 if the text is valid
};

// flags -> offsets: count per workgroup, scan, the total (a synchronise), scatter, the sentinel off[n_words] = n.
// *off (n_words + 1 entries) belongs to S.  More than max_words starts: -2, with *n_words set and *off not allocated.
// The scatter and the sentinel are left in flight; n is read by the sentinel copy, so it must outlive the next synchronise.
inline int pt_offsets(hipStream_t s, Scratch &S, const uint8_t *flags, const unsigned long long &n, unsigned long long max_words,
                      unsigned long long **off, unsigned long long *n_words) {
    const unsigned long long nb = (n + PT_PER_BLOCK - 1) / PT_PER_BLOCK;
    unsigned long long *sums = nullptr, *bases = nullptr;
    YB_RET(S.get(&sums, nb));
    YB_RET(S.get(&bases, nb + 1));
    hipLaunchKernelGGL(k_pt_count, dim3((uint32_t)nb), dim3(BLOCK), 0, s, flags, n, sums);
    YB_RET(hipGetLastError());
    if (exclusive_scan<unsigned long long>(s, sums, nb, bases, nb + 1) != 0) return -1;
    YB_RET(hipMemcpyAsync(n_words, bases + nb, 8, hipMemcpyDeviceToHost, s));
    YB_RET(hipStreamSynchronize(s));
    if (*n_words > max_words) return -2;
    YB_RET(S.get(off, *n_words + 1));
    hipLaunchKernelGGL(k_pt_scatter, dim3((uint32_t)nb), dim3(BLOCK), 0, s, flags, n, bases, *off);
    YB_RET(hipMemcpyAsync(*off + *n_words, &n, 8, hipMemcpyHostToDevice, s));
    YB_RET(hipGetLastError());
    return 0;
}

// Runs all passes on `text` (device).  chunk_off: device array of n_chunks chunk starts.  cls: device class table.
// digit_group: 0, or G of group_logic.h (no special may then begin with a \p{N} character: the caller checks).
// pattern: 0 GPT-2, 1 cl100k (split4_logic.h; digit_group >= 1, and no special begins with \s either: the caller checks),
// 3 o200k_base (split5_logic.h; as 1, `cls` is then the table of pt5_table_entry and the caller has run s5_specials_check).
// Scratch (meta, flags) is allocated and released here; out->off is the caller's to free (dev_free).
inline int pretokenize(hipStream_t s, const uint8_t *text, unsigned long long n, const unsigned long long *chunk_off, uint32_t n_chunks,
                       const uint8_t *cls, const PtSpecials &sp_dev, uint32_t digit_group, uint32_t pattern, PretokOut *out) {
    *out = PretokOut{nullptr, 0, -1};
    Scratch S;
    unsigned long long *off = nullptr;
    if (n == 0) {
        YB_RET(S.get(&off, 1));
        YB_RET(hipMemsetAsync(off, 0, 8, s));
        YB_RET(hipStreamSynchronize(s));
        out->off = S.take(off);
        return 0;
    }
    uint8_t *meta = nullptr, *flags = nullptr;
    unsigned long long *err = nullptr;
    YB_RET(S.get(&meta, n));
    YB_RET(S.get(&flags, n + 8));
    YB_RET(S.get(&err, 1));
    YB_RET(hipMemsetAsync(meta, 0, n, s));
    YB_RET(hipMemsetAsync(err, 0xff, 8, s));
    const uint32_t grid = (uint32_t)std::min<unsigned long long>((n + BLOCK - 1) / BLOCK, 1u << 20);
    PretokParams P{text, meta, flags, n, cls, err, sp_dev, (uint8_t)(digit_group ? GRP_INSIDE : 0)};
    hipLaunchKernelGGL(k_pt_mark_chunks, dim3((n_chunks + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, meta, chunk_off, n_chunks, n);
    const uint32_t wgrid = (uint32_t)std::min<unsigned long long>((n + PT_WIN - 1) / PT_WIN, 1u << 20);
    if (pattern == 3) { // the marks stay where they are; the classes go to an array of their own
        uint8_t *meta5 = nullptr;
        YB_RET(S.get(&meta5, n));
        if (pt_split5(s, S, text, meta, meta5, flags, n, cls, err, sp_dev) != 0) return -1;
        meta = meta5;
    } else if (pattern) hipLaunchKernelGGL(k_pt4_fused, dim3(wgrid), dim3(BLOCK), 0, s, P);
    else hipLaunchKernelGGL(k_pt_fused, dim3(wgrid), dim3(BLOCK), 0, s, P);
    unsigned long long h_err = 0;
    YB_RET(hipMemcpyAsync(&h_err, err, 8, hipMemcpyDeviceToHost, s));
    YB_RET(hipStreamSynchronize(s));
    if (h_err != ~0ull) { // malformed UTF-8: nothing else is computed (the neighbour walks assume valid text)
        out->bad_pos = (long long)h_err;
        return 0;
    }
    if (sp_dev.n && pattern != 3) {
        if (pattern) hipLaunchKernelGGL(k_pt4_special, dim3(grid), dim3(BLOCK), 0, s, P);
        else hipLaunchKernelGGL(k_pt_special, dim3(grid), dim3(BLOCK), 0, s, P);
    }
    if (pattern == 1 && pt_newlines(s, S, meta, flags, n) != 0) return -1;
    if (digit_group && pt_group(s, S, meta, flags, n, digit_group) != 0) return -1;
    unsigned long long total = 0;
    if (pt_offsets(s, S, flags, n, ~0ull, &off, &total) != 0) return -1;
    YB_RET(hipStreamSynchronize(s));
    out->off = S.take(off);
    out->n_words = total;
    return 0;
}

} // namespace yb
