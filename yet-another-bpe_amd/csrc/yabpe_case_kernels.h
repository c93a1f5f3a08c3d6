// yabpe_case_kernels.h -- str.lower() for UTF-8 text on the device (yabpe_lowercase; the rules are in case_logic.h, shared with
// the CPU model the tests run against str.lower(); the kernels only map bytes and windows to threads).
//
// Input: UTF-8 text in HBM, cut into parts (every part is a text of its own).  Output: the text with every part lowered, and
// the part offsets into it.  A thread owns a piece of 16 bytes, a workgroup a window of 4096.  Passes:
//   check   k_case_check      text, part marks -> the first malformed byte (atomicMin); per call the code points that change,
//                             those that change length and the capital sigmas; per window the bytes it writes.  A piece of 16
//                             ASCII bytes is one load and a SWAR test for 'A'..'Z'.
//                             NOTHING CHANGES: the driver stops here.
//   same    k_case_same       no length changes, no sigma -- almost all real text: out[i] for every i, 16 bytes a store; ASCII
//                             is lowered in registers.
//   sigma   k_case_fwd_* / k_case_bwd_*   two windowed scans (yabpe_scan_kernels.h) of the three-valued state of case_logic.h:
//                             forward, a bit for every sigma with a cased code point in front of it; backward, that bit
//                             cleared where a cased one follows (the write pass counts what is left).  An ignorable code point is the identity, so no lane walks a
//                             run of them: a piece is 16 bytes whatever they hold.
//   write   k_case_write      after the exclusive scan of the window sums: every window stages its output in LDS, shifted so
//                             that the 16-byte windows of the output are 16-byte windows of the stage, and writes it with
//                             16-byte stores.  The parts that start in the window get their new offsets.  A piece of 16 ASCII
//                             bytes is one load here too: it is lowered in registers and goes to the stage in dwords.
// A text that is one part has no part marks: no pass reads or writes an array of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "case_logic.h"
#include "yabpe_aux_kernels.h"
#include "yabpe_scan_kernels.h"

namespace yb {

static_assert(CASE_WIN == SCAN_WIN && CASE_PIECE == SCAN_PIECE, "one piece per thread, one window per workgroup");

struct CaseCheckParams {
    const uint8_t *text;
    const uint8_t *marks;     // PT_CHUNK0 at every part's first byte (NULL: the text is one part)
    unsigned long long n;
    CaseTables T;
    uint32_t *wout;           // out, per window: bytes of the lowered characters whose lead byte is in it
    unsigned long long *ctr;  // [0] first malformed byte (atomicMin), [1] += changing code points, [2] += length changers, [3] += sigmas
};

__global__ __launch_bounds__(BLOCK) void k_case_check(CaseCheckParams P) {
    __shared__ uint32_t s_c[WPB], s_r[WPB], s_s[WPB];
    __shared__ uint32_t s_d[WPB];
    const PtView v{P.text, P.marks, P.n, 0};
    const bool wide = (reinterpret_cast<uintptr_t>(P.text) & 15u) == 0;
    const unsigned long long n_win = (P.n + CASE_WIN - 1) / CASE_WIN;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    unsigned long long bad = ~0ull;
    uint32_t changed = 0, resized = 0, sigma = 0;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * CASE_WIN + (unsigned long long)threadIdx.x * CASE_PIECE;
        uint32_t outb = 0;
        if (g < P.n) {
            uint32_t x[4] = {0x80808080u, 0u, 0u, 0u};  // (a piece that is not read whole takes the byte loop)
            if (wide && g + CASE_PIECE <= P.n) {
                const uint4 q = *reinterpret_cast<const uint4 *>(P.text + g);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            }
            if (((x[0] | x[1] | x[2] | x[3]) & 0x80808080u) == 0) {
                outb = CASE_PIECE;
                changed += __popc(case_upper_bits4(x[0])) + __popc(case_upper_bits4(x[1])) + __popc(case_upper_bits4(x[2])) + __popc(case_upper_bits4(x[3]));
            } else {
                CaseCounts c{~0ull, 0, 0, 0, 0};
                case_check_piece(v, P.T, g, &c);
                bad = c.bad < bad ? c.bad : bad;
                changed += c.changed;
                resized += c.resized;
                sigma += c.sigma;
                outb = c.out;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) outb += __shfl_xor(outb, o);
        if (lane == 0) s_d[wib] = outb;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t d = 0;
            for (int k = 0; k < WPB; ++k) d += s_d[k];
            P.wout[w] = d;
        }
        __syncthreads();
    }
    if (bad != ~0ull) atomicMin(&P.ctr[0], bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        changed += __shfl_xor(changed, o);
        resized += __shfl_xor(resized, o);
        sigma += __shfl_xor(sigma, o);
    }
    if (lane == 0) {
        s_c[wib] = changed;
        s_r[wib] = resized;
        s_s[wib] = sigma;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one atomic per counter and workgroup
        unsigned long long c = 0, r = 0, sg = 0;
        for (int k = 0; k < WPB; ++k) {
            c += s_c[k];
            r += s_r[k];
            sg += s_s[k];
        }
        if (c) atomicAdd(&P.ctr[1], c);
        if (r) atomicAdd(&P.ctr[2], r);
        if (sg) atomicAdd(&P.ctr[3], sg);
    }
}

// out: 16-byte aligned, n bytes
__global__ __launch_bounds__(BLOCK) void k_case_same(const uint8_t *text, unsigned long long n, CaseTables T, uint8_t *out) {
    const PtView v{text, nullptr, n, 0};
    const bool wide = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    const unsigned long long n_pieces = (n + CASE_PIECE - 1) / CASE_PIECE;
    for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_pieces; p += (unsigned long long)gridDim.x * BLOCK) {
        const unsigned long long g = p * CASE_PIECE;
        const bool whole = g + CASE_PIECE <= n;
        uint4 q = make_uint4(0x80808080u, 0u, 0u, 0u);
        if (wide && whole) q = *reinterpret_cast<const uint4 *>(text + g);
        if (((q.x | q.y | q.z | q.w) & 0x80808080u) == 0) {
            q.x |= case_upper_bits4(q.x);
            q.y |= case_upper_bits4(q.y);
            q.z |= case_upper_bits4(q.z);
            q.w |= case_upper_bits4(q.w);
        } else {
            uint64_t lo, hi;
            case_same_piece(v, T, g, &lo, &hi);
            q = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
        if (whole) {
            *reinterpret_cast<uint4 *>(out + g) = q;
        } else {
            const uint64_t lo = q.x | (uint64_t)q.y << 32, hi = q.z | (uint64_t)q.w << 32;
            for (unsigned long long k = 0; g + k < n; ++k) out[g + k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu);
        }
    }
}

// ---------------------------------------------------------------- final sigma: two windowed scans
struct CaseOp {
    typedef uint32_t State;
    __device__ __forceinline__ State identity() const { return CASE_ST_NONE; }
    __device__ __forceinline__ State combine(State a, State b) const { return case_combine(a, b); }
};

// A piece and its part marks.  plain: 16 ASCII bytes without a part start -- its state comes from the registers, and it holds
// no sigma; every other piece is read through the view by the rules of case_logic.h.
struct CasePiece {
    ScanPiece t, m;
    bool plain;
};

template <ScanDir D>
struct CasePass {
    const uint8_t *text, *marks;  // both 16-byte aligned; marks NULL: the text is one part
    unsigned long long n;
    CaseTables T;
    uint16_t *fin;  // per piece: the sigma bits (forward: written; backward: narrowed to the final ones)
    __device__ __forceinline__ PtView view() const { return PtView{text, marks, n, 0}; }
    __device__ __forceinline__ CasePiece load(unsigned long long g) const {
        CasePiece p;
        p.t = scan_load(text, g, n, 0x80);
        if (marks) {
            p.m = scan_load(marks, g, n, 0);
        } else {  // one part: it starts at byte 0
            p.m.w[0] = g == 0 ? PT_CHUNK0 : 0u;
            p.m.w[1] = p.m.w[2] = p.m.w[3] = 0u;
        }
        p.plain = (((p.t.w[0] | p.t.w[1] | p.t.w[2] | p.t.w[3]) & 0x80808080u) | p.m.w[0] | p.m.w[1] | p.m.w[2] | p.m.w[3]) == 0;
        return p;
    }
    __device__ __forceinline__ uint32_t state(const CasePiece &p, unsigned long long g) const {
        if (g >= n) return CASE_ST_NONE;
        if (p.plain) {
            uint32_t st = CASE_ST_NONE;
#pragma unroll
            for (int j = 0; j < CASE_PIECE; ++j) st = case_combine(st, case_ascii_state(p.t.byte(D == SCAN_FWD ? j : CASE_PIECE - 1 - j)));
            return st;
        }
        return D == SCAN_FWD ? case_piece_fwd(view(), T, g) : case_piece_bwd(view(), T, g);
    }
    __device__ __forceinline__ void finish(uint32_t x, CasePiece &p, unsigned long long g) const {
        if (g >= n) return;
        if (D == SCAN_FWD) {
            fin[g / CASE_PIECE] = p.plain ? (uint16_t)0 : (uint16_t)case_piece_mark_fwd(view(), T, g, x);
        } else {
            const uint32_t m = p.plain ? 0u : fin[g / CASE_PIECE];
            if (m == 0) return;
            const uint32_t f = case_piece_mark_bwd(view(), T, g, x, m);
            if (f != m) fin[g / CASE_PIECE] = (uint16_t)f;
        }
    }
};

__global__ __launch_bounds__(BLOCK) void k_case_fwd_windows(CasePass<SCAN_FWD> P, uint32_t *win) {
    scan_windows_body<SCAN_FWD>(CaseOp{}, P, P.n, win);
}
__global__ __launch_bounds__(BLOCK) void k_case_fwd_carry(uint32_t *win, unsigned long long n_win) {
    scan_carry_body<SCAN_FWD, SCAN_WHOLE>(CaseOp{}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_case_fwd_apply(CasePass<SCAN_FWD> P, const uint32_t *win) {
    scan_apply_body<SCAN_FWD>(CaseOp{}, P, P.n, win);
}
__global__ __launch_bounds__(BLOCK) void k_case_bwd_windows(CasePass<SCAN_BWD> P, uint32_t *win) {
    scan_windows_body<SCAN_BWD>(CaseOp{}, P, P.n, win);
}
__global__ __launch_bounds__(BLOCK) void k_case_bwd_carry(uint32_t *win, unsigned long long n_win) {
    scan_carry_body<SCAN_BWD, SCAN_WHOLE>(CaseOp{}, win, n_win);
}
__global__ __launch_bounds__(BLOCK) void k_case_bwd_apply(CasePass<SCAN_BWD> P, const uint32_t *win) {
    scan_apply_body<SCAN_BWD>(CaseOp{}, P, P.n, win);
}

// Both scans on a text of n > 0 bytes, left in flight on s.  fin: one u16 per piece.
inline hipError_t case_sigma_scans(hipStream_t s, Scratch &S, const uint8_t *text, const uint8_t *marks, unsigned long long n, CaseTables T,
                                   uint16_t *fin) {
    const CasePass<SCAN_FWD> F{text, marks, n, T, fin};
    const CasePass<SCAN_BWD> B{text, marks, n, T, fin};
    uint32_t *wf = nullptr, *wb = nullptr;
    const hipError_t e = scan_launch(
        S, n, &wf, [&](dim3 grid, uint32_t *w) { hipLaunchKernelGGL(k_case_fwd_windows, grid, dim3(BLOCK), 0, s, F, w); },
        [&](uint32_t *w, unsigned long long n_win) { hipLaunchKernelGGL(k_case_fwd_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
        [&](dim3 grid, const uint32_t *w) { hipLaunchKernelGGL(k_case_fwd_apply, grid, dim3(BLOCK), 0, s, F, w); });
    if (e != hipSuccess) return e;
    return scan_launch(
        S, n, &wb, [&](dim3 grid, uint32_t *w) { hipLaunchKernelGGL(k_case_bwd_windows, grid, dim3(BLOCK), 0, s, B, w); },
        [&](uint32_t *w, unsigned long long n_win) { hipLaunchKernelGGL(k_case_bwd_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
        [&](dim3 grid, const uint32_t *w) { hipLaunchKernelGGL(k_case_bwd_apply, grid, dim3(BLOCK), 0, s, B, w); });
}

// ---------------------------------------------------------------- general write
struct CaseWriteParams {
    const uint8_t *text;
    unsigned long long n;
    CaseTables T;
    const uint16_t *fin;              // per piece: the final sigmas (NULL: the text has no sigma)
    const unsigned long long *parts;  // n_parts ascending part starts (device)
    uint32_t n_parts;
    const unsigned long long *rbase;  // per window: first output byte ([n_win] = bytes out)
    uint8_t *out;                     // 16-byte aligned
    unsigned long long *out_off;      // out: n_parts + 1 part offsets into out
    unsigned long long *n_final;      // += the final sigmas written (one atomic per workgroup)
};

// first k in [0, n) with a[k] >= x (n: none)
__device__ __forceinline__ uint32_t case_lower_bound(const unsigned long long *a, uint32_t n, unsigned long long x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

constexpr int CASE_STAGE = CASE_WIN / 2 * 3 + 32;  // a window's output (at most 1.5 x its bytes) behind (its base & 15) bytes

// 16 bytes from registers into the stage at any byte offset: whole dwords where they are the piece's alone, bytes at the two
// ends (the neighbouring pieces write the rest of those dwords).
__device__ __forceinline__ void case_stage16(uint8_t *s, uint32_t at, const uint4 &q) {
    const uint32_t r = at & 3u;
    if (r == 0) {
        uint32_t *d = reinterpret_cast<uint32_t *>(s + at);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        return;
    }
    const uint32_t head = 4u - r, hs = 8u * head;  // bytes in front of the first whole dword: 1..3
    uint32_t *d = reinterpret_cast<uint32_t *>(s + at + head);
    d[0] = q.x >> hs | q.y << (32u - hs);
    d[1] = q.y >> hs | q.z << (32u - hs);
    d[2] = q.z >> hs | q.w << (32u - hs);
    const uint32_t tail = q.w >> hs;  // the last r bytes
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        if (k < head) s[at + k] = (uint8_t)(q.x >> (8u * k));
        if (k < r) s[at + head + 12u + k] = (uint8_t)(tail >> (8u * k));
    }
}

__global__ __launch_bounds__(BLOCK) void k_case_write(CaseWriteParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[CASE_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t s_len[CASE_WIN];  // output bytes of every byte of the window (continuation bytes, bytes past the text: 0)
    __shared__ uint32_t s_tb[BLOCK];      // output bytes in front of every piece
    __shared__ uint32_t s_k[2], s_w[WPB];
    const PtView v{P.text, nullptr, P.n, 0};
    const bool wide = (reinterpret_cast<uintptr_t>(P.text) & 15u) == 0;
    const unsigned long long n_win = (P.n + CASE_WIN - 1) / CASE_WIN;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    uint32_t finals = 0;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long W0 = w * CASE_WIN, g = W0 + (unsigned long long)threadIdx.x * CASE_PIECE;
        const bool last = W0 + CASE_WIN >= P.n;
        // the parts that get their offsets here: those that start in the window (the last window: at the text's end too)
        if (threadIdx.x == 0) s_k[0] = case_lower_bound(P.parts, P.n_parts, W0);
        if (threadIdx.x == 64) s_k[1] = last ? P.n_parts : case_lower_bound(P.parts, P.n_parts, W0 + CASE_WIN);
        const uint32_t nb = g < P.n ? (uint32_t)(g + CASE_PIECE < P.n ? CASE_PIECE : P.n - g) : 0u;  // bytes of this piece
        // a piece of 16 ASCII bytes: one load, 16 output bytes built in registers; every other piece byte by byte
        uint4 q = make_uint4(0x80808080u, 0u, 0u, 0u);
        if (wide && nb == CASE_PIECE) q = *reinterpret_cast<const uint4 *>(P.text + g);
        const bool ascii = ((q.x | q.y | q.z | q.w) & 0x80808080u) == 0;
        uint32_t mine = 0;
        if (ascii) {
            *reinterpret_cast<uint4 *>(s_len + threadIdx.x * CASE_PIECE) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
            mine = CASE_PIECE;
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < CASE_PIECE; ++k) {
                const uint32_t ol = k < nb ? case_byte_out_len(v, P.T, g + k) : 0u;
                s_len[threadIdx.x * CASE_PIECE + k] = (uint8_t)ol;
                mine += ol;
            }
        }
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_w[wib] = inc;
        __syncthreads();
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (int k = 0; k < WPB; ++k) {
            woff += k < wib ? s_w[k] : 0u;
            total += s_w[k];
        }
        const unsigned long long B0 = P.rbase[w];
        const uint32_t sh = (uint32_t)(B0 & 15u);
        uint32_t o = woff + inc - mine;
        s_tb[threadIdx.x] = o;
        if (ascii) {
            q.x |= case_upper_bits4(q.x);
            q.y |= case_upper_bits4(q.y);
            q.z |= case_upper_bits4(q.z);
            q.w |= case_upper_bits4(q.w);
            case_stage16(s_out, sh + o, q);
        } else {
            const uint32_t fin = P.fin && nb ? P.fin[g / CASE_PIECE] : 0u;
            finals += __popc(fin);
#pragma unroll 1
            for (uint32_t k = 0; k < nb; ++k) {
                if (s_len[threadIdx.x * CASE_PIECE + k] == 0) continue;
                uint32_t len;
                case_emit(v, P.T, g + k, (fin >> k) & 1u, s_out + sh + o, &len);
                o += len;
            }
        }
        __syncthreads();
        // part offsets
        for (uint32_t k = s_k[0] + threadIdx.x; k < s_k[1]; k += BLOCK) {
            const uint32_t r = (uint32_t)(P.parts[k] - W0);  // <= CASE_WIN (the text's end in the last window)
            const uint32_t t = r / CASE_PIECE;
            uint32_t x = total;
            if (r < CASE_WIN) {
                x = s_tb[t];
                for (uint32_t q = t * CASE_PIECE; q < r; ++q) x += s_len[q];
            }
            P.out_off[k] = B0 + x;
        }
        if (last && threadIdx.x == 0) P.out_off[P.n_parts] = B0 + total;
        // the stage, window by window of 16 bytes of the output
        const unsigned long long B1 = B0 + total;
        for (unsigned long long a = (B0 - sh) + 16ull * threadIdx.x; a < B1; a += 16ull * BLOCK) {
            const uint32_t at = (uint32_t)(a - (B0 - sh));
            if (a >= B0 && a + 16 <= B1) {
                *reinterpret_cast<uint4 *>(P.out + a) = *reinterpret_cast<const uint4 *>(s_out + at);
            } else {
                for (unsigned long long x = a > B0 ? a : B0; x < a + 16 && x < B1; ++x) P.out[x] = s_out[at + (uint32_t)(x - a)];
            }
        }
        __syncthreads();
    }
    if (!P.fin) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) finals += __shfl_xor(finals, o);
    if (lane == 0) s_w[wib] = finals;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long f = 0;
        for (int k = 0; k < WPB; ++k) f += s_w[k];
        if (f) atomicAdd(P.n_final, f);
    }
}

}  // namespace yb
