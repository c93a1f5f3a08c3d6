// yabpe_norm_kernels.h -- Unicode NFC normalisation on the device (yabpe_normalize; the rules are in nfc_logic.h, shared with
// the CPU model the tests run against unicodedata.normalize; the kernels only map bytes and segments to threads).
//
// Input: UTF-8 text in HBM, cut into parts (every part is a text of its own).  Output: the text with every part normalised,
// and the part offsets into it.  Passes:
//   class     k_nfc_class     text, part marks -> the first malformed byte (atomicMin), the number of suspects and, when asked
//                             for, the meta byte of every byte.  A piece of 16 ASCII bytes is one load and one store.
//                             NO SUSPECT: the text is NFC, the driver stops here -- the path almost every corpus takes.
//   find      k_nfc_windows / k_nfc_carry / k_nfc_apply   inclusive max-scan of the segment-start positions in the three
//                             steps of the digit groups (a state per piece and per window, the carry in front of every
//                             window); every suspect marks the start of its segment in a flag array, which k_pt_count /
//                             k_pt_scatter compact into the ascending list of dirty segment starts.  No lane walks a clean
//                             segment, none walks backwards.
//   segments  k_nfc_short     one lane per dirty segment walks it forward, decomposes into a buffer of NFC_SHORT entries in
//                             LDS, insertion-sorts, composes; first for the lengths, after the scan of out - in for the bytes
//             k_nfc_long      the segments that did not fit: one wave each, buffers in global scratch sized from the measured
//                             lengths, counting sort over the 255 classes, the same linear compose (nfc_logic.h)
//   write     k_nfc_copy      every byte outside a dirty segment goes to i + shift; the dirty segments around a window are
//                             found once per window by binary search
//             k_nfc_offsets   the part offsets, moved the same way
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nfc_logic.h"
#include "yabpe_aux_kernels.h"
#include "yabpe_scan_kernels.h"

namespace yb {

static_assert(NFC_WIN == SCAN_WIN && NFC_PIECE == SCAN_PIECE, "one piece per thread, one window per workgroup");

// 16 bytes at g (a multiple of 16) as four words; bytes past the array read as 0.  wide: the array is 16-byte aligned.
__device__ __forceinline__ void nfc_load(const uint8_t *a, unsigned long long g, unsigned long long n, bool wide, uint32_t w[4]) {
    if (wide && g + NFC_PIECE <= n) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + g);
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = 0u;
#pragma unroll
        for (int k = 0; k < NFC_PIECE; ++k)
            if (g + k < n) w[k >> 2] |= (uint32_t)a[g + k] << ((k & 3) * 8);
    }
}
__device__ __forceinline__ uint8_t nfc_byte(const uint32_t w[4], int k) { return (uint8_t)(w[k >> 2] >> ((k & 3) * 8)); }

// ctr[0]: smallest malformed byte position (~0: none), ctr[1]: suspects.  meta may be NULL (the first, counting run).
__global__ __launch_bounds__(BLOCK) void k_nfc_class(const uint8_t *text, const uint8_t *marks, uint8_t *meta, unsigned long long n, NfcTables T,
                                                     unsigned long long *ctr) {
    const PtView v{text, marks, n, 0};
    const bool wide = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    const unsigned long long n_pieces = (n + NFC_PIECE - 1) / NFC_PIECE;
    unsigned long long bad_pos = ~0ull, suspects = 0;
    for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_pieces; p += (unsigned long long)gridDim.x * BLOCK) {
        const unsigned long long g = p * NFC_PIECE;
        uint32_t w[4], o[4] = {0u, 0u, 0u, 0u};
        nfc_load(text, g, n, wide, w);
        if (((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) == 0) {  // ASCII: every byte starts a segment
            o[0] = o[1] = o[2] = o[3] = NFC_START * 0x01010101u;
        } else {
#pragma unroll 1
            for (int k = 0; k < NFC_PIECE && g + k < n; ++k) {
                const unsigned long long i = g + k;
                uint8_t m = NFC_START;
                if (nfc_byte(w, k) & 0x80) {
                    unsigned long long end = n;
                    for (unsigned long long q = i + 1; q < i + 4 && q < n; ++q)
                        if (marks[q] & NFC_PART0) {
                            end = q;
                            break;
                        }
                    bool bad = false;
                    m = nfc_classify(v, i, end, T, &bad);
                    if (bad && i < bad_pos) bad_pos = i;
                    if (m & NFC_SUSPECT) ++suspects;
                }
                o[k >> 2] |= (uint32_t)m << ((k & 3) * 8);
            }
        }
        if (meta) {
            if (g + NFC_PIECE <= n) {
                *reinterpret_cast<uint4 *>(meta + g) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
                for (int k = 0; k < NFC_PIECE && g + k < n; ++k) meta[g + k] = nfc_byte(o, k);
            }
        }
    }
    if (bad_pos != ~0ull) atomicMin(&ctr[0], bad_pos);
    suspects = wave_sum_u64(suspects);
    if ((threadIdx.x & 63) == 0 && suspects) atomicAdd(&ctr[1], suspects);
}

// The segment start in front of every byte: a forward scan in the three launches of yabpe_scan_kernels.h.
struct NfcOp {
    typedef NfcPos State;
    __device__ __forceinline__ State identity() const { return 0; }
    __device__ __forceinline__ State combine(State a, State b) const { return nfc_combine(a, b); }
};

struct NfcPass { // (no finish: k_nfc_apply has a loop of its own, 1 VGPR cheaper than through scan_apply_body)
    const uint8_t *meta;
    unsigned long long n;
    __device__ __forceinline__ ScanPiece load(unsigned long long g) const { return scan_load(meta, g, n, 0); }
    __device__ __forceinline__ NfcPos state(const ScanPiece &m, unsigned long long g) const {
        return nfc_piece_state([&](int k) { return m.byte(k); }, g);
    }
};

__global__ __launch_bounds__(BLOCK) void k_nfc_windows(const uint8_t *meta, unsigned long long n, NfcPos *win) {
    scan_windows_body<SCAN_FWD>(NfcOp{}, NfcPass{meta, n}, n, win);
}
__global__ __launch_bounds__(BLOCK) void k_nfc_carry(NfcPos *win, unsigned long long n_win) {
    scan_carry_body<SCAN_FWD, SCAN_WHOLE>(NfcOp{}, win, n_win);
}
// flags[start of its segment] = 1 for every suspect (flags was zeroed; equal stores race harmlessly)
__global__ __launch_bounds__(BLOCK) void k_nfc_apply(const uint8_t *meta, unsigned long long n, const NfcPos *win, uint8_t *flags) {
    __shared__ NfcPos s_w[WPB];
    const NfcOp op;
    const unsigned long long n_win = (n + NFC_WIN - 1) / NFC_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * NFC_WIN + (unsigned long long)threadIdx.x * NFC_PIECE;
        const ScanPiece m = scan_load(meta, g, n, 0);
        auto get = [&](int k) { return m.byte(k); };
        NfcPos total;
        const NfcPos before = nfc_combine(win[w], scan_block<SCAN_FWD>(op, nfc_piece_state(get, g), s_w, &total));
        if ((m.w[0] | m.w[1] | m.w[2] | m.w[3]) & (NFC_SUSPECT * 0x01010101u))
            nfc_piece_mark(before, get, g, [&](uint64_t p) { flags[p] = 1; });
        __syncthreads();
    }
}

// The three steps on the meta bytes of n > 0 bytes, left in flight on s.  *win belongs to S.
inline hipError_t nfc_find(hipStream_t s, Scratch &S, const uint8_t *meta, uint8_t *flags, unsigned long long n, NfcPos **win) {
    return scan_launch(
        S, n, win, [&](dim3 grid, NfcPos *w) { hipLaunchKernelGGL(k_nfc_windows, grid, dim3(BLOCK), 0, s, meta, n, w); },
        [&](NfcPos *w, unsigned long long n_win) { hipLaunchKernelGGL(k_nfc_carry, dim3(1), dim3(BLOCK), 0, s, w, n_win); },
        [&](dim3 grid, const NfcPos *w) { hipLaunchKernelGGL(k_nfc_apply, grid, dim3(BLOCK), 0, s, meta, n, w, flags); });
}

// ---------------------------------------------------------------- dirty segments
struct NfcLaneBuf {  // entry i of this lane's buffer: the lanes of a wave hit 64 different banks
    uint32_t *p;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return p[i * BLOCK]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t e) { p[i * BLOCK] = e; }
};
struct NfcGlobalBuf {
    uint32_t *p;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return p[i]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t e) { p[i] = e; }
};

struct NfcSegParams {
    const uint8_t *text, *meta;
    unsigned long long n;
    NfcTables T;
    const unsigned long long *dstart;  // n_dirty ascending segment starts
    unsigned long long n_dirty;
    unsigned long long *dend;          // first byte behind each segment
    unsigned long long *delta;         // bytes out - bytes in (mod 2^64)
    uint32_t *nent;                    // decomposed code points of a segment of the long path, 0 for the short path
    unsigned long long *long_list;     // the segments of the long path, in any order
    unsigned long long *ctr;           // [0] start of the first segment over NFC_CAP (atomicMin, ~0: none), [1] length of long_list
    // second pass (write != 0)
    const unsigned long long *shift;   // exclusive scan of delta
    uint8_t *out;
    // long path
    const unsigned long long *loff;    // exclusive scan of nent: a segment's place in gbuf / gtmp
    uint32_t *gbuf, *gtmp;
};

__global__ __launch_bounds__(BLOCK) void k_nfc_short(NfcSegParams P, int write) {
    __shared__ uint32_t s_buf[NFC_SHORT * BLOCK];
    const PtView v{P.text, P.meta, P.n, 0};
    NfcLaneBuf b{s_buf + threadIdx.x};
    for (unsigned long long d = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; d < P.n_dirty; d += (unsigned long long)gridDim.x * BLOCK) {
        if (write && P.nent[d]) continue;
        const unsigned long long s = P.dstart[d];
        const NfcSeg seg = nfc_seg_fill(P.T, v, s, b, NFC_SHORT);
        if (!write) {
            P.dend[d] = seg.end;
            P.delta[d] = 0;
            P.nent[d] = 0;
            if (seg.in_cps > NFC_CAP) {
                atomicMin(&P.ctr[0], s);  // (the call fails: nobody writes this segment)
                continue;
            }
            if (seg.n_ent > NFC_SHORT) {
                P.nent[d] = seg.n_ent;
                P.long_list[atomicAdd(&P.ctr[1], 1ull)] = d;
                continue;
            }
        }
        nfc_sort_insert(b, 0, seg.n_ent);
        const uint32_t m = nfc_compose(P.T, b, seg.n_ent);
        if (write) (void)nfc_emit(b, m, P.out + s + P.shift[d]);
        else P.delta[d] = nfc_emit(b, m, nullptr) - (seg.end - s);
    }
}

// one wave per segment of the long path; its first lane walks, the buffers are the segment's slices of gbuf / gtmp
__global__ __launch_bounds__(BLOCK) void k_nfc_long(NfcSegParams P, unsigned long long n_long, int write) {
    __shared__ uint32_t s_cnt[WPB][256];
    const PtView v{P.text, P.meta, P.n, 0};
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (unsigned long long w = (unsigned long long)blockIdx.x * WPB + wib; w < n_long; w += (unsigned long long)gridDim.x * WPB) {
        if (lane) continue;
        const unsigned long long d = P.long_list[w], s = P.dstart[d];
        NfcGlobalBuf b{P.gbuf + P.loff[d]}, t{P.gtmp + P.loff[d]};
        const NfcSeg seg = nfc_seg_fill(P.T, v, s, b, P.nent[d]);
        nfc_sort_long(b, t, seg.n_ent, s_cnt[wib]);
        const uint32_t m = nfc_compose(P.T, b, seg.n_ent);
        if (write) (void)nfc_emit(b, m, P.out + s + P.shift[d]);
        else P.delta[d] = nfc_emit(b, m, nullptr) - (seg.end - s);
    }
}

// ---------------------------------------------------------------- write
__global__ __launch_bounds__(BLOCK) void k_nfc_copy(const uint8_t *text, unsigned long long n, const unsigned long long *dstart,
                                                    const unsigned long long *dend, const unsigned long long *shift, unsigned long long n_dirty,
                                                    uint8_t *out, unsigned long long *copied) {
    __shared__ unsigned long long s_k[2];
    const unsigned long long n_win = (n + NFC_WIN - 1) / NFC_WIN;
    unsigned long long mine = 0;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long base = w * NFC_WIN, top = base + NFC_WIN < n ? base + NFC_WIN : n;
        if (threadIdx.x == 0) s_k[0] = nfc_lower_bound(dstart, 0, n_dirty, base + 1);  // segments that start at or before the window's first byte
        if (threadIdx.x == 64) s_k[1] = nfc_lower_bound(dstart, 0, n_dirty, top);      // ... or anywhere in front of its end
        __syncthreads();
        const unsigned long long klo = s_k[0], khi = s_k[1];
        if (klo == khi && (klo == 0 || dend[klo - 1] <= base)) {  // no dirty byte in the window: one shift, consecutive lanes take consecutive bytes
            const unsigned long long sh = shift[klo];
            for (unsigned long long i = base + threadIdx.x; i < top; i += BLOCK, ++mine) out[i + sh] = text[i];
        } else {
            const unsigned long long g = base + (unsigned long long)threadIdx.x * NFC_PIECE;
            uint64_t k = nfc_lower_bound(dstart, klo, khi, g + 1);
            for (int j = 0; j < NFC_PIECE && g + j < top; ++j) {
                uint64_t dst = 0;
                if (nfc_copy_dst(dstart, dend, shift, khi, g + j, &k, &dst)) {
                    out[dst] = text[g + j];
                    ++mine;
                }
            }
        }
        __syncthreads();
    }
    mine = wave_sum_u64(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(copied, mine);
}

// out_off[p] = part_off[p] moved by the segments in front of it (a part start is a segment start), out_off[n_parts] = n_out
__global__ __launch_bounds__(BLOCK) void k_nfc_offsets(const unsigned long long *part_off, uint32_t n_parts, unsigned long long n_out,
                                                       const unsigned long long *dstart, const unsigned long long *shift, unsigned long long n_dirty,
                                                       unsigned long long *out_off) {
    const unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p > n_parts) return;
    if (p == n_parts) {
        out_off[p] = n_out;
        return;
    }
    const unsigned long long x = part_off[p];
    out_off[p] = x + shift[nfc_lower_bound(dstart, 0, n_dirty, x)];
}

} // namespace yb
