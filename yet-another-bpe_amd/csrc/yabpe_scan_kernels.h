// yabpe_scan_kernels.h -- the windowed scan of a per-byte monoid over text of any length ("The windowed-scan
// template"): the one skeleton under the digit groups, the newline rules, the o200k_base look-ahead and scanner
// (yabpe_pretok_kernels.h) and the NFC segment starts (yabpe_norm_kernels.h).  A thread owns a piece of SCAN_PIECE = 16 bytes,
// kept in registers; a workgroup a window of SCAN_WIN bytes.  Three launches:
//   windows   per window: the states of its pieces combined into one
//   carry     one workgroup: exclusive scan of the window states, in place -> the state in front of (behind) every window
//   apply     per window: exclusive scan of the piece states behind that carry, then every thread rewrites its piece
// A family supplies
//   an operation   struct { typedef ... State; State identity() const; State combine(State a, State b) const; }: first a, then
//                  b (backward: a is the farther one).  An object, not a set of static functions: it may carry parameters.
//   a pass         struct { P load(g) const; State state(const P &, g) const; void finish(State x, P &, g) const; }: the thread's
//                  piece at byte g (a multiple of 16), its state, and what apply writes given x = everything in front of
//                  (behind) the piece
// and its three kernels as plain __global__ wrappers around scan_windows_body / scan_carry_body / scan_apply_body.  Where a
// body costs a kernel registers (the resource guards under tests/ hold every kernel to what it used before there was a
// template), that kernel keeps a loop of its own over the parts that cost it nothing: the apply kernels of the digit groups (scan_block;
// its store is written out) and of NFC (scan_block, scan_load), and the two-direction kernels of the newline rules (scan_store).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yabpe_aux_kernels.h"

namespace yb {

constexpr int SCAN_PIECE = 16;               // bytes one thread owns: one 16-B load
constexpr int SCAN_WIN = BLOCK * SCAN_PIECE; // bytes per workgroup and iteration
constexpr int SCAN_CARRY_ITEMS = 8;          // window states per thread and iteration of the carry kernel

// SCAN_FWD: over the threads in front, in thread order.  SCAN_BWD: over the threads behind, the nearest last.
enum ScanDir { SCAN_FWD, SCAN_BWD };

// ---------------------------------------------------------------- pieces
// A piece is indexed by unrolled constants only: a runtime index would move it out of the registers.
struct ScanPiece {
    uint32_t w[4];
    __device__ __forceinline__ uint8_t byte(int k) const { return (uint8_t)(w[k >> 2] >> ((k & 3) * 8)); }
};

// the 16 bytes of a at g (a multiple of 16); bytes past n read as `fill`
__device__ __forceinline__ ScanPiece scan_load(const uint8_t *a, unsigned long long g, unsigned long long n, uint32_t fill) {
    ScanPiece p;
    if (g + SCAN_PIECE <= n) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + g);
        p.w[0] = x.x; p.w[1] = x.y; p.w[2] = x.z; p.w[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.w[k] = fill * 0x01010101u;
#pragma unroll
        for (int k = 0; k < SCAN_PIECE; ++k)
            if (g + k < n) {
                const int sh = (k & 3) * 8;
                p.w[k >> 2] = (p.w[k >> 2] & ~(0xFFu << sh)) | ((uint32_t)a[g + k] << sh);
            }
    }
    return p;
}

__device__ __forceinline__ void scan_store(uint8_t *a, unsigned long long g, unsigned long long n, const uint32_t w[4]) {
    if (g + SCAN_PIECE <= n) {
        *reinterpret_cast<uint4 *>(a + g) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_PIECE; ++k)
            if (g + k < n) a[g + k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
    }
}

// ---------------------------------------------------------------- one workgroup, one state per thread
// Exclusive scan of one state per thread over the workgroup; *total = all of them combined.  s_w: WPB states in LDS, free
// again after the caller's next __syncthreads().
template <ScanDir D, class Op>
__device__ __forceinline__ typename Op::State scan_block(const Op &op, typename Op::State mine, typename Op::State *s_w,
                                                         typename Op::State *total) {
    typedef typename Op::State State;
    constexpr bool FWD = D == SCAN_FWD;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    // in the wave: the inclusive scan by shuffles; the wave's last lane in scan order leaves the wave's value in LDS
    State inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const State u = FWD ? __shfl_up(inc, o) : __shfl_down(inc, o);
        if (FWD ? lane >= o : lane + o < 64) inc = op.combine(u, inc);
    }
    const State next = FWD ? __shfl_up(inc, 1) : __shfl_down(inc, 1); // the neighbour's inclusive value = this lane's exclusive one
    if (lane == (FWD ? 63 : 0)) s_w[wib] = inc;
    __syncthreads();
    // across the waves, folded in scan order
    State before = op.identity(), all = op.identity();
#pragma unroll
    for (int i = 0; i < WPB; ++i) {
        const int w = FWD ? i : WPB - 1 - i;
        if (w == wib) before = all;
        all = op.combine(all, s_w[w]);
    }
    *total = all;
    return lane != (FWD ? 0 : 63) ? op.combine(before, next) : before;
}

// ---------------------------------------------------------------- the three kernel bodies
template <ScanDir D, class Op, class Pass>
__device__ __forceinline__ void scan_windows_body(const Op &op, const Pass &pass, unsigned long long n, typename Op::State *win) {
    __shared__ typename Op::State s_w[WPB];
    const unsigned long long n_win = (n + SCAN_WIN - 1) / SCAN_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * SCAN_WIN + (unsigned long long)threadIdx.x * SCAN_PIECE;
        const auto p = pass.load(g);
        typename Op::State total;
        (void)scan_block<D>(op, pass.state(p, g), s_w, &total);
        if (threadIdx.x == 0) win[w] = total;
        __syncthreads();
    }
}

// A piece is read as the passes before left it by the thread that then, in finish, writes it.
template <ScanDir D, class Op, class Pass>
__device__ __forceinline__ void scan_apply_body(const Op &op, const Pass &pass, unsigned long long n, const typename Op::State *win) {
    __shared__ typename Op::State s_w[WPB];
    const unsigned long long n_win = (n + SCAN_WIN - 1) / SCAN_WIN;
    for (unsigned long long w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned long long g = w * SCAN_WIN + (unsigned long long)threadIdx.x * SCAN_PIECE;
        auto p = pass.load(g);
        typename Op::State total;
        const typename Op::State in = scan_block<D>(op, pass.state(p, g), s_w, &total);
        pass.finish(op.combine(win[w], in), p, g);
        __syncthreads();
    }
}

// The part of a window state the carry kernel scans: all of it, or one value of a packed pair (the other one stays).
enum ScanField { SCAN_WHOLE, SCAN_LO, SCAN_HI };
template <ScanField F, class Op>
__device__ __forceinline__ typename Op::State scan_get(const Op &op, typename Op::State x) {
    if constexpr (F == SCAN_WHOLE) return x;
    else return F == SCAN_LO ? op.lo(x) : op.hi(x);
}
template <ScanField F, class Op>
__device__ __forceinline__ typename Op::State scan_set(const Op &op, typename Op::State x, typename Op::State v) {
    if constexpr (F == SCAN_WHOLE) return v;
    else return F == SCAN_LO ? op.pack(v, op.hi(x)) : op.pack(op.lo(x), v);
}

// One workgroup: win[w] = the states of the windows in front of (D = SCAN_BWD: behind) w combined, in place, a tile of
// BLOCK * SCAN_CARRY_ITEMS states per iteration.  A thread reads its states of a tile, then writes the same ones: no state
// passes between threads through memory.  Slots past n_win read as the identity.
template <ScanDir D, ScanField F, class Op>
__device__ __forceinline__ void scan_carry_body(const Op &op, typename Op::State *win, unsigned long long n_win) {
    typedef typename Op::State State;
    __shared__ State s_w[WPB];
    constexpr unsigned long long TILE = (unsigned long long)BLOCK * SCAN_CARRY_ITEMS;
    const unsigned long long last = (n_win + TILE - 1) / TILE * TILE - TILE; // the tile that holds the last window
    State carry = op.identity();
    for (unsigned long long t = 0; t < n_win; t += TILE) {
        const unsigned long long base = (D == SCAN_FWD ? t : last - t) + (unsigned long long)threadIdx.x * SCAN_CARRY_ITEMS;
        State v[SCAN_CARRY_ITEMS], mine = op.identity();
#pragma unroll
        for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) {
            const int k = D == SCAN_FWD ? j : SCAN_CARRY_ITEMS - 1 - j;
            v[k] = base + k < n_win ? win[base + k] : scan_set<F>(op, State(0), op.identity());
            mine = op.combine(mine, scan_get<F>(op, v[k]));
        }
        State total;
        State run = op.combine(carry, scan_block<D>(op, mine, s_w, &total));
#pragma unroll
        for (int j = 0; j < SCAN_CARRY_ITEMS; ++j) {
            const int k = D == SCAN_FWD ? j : SCAN_CARRY_ITEMS - 1 - j;
            if (base + k < n_win) win[base + k] = scan_set<F>(op, v[k], run);
            run = op.combine(run, scan_get<F>(op, v[k]));
        }
        carry = op.combine(carry, total);
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host
// The three launches on a text of n > 0 bytes, left in flight on s.  *win (one state per window) is taken from S.
// windows(grid, win), carry(win, n_win) and apply(grid, win) launch the family's kernels on s with BLOCK threads.
// Returns the error of the allocation or of the launches, for the caller to report.
template <class State, class Windows, class Carry, class Apply>
inline hipError_t scan_launch(Scratch &S, unsigned long long n, State **win, Windows windows, Carry carry, Apply apply) {
    const unsigned long long n_win = (n + SCAN_WIN - 1) / SCAN_WIN;
    const hipError_t e = S.get(win, n_win);
    if (e != hipSuccess) return e;
    const dim3 wgrid((uint32_t)std::min<unsigned long long>(n_win, 1u << 20));
    windows(wgrid, *win);
    carry(*win, n_win);
    apply(wgrid, (const State *)*win);
    return hipGetLastError();
}

} // namespace yb
