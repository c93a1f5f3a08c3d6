// yabpe_dup_kernels.h -- exact-substring duplicates of ragged ids: every run of min_len ids that occurs again, marked and
// optionally removed (rule in dup_logic.h; contract: BBPETokenizer.duplicate_spans, yet_another_bpe/tokenizer.py).  Host
// orchestration: yabpe_dup_spans in yabpe.hip.
//
//   k_dup_plan     one thread per document: its piece count (a piece: up to DUP_TILE consecutive window positions of one
//                  document) and its tile count (a tile: up to DUP_TILE consecutive ids of one document); n_dup[d] = 0, the
//                  counters 0.  exclusive_scan over either gives every document's first piece and first tile.
//   k_dup_insert   one workgroup of four waves per piece.  The piece's ids and the n - 1 behind them go to LDS (2,047 at most).
//                  The Horner prefix P over them is an affine scan: thread t runs Horner serially over elements 8 t .. 8 t + 7
//                  (m() of the eight stays in registers), the thread values are combined across the wave in six shuffle steps
//                  -- every thread spans exactly eight elements, padding included, so step o multiplies by the constant
//                  B^(8 o) -- and across the four waves through LDS: the waves in front of a thread weigh B^(8 lane) there,
//                  which every thread raises itself (dup_pow: at most six rounds of square-and-multiply; carrying the
//                  (B^len, value) pair through the shuffles instead would double them -- neither was measured).  The thread
//                  then replays its eight steps from its exclusive value and leaves P in LDS.  H(p) = P[p + n] - P[p] * B^n: one multiply-subtract per window.
//                  Then CONSECUTIVE LANES OWN CONSECUTIVE POSITIONS: lane l of round j inserts window j * 256 + l.  From the
//                  home slot: an empty slot is claimed with atomicCAS(DUP_EMPTY -> p), and a failed CAS hands back the
//                  resident the thread then looks at; an occupied slot's resident r is compared with p id by id, straight
//                  from ids[] (early exit at the first difference; inside a long repeated span lane l compares against
//                  r + l, so the loads coalesce) -- equal: atomicMin(slot, p) when p is smaller, done; unequal: next slot.
//                  A slot's value only ever moves between positions of EQUAL windows, so a comparison stays valid whatever
//                  the other threads do, every window of a class ends in the same slot, and the slot ends at first[].  One
//                  4-byte array; no key is stored, no value reserved, nobody waits.  The probe loop is bounded by the slot
//                  count.  slot_of[p] = the slot.
//   k_dup_mark     in a launch of its own, once the table is final: one workgroup per tile.  The repeat flags
//                  (table[slot_of[p]] + n <= p) of the tile and of the n positions in front of it inside the document are
//                  staged in LDS as "index + 1 or 0" (n - 1 of them reach into the tile; the n-th gives dup[] of the id in
//                  front of the tile, for the span count), an inclusive max-scan of the same shape as the Horner scan gives
//                  "the last repeat at or before i", and dup[i] is set iff that is less than n back.  n <= 1,024 keeps the
//                  halo within one tile.  dup u8 is written with coalesced stores; the waves' counts meet in LDS, and n_dup[d]
//                  and the three counters take one atomic add a tile (integer adds commute).
//   k_dup_compact  only with YABPE_DUP_COMPACT, after exclusive_scan<uint8_t> over dup[]: id i with dup 0 goes to
//                  i - scan[i]; the new document starts are start - scan[start].
//
// Hashing, equality, min and compare-and-swap have no matrix instruction on gfx950 (MFMA multiplies and sums): VALU and atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dup_logic.h"

namespace yb {

constexpr uint32_t DUP_ITEMS = 2 * DUP_TILE / BLOCK;  // elements a thread scans: tile + halo over the workgroup
static_assert(DUP_ITEMS == 8 && BLOCK == 256, "the scans below: 256 threads x 8 elements = 2,048");
enum { DUP_C_REPEATS, DUP_C_DUP_IDS, DUP_C_SPANS, DUP_COUNTERS };

struct DupParams {
    const uint32_t *ids;
    uint32_t n_ids;
    const unsigned long long *doc_off;    // n_docs document starts (ids), ascending, doc_off[0] = 0
    uint32_t n_docs;
    uint32_t n;                           // min_len
    unsigned long long pow_n;             // B^n
    uint32_t slots_log2;
    uint32_t *pieces, *tiles;             // [n_docs] counts
    const unsigned long long *piece_off, *tile_off;  // [n_docs + 1] their exclusive scans
    uint32_t *table;                      // [slots] window positions
    uint32_t *slot_of;                    // [n_ids] (written at window positions only)
    uint8_t *dup;                         // [n_ids] the result
    unsigned long long *n_dup;            // [n_docs] the result
    unsigned long long *counters;         // [DUP_COUNTERS]
    const unsigned long long *dup_off;    // [n_ids + 1] exclusive scan of dup[] (compaction)
    uint32_t *out_ids;                    // the kept ids
    unsigned long long *out_off;          // [n_docs + 1] their document offsets
};

__device__ __forceinline__ uint32_t dup_doc_end(const DupParams &P, uint32_t d) { return (uint32_t)(d + 1 < P.n_docs ? P.doc_off[d + 1] : P.n_ids); }
__device__ __forceinline__ uint32_t dup_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t dup_lanes(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }  // (wave-uniform)

__global__ __launch_bounds__(BLOCK) void k_dup_plan(DupParams P) {
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    if (d < DUP_COUNTERS) P.counters[d] = 0;
    if (d >= P.n_docs) return;
    const unsigned long long L = dup_doc_end(P, d) - P.doc_off[d];
    P.pieces[d] = (uint32_t)dup_tiles(dup_windows(L, P.n));
    P.tiles[d] = (uint32_t)dup_tiles(L);
    P.n_dup[d] = 0;
}

// B^(8 o) for the shuffle steps o = 1, 2, 4, 8, 16, 32; B^512 shifts over a whole wave
constexpr unsigned long long DUP_POW_WAVE = dup_pow(DUP_B, 64 * DUP_ITEMS);
__device__ __forceinline__ unsigned long long dup_step_pow(int k) {
    constexpr unsigned long long T[6] = {dup_pow(DUP_B, 8), dup_pow(DUP_B, 16), dup_pow(DUP_B, 32), dup_pow(DUP_B, 64), dup_pow(DUP_B, 128), dup_pow(DUP_B, 256)};
    return T[k];
}

__global__ __launch_bounds__(BLOCK) void k_dup_insert(DupParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ids[2 * DUP_TILE];
    __shared__ unsigned long long s_P[2 * DUP_TILE + 1];
    __shared__ unsigned long long s_w[WPB];
    const unsigned long long piece = blockIdx.x;  // (< the number of pieces: the grid)
    const uint32_t d = mh_doc_of(P.piece_off, piece, P.n_docs), n = P.n;
    const uint32_t lo = (uint32_t)P.doc_off[d], W = (uint32_t)dup_windows(dup_doc_end(P, d) - lo, n);
    const uint32_t w0 = (uint32_t)(piece - P.piece_off[d]) * DUP_TILE;  // the piece's first window (w0 < W: d has this piece)
    const uint32_t cnt = W - w0 < DUP_TILE ? W - w0 : DUP_TILE, E = cnt + n - 1;  // (lo + w0 + E <= the document's end)
    const uint32_t base = lo + w0;
    for (uint32_t i = threadIdx.x; i < 2 * DUP_TILE; i += BLOCK) s_ids[i] = i < E ? P.ids[base + i] : 0u;  // (padding: its P is never read)
    __syncthreads();
    // the affine scan: thread t spans elements 8 t .. 8 t + 7
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t e0 = threadIdx.x * DUP_ITEMS;
    const uint4 a = *reinterpret_cast<const uint4 *>(s_ids + e0), b = *reinterpret_cast<const uint4 *>(s_ids + e0 + 4);
    const unsigned long long mv[DUP_ITEMS] = {dup_m(a.x), dup_m(a.y), dup_m(a.z), dup_m(a.w), dup_m(b.x), dup_m(b.y), dup_m(b.z), dup_m(b.w)};
    unsigned long long inc = 0;
#pragma unroll
    for (uint32_t k = 0; k < DUP_ITEMS; ++k) inc = inc * DUP_B + mv[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {  // after the step with o = 2^k lane l holds lanes max(0, l - 2 o + 1) .. l
        const unsigned long long u = __shfl_up(inc, 1u << k);
        if (lane >= (1u << k)) inc = u * dup_step_pow(k) + inc;
    }
    if (lane == 63) s_w[wave] = inc;
    unsigned long long x = __shfl_up(inc, 1);  // exclusive inside the wave
    if (lane == 0) x = 0;
    __syncthreads();
    unsigned long long carry = 0;
    for (uint32_t w = 0; w < wave; ++w) carry = carry * DUP_POW_WAVE + s_w[w];
    x += carry * dup_pow(dup_step_pow(0), lane);  // the waves before, shifted over this lane's 8 * lane elements
    if (threadIdx.x == 0) s_P[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < DUP_ITEMS; ++k) {
        x = x * DUP_B + mv[k];
        s_P[e0 + k + 1] = x;
    }
    __syncthreads();
    // insert: lane l of round j owns window j * BLOCK + l
    const uint32_t n_slots = 1u << P.slots_log2, mask = n_slots - 1;
    for (uint32_t i = threadIdx.x; i < cnt; i += BLOCK) {
        const uint32_t p = base + i;
        uint32_t slot = dup_home(dup_window_hash(s_P[i], s_P[i + n], P.pow_n), P.slots_log2), found = DUP_EMPTY;
        for (uint32_t probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask) {
            uint32_t r = dup_load(&P.table[slot]);
            if (r == DUP_EMPTY) {
                r = atomicCAS(&P.table[slot], DUP_EMPTY, p);
                if (r == DUP_EMPTY) r = p;  // claimed
            }
            bool equal = true;  // (r == p: nothing to compare.  r + n <= n_ids: r starts a window)
            if (r != p)
                for (uint32_t j = 0; j < n; ++j)
                    if (P.ids[r + j] != s_ids[i + j]) {
                        equal = false;
                        break;
                    }
            if (equal) {
                if (r > p) atomicMin(&P.table[slot], p);
                found = slot;
                break;
            }
        }
        P.slot_of[p] = found;  // (DUP_EMPTY only in a table without a free slot, which yabpe_dup_spans refuses)
    }
}

__global__ __launch_bounds__(BLOCK) void k_dup_mark(DupParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_v[2 * DUP_TILE];
    __shared__ uint32_t s_w[WPB], s_cnt[DUP_COUNTERS];
    if (threadIdx.x < DUP_COUNTERS) s_cnt[threadIdx.x] = 0;  // (two barriers lie between this and the adds)
    uint32_t cnt_w[DUP_COUNTERS] = {0, 0, 0};                // this wave's counts
    const unsigned long long tile = blockIdx.x;  // (< the number of tiles: the grid)
    const uint32_t d = mh_doc_of(P.tile_off, tile, P.n_docs), n = P.n;
    const uint32_t lo = (uint32_t)P.doc_off[d], hi = dup_doc_end(P, d);
    const uint32_t t0 = (uint32_t)(tile - P.tile_off[d]) * DUP_TILE;  // the tile's first id inside the document (t0 < hi - lo)
    const uint32_t cnt = hi - lo - t0 < DUP_TILE ? hi - lo - t0 : DUP_TILE;
    const uint32_t halo = t0 ? n : 0u;  // (t0 >= DUP_TILE >= n when it is not 0)
    const uint32_t g0 = lo + t0 - halo, E = halo + cnt;  // staged: positions g0 .. g0 + E - 1, E <= 2,048
#pragma unroll
    for (uint32_t k = 0; k < 2 * DUP_TILE / BLOCK; ++k) {
        const uint32_t j = k * BLOCK + threadIdx.x, p = g0 + j;
        bool rep = false;
        if (j < E && p + n <= hi) {
            const uint32_t slot = P.slot_of[p];
            rep = slot != DUP_EMPTY && dup_is_repeat(P.table[slot], p, n);
        }
        s_v[j] = rep ? j + 1 : 0u;
        cnt_w[DUP_C_REPEATS] += dup_lanes(rep && j >= halo);
    }
    __syncthreads();
    // inclusive max-scan: thread t spans elements 8 t .. 8 t + 7
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t e0 = threadIdx.x * DUP_ITEMS;
    uint4 a = *reinterpret_cast<const uint4 *>(s_v + e0), b = *reinterpret_cast<const uint4 *>(s_v + e0 + 4);
    a.y = max(a.y, a.x); a.z = max(a.z, a.y); a.w = max(a.w, a.z);
    b.x = max(b.x, a.w); b.y = max(b.y, b.x); b.z = max(b.z, b.y); b.w = max(b.w, b.z);
    uint32_t inc = b.w;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc = max(inc, u);
    }
    if (lane == 63) s_w[wave] = inc;
    uint32_t x = __shfl_up(inc, 1);
    if (lane == 0) x = 0;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) x = max(x, s_w[w]);
    a.x = max(a.x, x); a.y = max(a.y, x); a.z = max(a.z, x); a.w = max(a.w, x);
    b.x = max(b.x, x); b.y = max(b.y, x); b.z = max(b.z, x); b.w = max(b.w, x);
    *reinterpret_cast<uint4 *>(s_v + e0) = a;
    *reinterpret_cast<uint4 *>(s_v + e0 + 4) = b;
    __syncthreads();
    // s_v[j] = 1 + the last repeat at or before j, or 0: id j is duplicated iff that repeat starts less than n back
    auto is_dup = [&](uint32_t j) { return s_v[j] != 0 && j + 1 - s_v[j] < n; };
#pragma unroll
    for (uint32_t k = 0; k < DUP_TILE / BLOCK; ++k) {
        const uint32_t i = k * BLOCK + threadIdx.x, j = halo + i;
        const bool in = i < cnt, dp = in && is_dup(j);
        if (in) P.dup[lo + t0 + i] = dp ? 1 : 0;
        cnt_w[DUP_C_DUP_IDS] += dup_lanes(dp);
        cnt_w[DUP_C_SPANS] += dup_lanes(dp && !(j > 0 && is_dup(j - 1)));  // (j == 0: the document's first id)
    }
    if (lane == 0)
        for (uint32_t k = 0; k < DUP_COUNTERS; ++k)
            if (cnt_w[k]) atomicAdd(&s_cnt[k], cnt_w[k]);
    __syncthreads();
    if (threadIdx.x < DUP_COUNTERS && s_cnt[threadIdx.x]) atomicAdd(&P.counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x == DUP_COUNTERS && s_cnt[DUP_C_DUP_IDS]) atomicAdd(&P.n_dup[d], (unsigned long long)s_cnt[DUP_C_DUP_IDS]);
}

__global__ __launch_bounds__(BLOCK) void k_dup_compact(DupParams P) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P.n_ids && !P.dup[i]) P.out_ids[i - P.dup_off[i]] = P.ids[i];
    if (i <= P.n_docs) {
        const uint32_t s = i < P.n_docs ? (uint32_t)P.doc_off[i] : P.n_ids;
        P.out_off[i] = s - P.dup_off[s];
    }
}

}  // namespace yb
