// yabpe_utf8_kernels.h -- errors="replace" / "ignore" for raw text on the device (yabpe_utf8_repair; the rules are in
// utf8_logic.h, shared with the CPU model the tests run against bytes.decode; the kernels only map bytes and tiles to threads).
//
// Input: text in HBM, cut into parts (every part is a text of its own).  Output: the text with every maximal subpart of an
// ill-formed sequence replaced by U+FFFD or dropped, and the part offsets into it.  One workgroup per tile of U8_TILE bytes:
//   check   k_u8_check   a piece of 16 ASCII bytes is one load and one compare; the other pieces run the look-back / look-ahead
//                        on the LDS tile (U8_HALO bytes of the neighbours on either side), a character at a time where the
//                        text is well formed.  Per tile: the output bytes and the
//                        bytes that are not copied; per call: the subparts and the first ill-formed byte (atomicMin).
//                        NO SUBPART: the text is valid, the driver stops here -- the path almost every corpus takes.
//   write   k_u8_write   after the exclusive scan of the tile sums: every tile stages its output in LDS, shifted so that the
//                        16-byte windows of the output are 16-byte windows of the stage, and writes it with 16-byte stores; a
//                        tile whose bytes are all copied skips the rules.  The parts that start in the tile get their new offsets.
// The parts of a tile are looked up once per tile (binary searches by single lanes over the part offsets); where a part
// starts inside the tile or its halo the starts become marks in LDS, which is all the per-byte rules read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "utf8_logic.h"
#include "yabpe_kernels.h"  // BLOCK, WPB

namespace yb {

static_assert(U8_TILE == BLOCK * U8_PIECE, "one piece per thread, one tile per workgroup");
static_assert(U8_HALO >= U8_LOOK && U8_HALO % 16 == 0 && U8_HALO <= BLOCK / 2, "the halo holds the look-around and keeps the tile 16-byte aligned");

// first k in [0, n) with a[k] >= x (n: none)
__device__ __forceinline__ uint32_t u8_lower_bound(const unsigned long long *a, uint32_t n, unsigned long long x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The tile [T0, T0 + U8_TILE) and its halo, inside [0, n), into s_t (s_t[0] = byte T0 - U8_HALO).  -> this thread's piece as
// four words (bytes past the text: 0).  wide: the text is 16-byte aligned.  The caller synchronises.
__device__ __forceinline__ uint4 u8_load_tile(const uint8_t *text, unsigned long long n, unsigned long long T0, bool wide, uint8_t *s_t) {
    const unsigned long long p0 = T0 + (unsigned long long)threadIdx.x * U8_PIECE;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (wide && p0 + U8_PIECE <= n) {
        w = *reinterpret_cast<const uint4 *>(text + p0);
    } else {
        uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < U8_PIECE; ++k)
            if (p0 + k < n) x[k >> 2] |= (uint32_t)text[p0 + k] << ((k & 3) * 8);
        w = make_uint4(x[0], x[1], x[2], x[3]);
    }
    *reinterpret_cast<uint4 *>(s_t + U8_HALO + threadIdx.x * U8_PIECE) = w;
    if (threadIdx.x < 2 * U8_HALO) {
        const bool before = threadIdx.x < U8_HALO;
        const unsigned long long back = U8_HALO - threadIdx.x;  // (before only)
        const unsigned long long x = before ? T0 - back : T0 + U8_TILE + (threadIdx.x - U8_HALO);
        if ((!before || T0 >= back) && x < n) s_t[before ? threadIdx.x : U8_HALO + U8_TILE + (threadIdx.x - U8_HALO)] = text[x];
    }
    return w;
}

// The part starts in [T0 - U8_HALO, T0 + U8_TILE + U8_HALO) as marks in s_m (s_m[0] = byte T0 - U8_HALO).  -> whether there is
// one (false: s_m is left alone).  s_k: 2 words of LDS.  Every thread calls it; it synchronises.
__device__ __forceinline__ bool u8_mark_tile(const unsigned long long *parts, uint32_t n_parts, unsigned long long T0, uint8_t *s_m, uint32_t *s_k) {
    const unsigned long long org = T0 >= U8_HALO ? T0 - U8_HALO : 0;  // (first byte the marks may name)
    if (threadIdx.x == 0) s_k[0] = u8_lower_bound(parts, n_parts, org);
    if (threadIdx.x == 64) s_k[1] = u8_lower_bound(parts, n_parts, T0 + U8_TILE + U8_HALO);
    __syncthreads();
    const uint32_t klo = s_k[0], khi = s_k[1];
    if (klo == khi) return false;
    for (int i = threadIdx.x; i < (U8_TILE + 2 * U8_HALO) / 16; i += BLOCK) reinterpret_cast<uint4 *>(s_m)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint32_t k = klo + threadIdx.x; k < khi; k += BLOCK) s_m[parts[k] + U8_HALO - T0] = 1;  // (equal stores race harmlessly)
    __syncthreads();
    return true;
}

struct U8CheckParams {
    const uint8_t *text;
    unsigned long long n;
    const unsigned long long *parts;  // n_parts ascending part starts (device)
    uint32_t n_parts;
    uint32_t mode;
    uint32_t *osum;                   // out, per tile: output bytes
    uint32_t *tbad;                   // out, per tile: bytes that are not copied (lead or inside of a subpart)
    unsigned long long *ctr;          // [0] first ill-formed byte (atomicMin), [1] += subparts
};

__global__ __launch_bounds__(BLOCK) void k_u8_check(U8CheckParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_t[U8_TILE + 2 * U8_HALO];
    __shared__ __attribute__((aligned(16))) uint8_t s_m[U8_TILE + 2 * U8_HALO];
    __shared__ uint32_t s_k[2], s_o[WPB], s_r[WPB], s_c[WPB];
    __shared__ unsigned long long s_f[WPB];
    const unsigned long long T0 = (unsigned long long)blockIdx.x * U8_TILE, p0 = T0 + (unsigned long long)threadIdx.x * U8_PIECE;
    const bool wide = (reinterpret_cast<uintptr_t>(P.text) & 15u) == 0;
    const uint4 w = u8_load_tile(P.text, P.n, T0, wide, s_t);
    const bool high = ((w.x | w.y | w.z | w.w) & 0x80808080u) != 0;
    // (a tile of ASCII needs neither its parts nor the LDS tile)
    if (!__syncthreads_or(high)) {
        if (threadIdx.x == 0) {
            P.osum[blockIdx.x] = (uint32_t)(T0 + U8_TILE <= P.n ? U8_TILE : P.n - T0);
            P.tbad[blockIdx.x] = 0;
        }
        return;
    }
    const bool marked = u8_mark_tile(P.parts, P.n_parts, T0, s_m, s_k);
    uint32_t outb = 0, rep = 0, chg = 0;
    unsigned long long first = ~0ull;
    if (p0 < P.n) {
        const unsigned long long p1 = p0 + U8_PIECE < P.n ? p0 + U8_PIECE : P.n;
        if (!high) {
            outb = (uint32_t)(p1 - p0);
        } else {
            const U8View v{s_t, s_m, T0 - U8_HALO};
#pragma unroll 1
            for (unsigned long long p = p0; p < p1;) {  // (a character at a time where the text is well formed)
                uint32_t run;
                const uint32_t raw = u8_raw_len(v, p, P.n, marked, &run);
                if (raw == 1u) {
                    const uint32_t take = p + run < p1 ? run : (uint32_t)(p1 - p);
                    outb += take;
                    p += take;
                    continue;
                }
                outb += u8_charge(raw, P.mode);
                ++chg;
                if (raw == 3u) {
                    ++rep;
                    if (p < first) first = p;
                }
                ++p;
            }
        }
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        outb += __shfl_xor(outb, o);
        rep += __shfl_xor(rep, o);
        chg += __shfl_xor(chg, o);
        const unsigned long long f = __shfl_xor(first, o);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_o[wib] = outb;
        s_r[wib] = rep;
        s_c[wib] = chg;
        s_f[wib] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one atomic per counter and tile
        uint32_t a = 0, r = 0, ch = 0;
        unsigned long long f = ~0ull;
        for (int k = 0; k < WPB; ++k) {
            a += s_o[k];
            r += s_r[k];
            ch += s_c[k];
            f = s_f[k] < f ? s_f[k] : f;
        }
        P.osum[blockIdx.x] = a;
        P.tbad[blockIdx.x] = ch;
        if (r) {
            atomicAdd(&P.ctr[1], (unsigned long long)r);
            atomicMin(&P.ctr[0], f);
        }
    }
}

struct U8WriteParams {
    const uint8_t *text;
    unsigned long long n;
    const unsigned long long *parts;  // n_parts ascending part starts (device)
    uint32_t n_parts;
    uint32_t mode;
    const unsigned long long *rbase;  // per tile: first output byte ([n_tiles] = bytes out)
    const uint32_t *tbad;             // per tile: bytes that are not copied (0: the tile is)
    uint8_t *out;                     // 16-byte aligned
    unsigned long long *out_off;      // out: n_parts + 1 part offsets into out
};

__global__ __launch_bounds__(BLOCK) void k_u8_write(U8WriteParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_t[U8_TILE + 2 * U8_HALO];
    __shared__ __attribute__((aligned(16))) uint8_t s_m[U8_TILE + 2 * U8_HALO];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[3 * U8_TILE + 32];  // the tile's output behind (its base & 15) bytes
    __shared__ uint8_t s_len[U8_TILE];   // output bytes of every byte of the tile (bytes past the text: 0)
    __shared__ uint32_t s_tb[BLOCK + 1]; // output bytes in front of every piece; [BLOCK]: the tile's
    __shared__ uint32_t s_k[4], s_w[WPB];
    const unsigned long long T0 = (unsigned long long)blockIdx.x * U8_TILE, p0 = T0 + (unsigned long long)threadIdx.x * U8_PIECE;
    const bool wide = (reinterpret_cast<uintptr_t>(P.text) & 15u) == 0;
    const bool last = T0 + U8_TILE >= P.n;
    (void)u8_load_tile(P.text, P.n, T0, wide, s_t);
    // the parts that get their offsets here: those that start in the tile (the last tile: at the text's end too)
    if (threadIdx.x == 128) s_k[2] = u8_lower_bound(P.parts, P.n_parts, T0);
    if (threadIdx.x == 192) s_k[3] = last ? P.n_parts : u8_lower_bound(P.parts, P.n_parts, T0 + U8_TILE);
    const bool dirty = P.tbad[blockIdx.x] != 0;
    const bool marked = u8_mark_tile(P.parts, P.n_parts, T0, s_m, s_k);  // (synchronises: the tile and s_k are there)
    const unsigned long long B0 = P.rbase[blockIdx.x];
    const uint32_t sh = (uint32_t)(B0 & 15u);
    const uint32_t nb = p0 < P.n ? (uint32_t)(p0 + U8_PIECE < P.n ? U8_PIECE : P.n - p0) : 0u;  // bytes of this piece
    const U8View v{s_t, s_m, T0 - U8_HALO};
    uint32_t total;
    if (!dirty) {
        const uint32_t o = threadIdx.x * U8_PIECE;
        for (uint32_t k = 0; k < nb; ++k) s_out[sh + o + k] = s_t[U8_HALO + o + k];
        total = (uint32_t)(last ? P.n - T0 : U8_TILE);
    } else {
        uint32_t mine = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < U8_PIECE; ++k) {  // (byte by byte: a tile that comes here holds damage, and every byte's charge is kept)
            uint32_t run;
            const uint32_t ol = k < nb ? u8_charge(u8_raw_len(v, p0 + k, P.n, marked, &run), P.mode) : 0u;
            s_len[threadIdx.x * U8_PIECE + k] = (uint8_t)ol;
            mine += ol;
        }
        const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_w[wib] = inc;
        __syncthreads();
        uint32_t woff = 0, all = 0;
#pragma unroll
        for (int w = 0; w < WPB; ++w) {
            woff += w < wib ? s_w[w] : 0u;
            all += s_w[w];
        }
        total = all;
        uint32_t o = woff + inc - mine;
        s_tb[threadIdx.x] = o;
        if (threadIdx.x == 0) s_tb[BLOCK] = all;
#pragma unroll 1
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t ol = s_len[threadIdx.x * U8_PIECE + k];
            dec_emit(s_t[U8_HALO + threadIdx.x * U8_PIECE + k], ol, s_out + sh + o);
            o += ol;
        }
    }
    __syncthreads();
    // part offsets
    for (uint32_t k = s_k[2] + threadIdx.x; k < s_k[3]; k += BLOCK) {
        const uint32_t r = (uint32_t)(P.parts[k] - T0);  // <= U8_TILE (the text's end in the last tile)
        uint32_t o = r;
        if (dirty) {
            const uint32_t t = r / U8_PIECE;
            o = s_tb[t];
            for (uint32_t q = t * U8_PIECE; q < r; ++q) o += s_len[q];
        }
        P.out_off[k] = B0 + o;
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
}

}  // namespace yb
