// yabpe_decode_kernels.h -- BBPETokenizer.decode on the device (yet_another_bpe/tokenizer.py; rules in decode_logic.h).
//
// Passes (host orchestration: yabpe_decode in yabpe.hip):
//   lengths   k_dec_lengths: per block of DEC_IPB ids, the sum of their byte lengths; exclusive_scan -> each block's output base
//   gather    k_dec_gather: the block re-reads its ids, forms the in-block prefix in registers and copies the token bytes from
//             the pool (L2-resident) into an LDS stage that it writes out with 16-B stores, window by window when the block's
//             output is larger than the stage; it also writes the byte offset of every document that starts in its ids
//   check     k_dec_check: per tile of DEC_TILE gathered bytes, the output bytes every byte is charged (decode_logic.h) and
//             the U+FFFD count.  Tiles of ASCII need no look-around at all.
//   repair    (only when a U+FFFD is due) exclusive_scan of the tile sums -> k_dec_repair rewrites every tile with U+FFFD in
//             place of each maximal subpart and moves the document offsets with it
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_logic.h"
#include "yabpe_kernels.h" // BLOCK, WPB

namespace yb {

constexpr int DEC_IPT = 8;                  // ids per thread
constexpr int DEC_IPB = BLOCK * DEC_IPT;    // ids per block
constexpr int DEC_STAGE = 16384;            // bytes of the gather's LDS stage (a multiple of 16)
constexpr int DEC_TPT = 16;                 // gathered bytes per thread in check / repair
constexpr int DEC_TILE = BLOCK * DEC_TPT;   // gathered bytes per block in check / repair
constexpr int DEC_HALO = 16;                // LDS bytes on either side of a tile (dec_out_len looks 3 bytes each way)

struct DecTable {
    const uint2 *ent;   // id -> (offset into pool, length); offset DEC_UNKNOWN = no bytes
    uint32_t n;         // ids in the table
    const uint8_t *pool;
};

__device__ __forceinline__ uint2 dec_entry(const DecTable &t, uint32_t id) {
    return id < t.n ? t.ent[id] : make_uint2(DEC_UNKNOWN, 0u);
}

// exclusive prefix of v over the block (every thread calls it); *total = the block's sum.  s_w: WPB entries of LDS.
__device__ __forceinline__ unsigned long long dec_block_scan(unsigned long long v, unsigned long long *s_w, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_w[wib] = inc;
    __syncthreads();
    unsigned long long woff = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WPB; ++w) {
        woff += w < wib ? s_w[w] : 0ull;
        all += s_w[w];
    }
    __syncthreads(); // (s_w may be reused)
    *total = all;
    return woff + inc - v;
}

// The DEC_IPT ids of this thread: ids[i0 + DEC_IPT * tid ...] (ids 16-B aligned: the host stages misaligned input).
__device__ __forceinline__ void dec_load_ids(const uint32_t *ids, unsigned long long n_ids, unsigned long long first, uint32_t (&id)[DEC_IPT],
                                             uint32_t &cnt) {
    if (first + DEC_IPT <= n_ids) {
        const uint4 a = *reinterpret_cast<const uint4 *>(ids + first), b = *reinterpret_cast<const uint4 *>(ids + first + 4);
        id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w; id[4] = b.x; id[5] = b.y; id[6] = b.z; id[7] = b.w;
        cnt = DEC_IPT;
        return;
    }
    cnt = first < n_ids ? (uint32_t)(n_ids - first) : 0u;
#pragma unroll
    for (int k = 0; k < DEC_IPT; ++k) id[k] = (uint32_t)k < cnt ? ids[first + k] : 0u;
}

// bsum[b] = bytes of block b's ids; counters[0] += ids not in the table
__global__ __launch_bounds__(BLOCK) void k_dec_lengths(const uint32_t *ids, unsigned long long n_ids, DecTable tab, unsigned long long *bsum,
                                                       unsigned long long *counters) {
    __shared__ unsigned long long s_w[WPB], s_u[WPB];
    uint32_t id[DEC_IPT], cnt;
    dec_load_ids(ids, n_ids, (unsigned long long)blockIdx.x * DEC_IPB + (unsigned long long)threadIdx.x * DEC_IPT, id, cnt);
    unsigned long long sum = 0, unk = 0;
#pragma unroll
    for (int k = 0; k < DEC_IPT; ++k) {
        if ((uint32_t)k >= cnt) break;
        const uint2 e = dec_entry(tab, id[k]);
        sum += e.y;
        unk += e.x == DEC_UNKNOWN ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        unk += __shfl_xor(unk, o);
    }
    if (lane == 0) {
        s_w[wib] = sum;
        s_u[wib] = unk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0, u = 0;
        for (int w = 0; w < WPB; ++w) {
            a += s_w[w];
            u += s_u[w];
        }
        bsum[blockIdx.x] = a;
        if (u) atomicAdd(&counters[0], u);
    }
}

struct DecGatherParams {
    const uint32_t *ids;
    unsigned long long n_ids;
    DecTable tab;
    const unsigned long long *bbase;  // per block: first output byte (exclusive scan of k_dec_lengths' sums; [nb] = total)
    const unsigned long long *doc;    // n_docs document starts (ids), ascending, doc[0] = 0
    uint32_t n_docs;
    uint8_t *out;                     // gathered bytes (16-B aligned)
    unsigned long long *gdoc;         // out: n_docs + 1 byte offsets of the documents in out
};

__global__ __launch_bounds__(BLOCK) void k_dec_gather(DecGatherParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[DEC_STAGE];
    __shared__ unsigned long long s_tbase[BLOCK];
    __shared__ unsigned long long s_w[WPB];
    __shared__ uint32_t s_d0;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * DEC_IPB, first = i0 + (unsigned long long)threadIdx.x * DEC_IPT;
    const unsigned long long i1 = i0 + DEC_IPB < P.n_ids ? i0 + DEC_IPB : P.n_ids;
    uint32_t id[DEC_IPT], cnt;
    dec_load_ids(P.ids, P.n_ids, first, id, cnt);
    uint2 e[DEC_IPT];
    unsigned long long tsum = 0;
#pragma unroll
    for (int k = 0; k < DEC_IPT; ++k) {
        e[k] = (uint32_t)k < cnt ? dec_entry(P.tab, id[k]) : make_uint2(0u, 0u);
        tsum += e[k].y;
    }
    if (threadIdx.x == 0) { // the first document that starts at or after i0
        uint32_t lo = 0, hi = P.n_docs;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.doc[mid] >= i0) hi = mid; else lo = mid + 1;
        }
        s_d0 = lo;
    }
    unsigned long long total;
    const unsigned long long tbase = dec_block_scan(tsum, s_w, &total);
    s_tbase[threadIdx.x] = tbase;
    __syncthreads();
    const unsigned long long B0 = P.bbase[blockIdx.x], B1 = B0 + total;
    // document offsets: every document that starts in [i0, i1) (the last block also takes those that start at n_ids)
    const bool last = i1 == P.n_ids;
    for (uint32_t d = s_d0 + threadIdx.x; d < P.n_docs; d += BLOCK) {
        const unsigned long long j = P.doc[d];
        if (j > i1 || (j == i1 && !last)) break;
        unsigned long long o = B1;
        if (j < i1) {
            const unsigned long long r = j - i0, t0 = r / DEC_IPT;
            o = B0 + s_tbase[t0];
            for (unsigned long long q = i0 + t0 * DEC_IPT; q < j; ++q) o += dec_entry(P.tab, P.ids[q]).y;
        }
        P.gdoc[d] = o;
    }
    if (last && threadIdx.x == 0) P.gdoc[P.n_docs] = B1;
    // the bytes, one stage window at a time; windows are 16-B aligned in the output
    for (unsigned long long ws = B0 & ~15ull; ws < B1; ws += DEC_STAGE) {
        const unsigned long long we = ws + DEC_STAGE;
        __syncthreads(); // the previous window has been written out
        unsigned long long o = B0 + tbase;
#pragma unroll
        for (int k = 0; k < DEC_IPT; ++k) {
            const unsigned long long a = o > ws ? o : ws, z = o + e[k].y < we ? o + e[k].y : we;
            for (unsigned long long x = a; x < z; ++x) s_stage[x - ws] = P.tab.pool[e[k].x + (x - o)];
            o += e[k].y;
        }
        __syncthreads();
        const unsigned long long lo = ws > B0 ? ws : B0, hi = we < B1 ? we : B1;
        for (unsigned long long a = ws + 16ull * threadIdx.x; a < hi; a += 16ull * BLOCK) {
            if (a >= lo && a + 16 <= hi) {
                *reinterpret_cast<uint4 *>(P.out + a) = *reinterpret_cast<const uint4 *>(s_stage + (a - ws));
            } else {
                for (unsigned long long x = a > lo ? a : lo; x < a + 16 && x < hi; ++x) P.out[x] = s_stage[x - ws];
            }
        }
    }
}

// The tile [T0, T0 + DEC_TILE) of the gathered text and DEC_HALO bytes on either side, inside [0, n).  -> this thread's 16 bytes.
__device__ __forceinline__ uint4 dec_load_tile(const uint8_t *g, unsigned long long n, unsigned long long T0, uint8_t *s_t) {
    const unsigned long long p0 = T0 + (unsigned long long)threadIdx.x * DEC_TPT;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (p0 + DEC_TPT <= n) {
        w = *reinterpret_cast<const uint4 *>(g + p0);
        *reinterpret_cast<uint4 *>(s_t + DEC_HALO + threadIdx.x * DEC_TPT) = w;
    } else {
        for (unsigned long long x = p0; x < n && x < p0 + DEC_TPT; ++x) s_t[DEC_HALO + (x - T0)] = g[x];
    }
    if (threadIdx.x < 2 * DEC_HALO) {
        const bool before = threadIdx.x < DEC_HALO;
        const long long x = before ? (long long)T0 - DEC_HALO + (long long)threadIdx.x : (long long)(T0 + DEC_TILE) + (threadIdx.x - DEC_HALO);
        if (x >= 0 && (unsigned long long)x < n) s_t[x - ((long long)T0 - DEC_HALO)] = g[x];
    }
    __syncthreads();
    return w;
}

// The document of byte p: gdoc[d] <= p < gdoc[d + 1] (d advances from its last value; d = ~0u: not looked up yet).
__device__ __forceinline__ void dec_doc_of(const unsigned long long *gdoc, uint32_t n_docs, unsigned long long p, uint32_t &d) {
    if (d == ~0u) {
        uint32_t lo = 0, hi = n_docs; // last d with gdoc[d] <= p
        while (lo + 1 < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (gdoc[mid] <= p) lo = mid; else hi = mid;
        }
        d = lo;
    }
    while (gdoc[d + 1] <= p) ++d;
}

struct DecCheckParams {
    const uint8_t *g;                 // gathered text
    unsigned long long n;             // its bytes
    const unsigned long long *gdoc;   // n_docs + 1 document offsets into it
    uint32_t n_docs;
    uint32_t *osum;                   // out, per tile: output bytes
    unsigned long long *counters;     // [1] += U+FFFD to write
};

__global__ __launch_bounds__(BLOCK) void k_dec_check(DecCheckParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_t[DEC_TILE + 2 * DEC_HALO];
    __shared__ uint32_t s_o[WPB], s_r[WPB];
    const unsigned long long T0 = (unsigned long long)blockIdx.x * DEC_TILE, p0 = T0 + (unsigned long long)threadIdx.x * DEC_TPT;
    const uint4 w = dec_load_tile(P.g, P.n, T0, s_t);
    uint32_t outb = 0, rep = 0;
    if (p0 < P.n) {
        const unsigned long long p1 = p0 + DEC_TPT < P.n ? p0 + DEC_TPT : P.n;
        if (p1 - p0 == DEC_TPT && !((w.x | w.y | w.z | w.w) & 0x80808080u)) {
            outb = DEC_TPT; // ASCII: every byte is itself
        } else {
            const DecView v{s_t, T0 - DEC_HALO};
            uint32_t d = ~0u;
            for (unsigned long long p = p0; p < p1; ++p) {
                uint32_t ol = 1;
                if (v.T(p) >= 0x80u) {
                    dec_doc_of(P.gdoc, P.n_docs, p, d);
                    ol = dec_out_len(v, p, P.gdoc[d], P.gdoc[d + 1]);
                }
                outb += ol;
                rep += ol == 3u ? 1u : 0u;
            }
        }
    }
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        outb += __shfl_xor(outb, o);
        rep += __shfl_xor(rep, o);
    }
    if (lane == 0) {
        s_o[wib] = outb;
        s_r[wib] = rep;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, r = 0;
        for (int k = 0; k < WPB; ++k) {
            a += s_o[k];
            r += s_r[k];
        }
        P.osum[blockIdx.x] = a;
        if (r) atomicAdd(&P.counters[1], (unsigned long long)r);
    }
}

struct DecRepairParams {
    const uint8_t *g;
    unsigned long long n;
    const unsigned long long *gdoc;
    uint32_t n_docs;
    const unsigned long long *rbase;  // per tile: first output byte ([n_tiles] = total)
    uint8_t *out;
    unsigned long long *rdoc;         // out: n_docs + 1 document offsets into out
    uint32_t *docbad;                 // out: 1 for every document with a U+FFFD (zeroed by the caller)
};

__global__ __launch_bounds__(BLOCK) void k_dec_repair(DecRepairParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_t[DEC_TILE + 2 * DEC_HALO];
    __shared__ unsigned long long s_w[WPB];
    const unsigned long long T0 = (unsigned long long)blockIdx.x * DEC_TILE, p0 = T0 + (unsigned long long)threadIdx.x * DEC_TPT;
    (void)dec_load_tile(P.g, P.n, T0, s_t);
    const DecView v{s_t, T0 - DEC_HALO};
    const unsigned long long p1 = p0 < P.n ? (p0 + DEC_TPT < P.n ? p0 + DEC_TPT : P.n) : p0;
    uint32_t d = ~0u;
    unsigned long long mine = 0;
    for (unsigned long long p = p0; p < p1; ++p) {
        uint32_t ol = 1;
        if (v.T(p) >= 0x80u) {
            dec_doc_of(P.gdoc, P.n_docs, p, d);
            ol = dec_out_len(v, p, P.gdoc[d], P.gdoc[d + 1]);
        }
        mine += ol;
    }
    unsigned long long total;
    unsigned long long o = P.rbase[blockIdx.x] + dec_block_scan(mine, s_w, &total);
    if (p0 >= P.n) return;
    uint32_t dn = 0, hi = P.n_docs; // the first document that starts at or after p0
    while (dn < hi) {
        const uint32_t mid = (dn + hi) >> 1;
        if (P.gdoc[mid] >= p0) hi = mid; else dn = mid + 1;
    }
    d = ~0u; // (the first pass left d at the document of the thread's last byte)
    for (unsigned long long p = p0; p < p1; ++p) {
        while (dn < P.n_docs && P.gdoc[dn] == p) P.rdoc[dn++] = o;
        const uint8_t b = v.T(p);
        uint32_t ol = 1;
        if (b >= 0x80u) {
            dec_doc_of(P.gdoc, P.n_docs, p, d);
            ol = dec_out_len(v, p, P.gdoc[d], P.gdoc[d + 1]);
            if (ol != 1u) P.docbad[d] = 1u;
        }
        dec_emit(b, ol, P.out + o);
        o += ol;
    }
    if (p1 == P.n) { // the last byte's thread: documents that start at the end, and the end itself
        while (dn < P.n_docs && P.gdoc[dn] == p1) P.rdoc[dn++] = o;
        P.rdoc[P.n_docs] = o;
    }
}

} // namespace yb
