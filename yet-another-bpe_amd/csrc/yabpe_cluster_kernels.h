// yabpe_cluster_kernels.h -- near-duplicate clusters from MinHash signatures and LSH band keys (rule in cluster_logic.h;
// contract: BBPETokenizer.minhash_clusters, yet_another_bpe/tokenizer.py).  Host orchestration: yabpe_minhash_cluster in yabpe.hip.
//
//   k_cluster_preset   one thread per slot / document: slots CL_EMPTY, anchors 0xFFFFFFFF, parent[d] = d, the counters 0.
//   k_cluster_insert   one thread per entry e = d * B + t.  The thread of a participating document probes from the entry's home
//                      slot, claims the first free slot with atomicCAS(CL_EMPTY -> e) or stops at a slot whose resident entry is
//                      of the same band and carries the same key -- read from keys[], the call's immutable input, so no thread
//                      ever waits for another one's store and no key value is reserved.  A slot is claimed once and for good:
//                      every entry of a bucket walks the same chain and ends in the same slot.  It lowers anchor[slot] to d
//                      (a read first: when d is not smaller the atomic is skipped -- the all-identical corpus is B hot
//                      addresses under n writers) and leaves its slot in slot_of[e].
//   k_cluster_link     in a launch of its own, once every anchor is final: one WAVE per participating document, four a
//                      workgroup.  The lanes read the anchors of the document's bands, 64 a round; a ballot of anchor != d
//                      sends the document without a candidate home after those B loads.  Else the distinct anchors are
//                      gathered in the wave's LDS list (duplicates dropped by lane comparison inside a round, against the list
//                      across rounds).  With min_agree > 0 the document's row then goes into registers once, coalesced (lane l
//                      holds k = l, l + 64, ...: at most 16 values), every distinct anchor's row is streamed the same way, the
//                      per-lane equality counts meet in one wave reduction.  Lane 0 unites accepted edges in a lock-free
//                      union-find: walk both ends to their roots (path halving), hook the LARGER root under the smaller with
//                      atomicCAS on parent[], go on from what the CAS found when it fails.  parent[x] <= x always, so a root is
//                      the minimum of its tree and the labelling does not depend on the order the waves arrive in.
//   k_cluster_flatten  in a launch of its own: one thread per document walks parent[] (read only) to the root, writes it to
//                      cluster[] and counts the roots, one atomicAdd a wave.
//
// Equality counts, minima and compare-and-swap have no matrix instruction on gfx950 (MFMA multiplies and sums): VALU and atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cluster_logic.h"

namespace yb {

constexpr uint32_t CL_WAVES = BLOCK / 64;              // documents of one workgroup of k_cluster_link
constexpr uint32_t CL_ROW_REGS = MH_MAX_PERM / 64;     // signature values a lane holds
enum { CL_C_PARTICIPATING, CL_C_CANDIDATES, CL_C_ACCEPTED, CL_C_CLUSTERS, CL_COUNTERS };

struct ClusterParams {
    const uint32_t *sig;                  // [n_docs][num_perm], or nullptr with min_agree == 0
    const unsigned long long *keys;       // [n_docs][bands]
    const unsigned long long *shingles;   // [n_docs], or nullptr: every document takes part
    uint32_t n_docs;
    ClusterRule rule;
    uint32_t slots_log2;
    uint32_t *table;                      // [slots] entry indices
    uint32_t *anchor;                     // [slots] the smallest document of the slot's bucket
    uint32_t *slot_of;                    // [n_docs * bands] (written for participating documents only)
    uint32_t *parent;                     // [n_docs]
    uint32_t *cluster;                    // [n_docs] the result
    uint32_t *counters;                   // [CL_COUNTERS]
};

__device__ __forceinline__ bool cl_takes_part(const ClusterParams &P, uint32_t d) { return !P.shingles || P.shingles[d] > 0; }
__device__ __forceinline__ uint32_t cl_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t cl_lane() { return threadIdx.x & 63u; }
// adds the number of lanes with `pred` to *ctr, one atomic a wave (every lane of the wave calls this)
__device__ __forceinline__ void cl_count(uint32_t *ctr, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m && cl_lane() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(ctr, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(BLOCK) void k_cluster_preset(ClusterParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i < (1ull << P.slots_log2)) {
        P.table[i] = CL_EMPTY;
        P.anchor[i] = CL_EMPTY;
    }
    if (i < P.n_docs) P.parent[i] = (uint32_t)i;
    if (i < CL_COUNTERS) P.counters[i] = 0;
}

__global__ __launch_bounds__(BLOCK) void k_cluster_insert(ClusterParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t B = P.rule.bands;
    const bool in = i < (unsigned long long)P.n_docs * B;
    const uint32_t e = (uint32_t)i, d = in ? e / B : 0u, t = e - d * B;
    const bool part = in && cl_takes_part(P, d);
    cl_count(&P.counters[CL_C_PARTICIPATING], part && t == 0);
    if (!part) return;
    const unsigned long long key = P.keys[e];
    const uint32_t n_slots = 1u << P.slots_log2, mask = n_slots - 1;
    uint32_t slot = cl_home(key, t, P.slots_log2), found = CL_EMPTY;
    for (uint32_t probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask) {
        uint32_t r = cl_load(&P.table[slot]);
        if (r == CL_EMPTY) {
            r = atomicCAS(&P.table[slot], CL_EMPTY, e);
            if (r == CL_EMPTY) r = e;  // claimed
        }
        if (r == e || (r % B == t && P.keys[r] == key)) {
            found = slot;
            break;
        }
    }
    // (found stays CL_EMPTY only in a table without a free slot, which yabpe_minhash_cluster refuses: k_cluster_link skips it)
    if (found != CL_EMPTY && cl_load(&P.anchor[found]) > d) atomicMin(&P.anchor[found], d);
    P.slot_of[e] = found;
}

// the root of x, halving the path on the way: parent[x] only ever moves to an ancestor of x, by anybody's store
__device__ __forceinline__ uint32_t cl_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cl_load(&parent[x]);
        if (p == x) return x;
        const uint32_t g = cl_load(&parent[p]);
        if (g != p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// Both ends strictly fall on every turn that does not return (a failed CAS hands back a smaller parent), so the loop ends.
__device__ __forceinline__ void cl_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t x = a;
            a = b;
            b = x;
        }
        const uint32_t old = atomicCAS(&parent[a], a, b);  // the larger root under the smaller
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(BLOCK) void k_cluster_link(ClusterParams P) {
    __shared__ uint32_t s_list[CL_WAVES][CL_MAX_BANDS];
    const uint32_t lane = cl_lane(), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t d = blockIdx.x * CL_WAVES + wave;
    if (d >= P.n_docs || !cl_takes_part(P, d)) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const uint32_t B = P.rule.bands, K = P.rule.num_perm, m = P.rule.min_agree;
    uint32_t *list = s_list[wave];
    uint32_t n_list = 0;
    for (uint32_t t0 = 0; t0 < B; t0 += 64) {
        const uint32_t t = t0 + lane;
        uint32_t a = CL_EMPTY;
        if (t < B) {
            const uint32_t slot = P.slot_of[(unsigned long long)d * B + t];
            if (slot != CL_EMPTY) a = P.anchor[slot];
            if (a >= d) a = CL_EMPTY;  // (its own bucket's anchor is d at most: d lowered it)
        }
        const unsigned long long has = __ballot(a != CL_EMPTY);
        if (!has) continue;
        bool keep = a != CL_EMPTY;
        for (unsigned long long todo = has; todo; todo &= todo - 1ull) {  // a lower lane with the same anchor
            const uint32_t j = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t aj = (uint32_t)__builtin_amdgcn_readlane((int)a, (int)j);
            if (lane > j && a == aj) keep = false;
        }
        for (uint32_t j = 0; j < n_list; ++j)  // an earlier round's (one LDS address for the whole wave: a broadcast)
            if (list[j] == a) keep = false;
        const unsigned long long km = __ballot(keep);
        if (keep) list[n_list + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))] = a;  // (n_list <= t0 before, <= B after)
        n_list += (uint32_t)__popcll(km);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (!n_list) return;
    uint32_t mine[CL_ROW_REGS];
    if (m) {
        const uint32_t *row = P.sig + (unsigned long long)d * K;
#pragma unroll
        for (uint32_t i = 0; i < CL_ROW_REGS; ++i) {
            const uint32_t k = i * 64 + lane;
            mine[i] = k < K ? row[k] : 0u;
        }
    }
    uint32_t n_acc = 0;
    for (uint32_t j = 0; j < n_list; ++j) {
        const uint32_t a = list[j];
        bool ok = true;
        if (m) {
            const uint32_t *row = P.sig + (unsigned long long)a * K;
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t i = 0; i < CL_ROW_REGS; ++i) {
                const uint32_t k = i * 64 + lane;
                if (i * 64 < K) cnt += k < K && row[k] == mine[i];
            }
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            ok = cnt >= m;
        }
        if (ok) {
            ++n_acc;
            if (lane == 0) cl_unite(P.parent, d, a);
        }
    }
    if (lane == 0) {
        atomicAdd(&P.counters[CL_C_CANDIDATES], n_list);
        if (n_acc) atomicAdd(&P.counters[CL_C_ACCEPTED], n_acc);
    }
}

__global__ __launch_bounds__(BLOCK) void k_cluster_flatten(ClusterParams P) {
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = d < P.n_docs;
    uint32_t x = d;
    if (in) {
        for (uint32_t p; (p = P.parent[x]) != x;) x = p;  // (parent[x] < x on the way: it ends)
        P.cluster[d] = x;
    }
    cl_count(&P.counters[CL_C_CLUSTERS], in && x == d);
}

}  // namespace yb
