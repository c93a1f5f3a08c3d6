// cluster_logic.h -- the near-duplicate clustering rule (BBPETokenizer.minhash_clusters, yet_another_bpe/tokenizer.py), host-
// and device-callable: yabpe_cluster_kernels.h and yabpe_minhash_cluster (yabpe.hip) call the same functions.
//
// Inputs sig u32[n][K], keys u64[n][B], optionally n_shingles u64[n]; min_agree in [0, K].  All of it integer:
//   takes part  document d iff n_shingles is absent or n_shingles[d] > 0; one that does not is its own cluster.
//   bucket      (t, v): the participating documents with keys[d][t] == v (64 bits, the same band t).  Its anchor is its
//               smallest document index.
//   candidate   (d, anchor) for every d of a bucket other than the anchor; a pair that several bands give is one candidate.
//   accepted    iff #{k : sig[d][k] == sig[anchor][k]} >= min_agree (min_agree 0: everything, sig is never read).
//   cluster[d]  the smallest document index of d's connected component under the accepted edges.
// The table of the device: open addressing, linear probing, a power of two of slots; a slot holds the ENTRY index
// e = d * B + t of whoever claimed it, CL_EMPTY before.  The home slot of an entry is the high bits of mix(key + G * (t + 1)).
#pragma once
#include <stdint.h>

#include "minhash_logic.h"

constexpr uint32_t CL_EMPTY = 0xFFFFFFFFu;               // a free slot; an anchor nobody has lowered; "no candidate"
constexpr uint32_t CL_MAX_BANDS = 1024;                  // the link wave's list of distinct anchors holds one per band
constexpr unsigned long long CL_MAX_ENTRIES = 1ull << 30;  // n_docs * bands: entry indices and slots stay below 2^32
constexpr uint32_t CL_MIN_SLOTS_LOG2 = 10, CL_MAX_SLOTS_LOG2 = 31;

struct ClusterRule {
    uint32_t num_perm, bands, min_agree;
};

// the rule's argument checks (yabpe_minhash_cluster and BBPETokenizer._cluster_args refuse the same things)
YB_HD bool cl_rule_valid(const ClusterRule &R) {
    return R.num_perm >= 1 && R.num_perm <= MH_MAX_PERM && R.bands >= 1 && R.bands <= CL_MAX_BANDS && R.min_agree <= R.num_perm;
}

// auto size: the smallest power of two >= 2 x entries, at least 2^10 (entries <= 2^30: at most 2^31 slots)
YB_HD uint32_t cl_slots_log2(unsigned long long entries) {
    uint32_t lg = CL_MIN_SLOTS_LOG2;
    while ((1ull << lg) < 2 * entries) ++lg;
    return lg;
}

YB_HD uint32_t cl_home(unsigned long long key, uint32_t band, uint32_t slots_log2) {
    return (uint32_t)(enc_mix(key + ENC_RND_G * ((unsigned long long)band + 1)) >> (64 - slots_log2));
}
