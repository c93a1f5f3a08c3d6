// train_rules.h -- what the training driver decides between launches, as functions of numbers: the shape of the sparse and
// the streaming launch, when the streaming form gives way to the sparse one, when the candidate list and the signatures are
// rebuilt, how many records the next exchange transmits, how large a round is, when the pair table grows and the stream is
// retiled ("Host drivers").  No HIP, no context, no option lookup: yabpe.hip and yabpe_id32_host.h call
// these with what they read from the context, tests/hostmodel/train_rules_model.cpp with what a test chooses.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "steal_logic.h"

namespace yb {

// launch-shape constants that the rules and the kernels share
constexpr int WPB = 4;               // waves per workgroup
constexpr int BLOCK = WPB * 64;
constexpr int AGG_N = 1024;          // LDS delta-aggregator entries per workgroup
constexpr int KMAX = 16;             // merges one sparse launch applies at most (a batch, see select_batch)
constexpr int scan_kt_max(int nw) { return nw >= 16 ? 2 : 4; } // (a workgroup's hit list lives in LDS: 64 * nw * kt entries)
constexpr uint32_t MAX_APPLY_BLOCKS = 8192;
constexpr uint32_t MAX_LISTS = 2048;  // the sparse launch's scan workgroups at most (blk_read slots)

constexpr int64_t OPT_UNSET = INT64_MIN;  // an option whose default depends on the launch: "not set" travels as this value

// ---------------------------------------------------------------------------------------------- launch shapes
// Streaming form (and every other pass over the tiles with k_apply's workgroups): apply_blocks unset = n_cu * apply_occ.
inline uint32_t count_grid_rule(uint32_t n_tiles, uint32_t n_cu, uint32_t apply_occ, int64_t apply_blocks) {
    const uint32_t want = (n_tiles + WPB - 1) / WPB;
    const uint32_t cap = (uint32_t)(apply_blocks == OPT_UNSET ? (int64_t)n_cu * apply_occ : apply_blocks);
    return std::max(1u, std::min(std::min(want, cap), MAX_APPLY_BLOCKS));
}

// Sparse form.  A grid that is resident all at once (no second round of workgroups behind the first): each thread tests kt
// tiles' signatures per merge, a workgroup owns `chunk` consecutive tiles at a time.  Wide workgroups (full_wpb waves, 16
// waves per CU either way): a merge late in a job has its sites in a few word types, so every workgroup with a site adds to
// the SAME few table counts -- same-address atomics are served one after the other, and the queue is as long as there are
// workgroups; a wider workgroup also evens out how many matched tiles a wave has to rewrite.  (full_wpb <= 0 = by the merge:
// 16 waves once a merge has so few sites that the queue on the hot counts is what is left -- and the whole stream fits one
// round of such workgroups -- else 8.  A 4-wave form existed until round 3: never chosen, pruned.)
struct SparseGeom {
    uint32_t nw;         // waves per workgroup: 8 or 16
    uint32_t chunk, kt;  // tiles a workgroup owns at a time, signature tests per thread
    uint32_t scan_grid;  // workgroups that scan
    uint32_t rest;       // tiles behind the first round of chunks
    uint32_t pieces;     // 1: they go out in pieces through the counter (steal_logic.h), 0: whole chunks by workgroup index
    uint32_t piece, n_pieces;
    uint32_t agg_mask;
};
inline SparseGeom sparse_geom_rule(uint32_t n_tiles, uint32_t n_cu, unsigned long long best_count, bool weighted, uint32_t kmax_now,
                                   int64_t full_wpb, int64_t wide_sites_per_cu, int64_t full_skip_blocks, int64_t chunk_steal, int64_t agg_small) {
    SparseGeom g{};
    if (full_wpb <= 0)
        full_wpb = (best_count <= (unsigned long long)wide_sites_per_cu * n_cu && (n_tiles + 2047u) / 2048u <= n_cu) ? 16 : 8;
    g.nw = full_wpb >= 16 ? 16u : 8u;
    const uint32_t nt = g.nw * 64u;
    const uint32_t target = (uint32_t)std::max<int64_t>(1, full_skip_blocks == OPT_UNSET ? (int64_t)n_cu * (16 / g.nw) : full_skip_blocks);
    // tiles per workgroup: what fills `target` workgroups, in whole waves of signature tests, at most kt_max per thread
    const uint32_t ktm = (uint32_t)scan_kt_max((int)g.nw);
    g.chunk = std::min<uint32_t>(nt * ktm, std::max<uint32_t>(64u, (uint32_t)(((uint64_t)(n_tiles + target - 1) / target + 63u) / 64u * 64u)));
    g.kt = (g.chunk + nt - 1) / nt;
    const uint32_t n_chunks = (n_tiles + g.chunk - 1) / g.chunk;
    g.scan_grid = std::max(1u, std::min<uint32_t>(std::min<uint32_t>(n_chunks, target), MAX_LISTS));
    // a stream of more chunks than workgroups (the early sparse merges: the chunk is capped by the registers of the
    // signature sweep): the tiles behind the first round go out in pieces, to whoever finishes first (steal_logic.h)
    g.rest = n_tiles - (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)g.scan_grid * g.chunk);
    g.pieces = (g.rest && g.nw == 8 && chunk_steal) ? 1u : 0u;  // (the 16-wave form has no counter path: chosen where ONE round covers the stream)
    g.piece = !g.rest ? 0u : g.pieces ? yb_piece_tiles(g.rest, g.scan_grid, g.chunk) : g.chunk;
    g.n_pieces = g.pieces ? yb_piece_count(g.rest, g.piece) : 0u;
    // (a sparse merge leaves a workgroup a few dozen deltas: a quarter of the aggregator per merge of the batch is
    // plenty -- less to initialise and to flush; the count of the LAST batch's merges bounds this batch's)
    g.agg_mask = (uint32_t)AGG_N - 1u;
    if (agg_small && !weighted && best_count * 4 < 48ull * std::max<uint32_t>(1u, n_cu * 3))
        g.agg_mask = (uint32_t)(kmax_now > 2 ? AGG_N : g.nw >= 16 ? AGG_N / 2 : AGG_N / 4) - 1u;
    return g;
}

// ---------------------------------------------------------------------------------------------- form
// Does a shard call for the sparse form?  Sites per merge never increase (the best count is monotone): once they are sparse
// relative to the number of tiles.  Pooled words: the count is weighted, what matters is how many resident sites the last
// merge had.
inline bool want_sparse_rule(uint32_t n_tiles, bool merged_any, bool weighted, unsigned long long sites, unsigned long long best_count, int64_t split_pct) {
    return n_tiles && merged_any && (weighted && sites ? sites : best_count) * 100 < (unsigned long long)n_tiles * (unsigned long long)split_pct;
}
// option split: -1 by want_sparse_rule (for good, and for all ranks), 0 never, 1 always
inline bool sparse_now_rule(int64_t split, bool sparse_global) { return split >= 0 ? split == 1 : sparse_global; }

// ---------------------------------------------------------------------------------------------- upkeep
// The candidate list stays exact for as long as the maximum stays >= its threshold T (slots that rise are appended by the
// argmax itself), so it is rebuilt -- a scan of the whole table -- only now and then: when there is none (start, table
// rebuilt or grown, fallback), every `every` merges to keep it short, before the maximum can reach T within the next two
// batches at the pace of the last one (a fallback costs the rest of a batch; early in a run the best count falls fast, so
// the list is rebuilt every batch there, late in the run hardly ever), and when it has grown long (appended slots): the
// fused selection is one workgroup reading all of it, 4 entries per thread in one pass.
// (multi-GPU: cand_n_all is the longest replica's length -- every rank must rebuild at the same merges.)
inline bool cand_rebuild_rule(bool use_cand, uint32_t i, uint32_t built_at, int64_t cand_rebuild_every, unsigned long long best,
                              unsigned long long cand_T, unsigned long long prev_best, uint32_t cand_n_all, int64_t cand_target) {
    const uint32_t every = (uint32_t)std::max<int64_t>(1, cand_rebuild_every);
    const unsigned long long drop = prev_best > best ? prev_best - best : 0;
    const bool near_T = best < cand_T + 2 * drop + 1;
    const bool long_list = cand_n_all > std::max<uint32_t>(4u * BLOCK - 64u, (uint32_t)cand_target);
    return !use_cand || i - built_at >= every || i < built_at || near_T || long_list;
}
// Signatures are built when the sparse form starts and refreshed now and then: rewrites only ever ADD bits (every merged
// site leaves up to two new pairs and three stale ones behind), so the stale share grows with the sites merged since.
inline bool sig_rebuild_rule(bool valid, uint32_t i, uint32_t built_at, int64_t sig_rebuild_every, uint64_t tokens_at_build, uint64_t tokens_now,
                             int64_t sig_rebuild_pct) {
    const uint32_t every = (uint32_t)std::max<int64_t>(1, sig_rebuild_every);
    const uint64_t merged_since = tokens_at_build > tokens_now ? tokens_at_build - tokens_now : 0;
    const bool stale = merged_since * 100 > tokens_at_build * (uint64_t)sig_rebuild_pct;
    return !valid || i - built_at >= every || i < built_at || stale;
}

// ---------------------------------------------------------------------------------------------- exchange
// Records per rank the next exchanges transmit: an overflow costs a recount of the whole stream, so (headroom: twice) the
// largest count of the last four rounds plus a margin, in whole granules, never less than the floor, never more than the
// buffers hold.
inline uint32_t xeff_next_rule(const uint32_t xseen[4], uint32_t xcap, int64_t delta_headroom_pct, int64_t delta_margin, int64_t delta_granule,
                               int64_t delta_floor) {
    const uint64_t recent = std::max(std::max(xseen[0], xseen[1]), std::max(xseen[2], xseen[3]));
    const uint64_t gran = (uint64_t)std::max<int64_t>(1, delta_granule);
    const uint64_t raw = recent * (uint64_t)std::max<int64_t>(1, delta_headroom_pct) / 100ull + (uint64_t)std::max<int64_t>(0, delta_margin);
    const uint64_t want = ((raw + gran - 1) / gran) * gran;
    return (uint32_t)std::min<uint64_t>(xcap, std::max<uint64_t>(want, std::min<uint64_t>((uint64_t)std::max<int64_t>(1, delta_floor), xcap)));
}
// after HALT_DELTA_FULL (a merge produced more records on some rank than an exchange transmits): 4x for everybody while
// the buffers hold it; at xeff == xcap the caller grows the buffers instead
inline uint32_t xeff_after_full_rule(uint32_t xeff, uint32_t xcap) { return (uint32_t)std::min<uint64_t>(xcap, 4ull * xeff); }

// ---------------------------------------------------------------------------------------------- rounds
// launches between two looks at the device state (the same on every rank: a launch is an exchange)
inline uint32_t round_launches_rule(bool first_round, bool sparse_now, uint32_t check) { return (first_round && !sparse_now) ? std::min<uint32_t>(check, 8) : check; }
// merges one selection may take: a batch in the sparse form, one in the streaming form (DESIGN (c))
inline uint32_t round_kmax_rule(bool sparse_now, int64_t batch_max) { return sparse_now ? (uint32_t)std::max<int64_t>(1, std::min<int64_t>(KMAX, batch_max)) : 1u; }
// records for everything the launches of a round can select
inline uint32_t round_records_rule(uint32_t num_merges, uint32_t i, uint32_t n_launch, uint32_t kmax) {
    return (uint32_t)std::min<uint64_t>(num_merges, (uint64_t)i + (uint64_t)(n_launch + 2) * kmax);
}
// records a u16 call starts with: it cannot run more merges than it has ids for plus the (rare) merges that reuse one
inline uint32_t rec_first_rule(uint32_t num_merges) { return (uint32_t)std::min<uint64_t>(num_merges, (uint64_t)YB_MAX_TOKENS + 4096); }
// token ids that can exist when the launched-th launch of a round runs
inline uint32_t tok_upper_rule(uint32_t tok_upper0, uint32_t launched, uint32_t kmax) { return tok_upper0 + (launched + 1u) * kmax + 1u; }
// workgroups of the argmax over the whole table
inline uint32_t partials_rule(uint64_t table_cap) { return (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, table_cap / (BLOCK * 8))); }

// ---------------------------------------------------------------------------------------------- housekeeping
// The table is kept at 12-30 % load: a key that is not at its home slot costs the flush of every merge a dependent trip (the
// 1 GiB job: 1.60 s at 50-70 % load, 1.42 s at 12-30 %), and the table is scanned only now and then.
inline bool table_grow_rule(uint64_t entries, uint64_t cap, int64_t table_load_pct) { return entries * 100 > cap * (uint64_t)table_load_pct; }
// (u16 loop: grow_x = option table_grow_x, floor 2^16; u32 loop: 4, floor 1024)
inline uint64_t table_grow_target_rule(uint64_t entries, int64_t grow_x, uint64_t floor) { return std::max<uint64_t>(entries * (uint64_t)std::max<int64_t>(2, grow_x), floor); }
// retile when the live slots fill less than retile_pct of the tiles (span: packed positions a tile owns when retiled)
inline bool retile_rule(uint32_t n_tiles, uint64_t retile_min_tiles, uint64_t live_slots, int64_t retile_pct, int span) {
    const double retile_frac = (double)retile_pct / 100.0;
    return n_tiles >= retile_min_tiles && (double)live_slots < retile_frac * (double)n_tiles * span;
}

}  // namespace yb
