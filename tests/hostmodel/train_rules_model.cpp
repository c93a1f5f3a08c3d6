// The training driver's decisions (yet-another-bpe_amd/csrc/train_rules.h) behind a C interface: the functions the host
// calls between launches, with nothing of HIP or the context around them.  Built by tests/test_train_rules_model.py.
#include <stdint.h>

#include "../../yet-another-bpe_amd/csrc/train_rules.h"

using namespace yb;

extern "C" {
int64_t rules_opt_unset() { return OPT_UNSET; }
uint32_t rules_scan_kt_max(uint32_t nw) { return (uint32_t)scan_kt_max((int)nw); }
uint32_t rules_max_lists() { return MAX_LISTS; }

uint32_t rules_count_grid(uint32_t n_tiles, uint32_t n_cu, uint32_t apply_occ, int64_t apply_blocks) { return count_grid_rule(n_tiles, n_cu, apply_occ, apply_blocks); }

// out[9]: nw, chunk, kt, scan_grid, rest, pieces, piece, n_pieces, agg_mask
void rules_sparse_geom(uint32_t n_tiles, uint32_t n_cu, uint64_t best_count, int weighted, uint32_t kmax_now, int64_t full_wpb, int64_t wide_sites_per_cu,
                       int64_t full_skip_blocks, int64_t chunk_steal, int64_t agg_small, uint32_t *out) {
    const SparseGeom g = sparse_geom_rule(n_tiles, n_cu, best_count, weighted != 0, kmax_now, full_wpb, wide_sites_per_cu, full_skip_blocks, chunk_steal, agg_small);
    out[0] = g.nw; out[1] = g.chunk; out[2] = g.kt; out[3] = g.scan_grid; out[4] = g.rest;
    out[5] = g.pieces; out[6] = g.piece; out[7] = g.n_pieces; out[8] = g.agg_mask;
}

int rules_want_sparse(uint32_t n_tiles, int merged_any, int weighted, uint64_t sites, uint64_t best_count, int64_t split_pct) {
    return want_sparse_rule(n_tiles, merged_any != 0, weighted != 0, sites, best_count, split_pct);
}
int rules_sparse_now(int64_t split, int sparse_global) { return sparse_now_rule(split, sparse_global != 0); }

int rules_cand_rebuild(int use_cand, uint32_t i, uint32_t built_at, int64_t every, uint64_t best, uint64_t cand_T, uint64_t prev_best, uint32_t cand_n_all,
                       int64_t cand_target) {
    return cand_rebuild_rule(use_cand != 0, i, built_at, every, best, cand_T, prev_best, cand_n_all, cand_target);
}
int rules_sig_rebuild(int valid, uint32_t i, uint32_t built_at, int64_t every, uint64_t tokens_at_build, uint64_t tokens_now, int64_t pct) {
    return sig_rebuild_rule(valid != 0, i, built_at, every, tokens_at_build, tokens_now, pct);
}

uint32_t rules_xeff_next(const uint32_t *xseen, uint32_t xcap, int64_t headroom_pct, int64_t margin, int64_t granule, int64_t floor) {
    return xeff_next_rule(xseen, xcap, headroom_pct, margin, granule, floor);
}
uint32_t rules_xeff_after_full(uint32_t xeff, uint32_t xcap) { return xeff_after_full_rule(xeff, xcap); }

uint32_t rules_round_launches(int first_round, int sparse_now, uint32_t check) { return round_launches_rule(first_round != 0, sparse_now != 0, check); }
uint32_t rules_round_kmax(int sparse_now, int64_t batch_max) { return round_kmax_rule(sparse_now != 0, batch_max); }
uint32_t rules_round_records(uint32_t num_merges, uint32_t i, uint32_t n_launch, uint32_t kmax) { return round_records_rule(num_merges, i, n_launch, kmax); }
uint32_t rules_rec_first(uint32_t num_merges) { return rec_first_rule(num_merges); }
uint32_t rules_tok_upper(uint32_t tok_upper0, uint32_t launched, uint32_t kmax) { return tok_upper_rule(tok_upper0, launched, kmax); }
uint32_t rules_partials(uint64_t table_cap) { return partials_rule(table_cap); }

int rules_table_grow(uint64_t entries, uint64_t cap, int64_t load_pct) { return table_grow_rule(entries, cap, load_pct); }
uint64_t rules_table_grow_target(uint64_t entries, int64_t grow_x, uint64_t floor) { return table_grow_target_rule(entries, grow_x, floor); }
int rules_retile(uint32_t n_tiles, uint64_t min_tiles, uint64_t live_slots, int64_t retile_pct, int span) { return retile_rule(n_tiles, min_tiles, live_slots, retile_pct, span); }
}
