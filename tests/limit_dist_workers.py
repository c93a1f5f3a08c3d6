"""Worker for the multi-rank test of the maximum token length (spawned by tests/dist_workers.spawn: gloo on 127.0.0.1, the
ranks share one GPU and exchange through the custom transport)."""
from __future__ import annotations


def gpu_sharded_limit(rank, world, dist, limit, num_merges, min_frequency):
    """The 6,000 pre-tokens of tests/limit_helpers.py, flat layout, word-sharded over the ranks, with max_token_bytes = limit on
    every rank.  -> (merges as hex pairs, words this rank held)"""
    from tests import helpers, limit_helpers as lh
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import train_sharded

    base = helpers.base_tokens(lh.SP)
    flat, off = helpers.flatten(list(lh.en_words()))
    left, right, merged, _count, stats = train_sharded(lambda: _native.Context(0), flat, off, None, base, num_merges, min_frequency, rank, world,
                                                       transport="torch", options={"verify": 1, "max_token_bytes": limit})
    toks = list(base)
    out = []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        out.append((toks[l].hex(), toks[r].hex()))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
    return out, int(stats["n_words"])
