"""GPU: the gathering retile (retile_form 1, k_retile_gather: new tiles written whole from images in LDS) against the scatter
form (retile_form 0: fill, then k_retile<true> element by element).  With retiles forced early and often, both forms give
the reference implementation's merges, ids and counts, at least one retile happens, and the streams read back at the end
with yabpe_stream_dump are identical -- tiles, tile_len and, in the sparse form, every signature row; also on a corpus where
whole tiles die at the first merge (kept == 0 tiles, one new tile left)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]
OPTS = {"retile_pct": 95, "retile_min_tiles": 16, "check_interval": 7, "verify": 1}
MERGES = 400


def corpus(kind: str):
    if kind == "random_words":
        from yet_another_bpe import synth

        return synth.generate(synth.SynthSpec(256 << 10, 5_000, 11, b"abcdefghijklmnopqrstuvwxyz", True))  # ~300 tiles
    # whole tiles die: ~19 tiles of words that are exactly the first merge's pair, then a few words that live on
    words = [b"ab"] * 6000 + [b"cdcdc", b"dcdcdd", b"ccd", b"xyzxyzxy", b"zyxzyx"] * 20
    return helpers.flatten(words)


@pytest.fixture(scope="module", params=["random_words", "tiles_die"])
def case(request):
    from oracle import oracle

    flat, off = corpus(request.param)
    base = helpers.base_tokens(SP)
    _vocab, _merges, ids = oracle.train_flat(flat, off, len(base) + MERGES, 1, SP, return_ids=True)
    return request.param, flat, off, base, ids


def run(flat, off, base, form: int, split: int):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for k, v in {**OPTS, "retile_form": form, "split": split}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(base)
        ctx.load_words(flat, off)
        left, right, merged, count = ctx.train(MERGES, 1)
        return {"left": left, "right": right, "merged": merged, "count": count, "retiles": ctx.stats()["retiles"], "dump": ctx.stream_dump()}


@pytest.mark.parametrize("split", [-1, 1])
def test_forms_agree_and_match_reference(case, split):
    kind, flat, off, base, ids = case
    a, b = run(flat, off, base, 0, split), run(flat, off, base, 1, split)
    for r in (a, b):
        assert r["retiles"] >= 1
        for k in ("left", "right", "merged", "count"):
            assert np.array_equal(r[k], ids[k]), k
    da, db = a["dump"], b["dump"]
    assert da["n_tiles"] == db["n_tiles"] >= 1
    assert np.array_equal(da["tile_len"], db["tile_len"])
    assert np.array_equal(da["tiles"], db["tiles"])
    assert (da["sig"] is None) == (db["sig"] is None)
    if split == 1:
        assert db["sig"] is not None
    if db["sig"] is not None:
        assert np.array_equal(da["sig"], db["sig"])
    if kind == "tiles_die":
        assert len(ids["left"]) < MERGES and db["n_tiles"] == 1  # (the 19 tiles of "ab" words are gone)
