"""GPU: the tile-centric loader (load_form 1, k_load_tiles) against the one-thread-per-word loader (load_form 0, k_load_words):
the resident stream read back with yabpe_stream_dump must be identical -- every slot of every tile, tile_len, tile_wbase --
and so must the long-word side (count, tokens, content through the checksum), in the flat layout and with frequencies, on
the cases of tests/load_cases.py; then 300 merges on a random-words corpus with verify=1 against the C reference
implementation under both forms."""
from __future__ import annotations

import numpy as np
import pytest

from tests import helpers, load_cases

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]


def loaded(form: int, flat, off, freq):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        ctx.set_option("load_form", form)
        ctx.set_vocab(helpers.base_tokens(SP))
        ctx.load_words(flat, off, freq)
        d = ctx.stream_dump()
        d["checksum"] = ctx.stream_checksum()
        d["n_long_words"] = ctx.stats()["n_long_words"]
    return d


@pytest.mark.parametrize("weighted", [False, True], ids=["flat", "freq"])
@pytest.mark.parametrize("name", list(load_cases.cases()))
def test_dumps_are_equal(name, weighted):
    lens, off_base = load_cases.cases()[name]
    flat, off = load_cases.build(lens, off_base)
    freq = (np.arange(len(lens), dtype=np.uint64) % 5 + 1) if weighted else None
    a, b = loaded(0, flat, off, freq), loaded(1, flat, off, freq)
    assert a["n_tiles"] == b["n_tiles"] == (int(off[-1] - off[0]) + len(lens) + load_cases.SPAN - 1) // load_cases.SPAN
    assert np.array_equal(a["tile_len"], b["tile_len"])
    assert np.array_equal(a["tiles"], b["tiles"])
    assert (a["tile_wbase"] is None) == (b["tile_wbase"] is None) == (not weighted)
    if weighted:
        assert np.array_equal(a["tile_wbase"], b["tile_wbase"])
    assert a["checksum"] == b["checksum"] and a["n_long_words"] == b["n_long_words"]
    assert a["n_long_words"] == sum(1 for L in lens if L >= load_cases.LMAX)
    if name == "longer_than_a_span":
        assert b["tile_len"][1] == 0 and (b["tiles"][1] == 0xFFFE).all()
    if name == "starts_on_slot_span_minus_1":
        assert b["tile_len"][0] == load_cases.CAP


@pytest.fixture(scope="module")
def random_words():
    from oracle import oracle
    from yet_another_bpe import synth

    flat, off = synth.generate(synth.SynthSpec(256 << 10, 5_000, 11, b"abcdefghijklmnopqrstuvwxyz", True))  # ~300 tiles
    base = helpers.base_tokens(SP)
    return flat, off, base, oracle.train_flat(flat, off, len(base) + 300, 1, SP)


@pytest.mark.parametrize("form", [0, 1])
def test_training_after_either_loader_matches_reference(random_words, form):
    from yet_another_bpe import _native

    flat, off, base, (exp_vocab, exp_merges) = random_words
    vocab, merges = _native.train_words(flat, off, None, base, 300, 1, options={"verify": 1, "load_form": form})
    assert merges == exp_merges and vocab == exp_vocab
