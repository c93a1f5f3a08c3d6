"""GPU (-m gpu; the first test holds the premises on the oracle and needs none): a second load on one context -- what the
load driver's steps (csrc/yabpe.hip, csrc/yabpe_id32_host.h) give up, reset and start over.  Job 1 loads corpus A and learns 40 merges; job 2 loads corpus B -- A's words in
another order, one word less -- on the SAME context and trains to N_MERGES; job 3 is job 2 on a fresh context.  Jobs 2 and 3
must both give the oracle's model of B bit for bit (ids and counts of every merge, the vocabulary), and every integer field of
yabpe_stats_t (and of yabpe_resume_stats_t after a resumed load) must be equal between them: nothing of job 1 is left.

Both id widths, verify = 1 everywhere.  For u16 one case per loader (k_load_tiles: load_form 1, k_load_words: load_form 0,
k_load_words_tok: the resumed load), each after a job 1 that used another loader and the other layout where there is one.
A resumed job 2 replays the 40 merges job 1 learned; B is chosen so that they are B's first 40 as well (asserted on the
oracle), which makes the oracle's model of B the expectation there too.

Corpora: `stems` with its three long words and the 200 KiB `en` words of tests/test_gpu_train_driver.py."""
from __future__ import annotations

import random
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle
from tests import helpers, resume_helpers as rh
from tests.test_gpu_batch_ties import assert_equals
from tests.test_gpu_train_driver import N_MERGES, SP, words

FIRST = 40  # merges of job 1
FIELDS = ("left", "right", "merged", "count")


@lru_cache(maxsize=None)
def corpus(name: str, which: str) -> tuple[bytes, ...]:
    """A: the words of the training-driver tests.  B: the same in a seeded other order, one occurrence of A's first word
    dropped (a short word that A holds more than once: the first merges stay the same, the test below holds that)."""
    if which == "A":
        return words(name)
    ws = list(words(name))
    del ws[0]
    random.Random(5).shuffle(ws)
    return tuple(ws)


@lru_cache(maxsize=None)
def inputs(name: str, which: str, layout: str):
    ws = corpus(name, which)
    if layout == "weighted":
        uw, fq = helpers.pooled(ws)
        return (*helpers.flatten(uw), fq)
    return (*helpers.flatten(list(ws)), None)


@lru_cache(maxsize=None)
def expected(name: str, which: str):
    """The oracle's model of a corpus, computed once, read-only afterwards."""
    flat, off, fq = inputs(name, which, "weighted")
    vocab, merges, ids = oracle.train_flat(flat, off, len(helpers.base_tokens(SP)) + N_MERGES[name], 1, SP, return_ids=True, freq=fq)
    for a in ids.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, merges, ids


@pytest.mark.parametrize("name", ["stems", "en"])
def test_corpus_b_differs_and_keeps_the_first_merges(name):
    """(No GPU work: the premises of the cases below, on the oracle.)"""
    a, b = corpus(name, "A"), corpus(name, "B")
    assert len(b) == len(a) - 1 and list(b) != list(a[:len(b)]) and sorted(set(b)) != sorted(b)
    assert expected(name, "A")[1][:FIRST] == expected(name, "B")[1][:FIRST]
    assert all(np.array_equal(expected(name, "A")[2][f][:FIRST], expected(name, "B")[2][f][:FIRST]) for f in FIELDS[:3])
    assert not np.array_equal(expected(name, "A")[2]["count"], expected(name, "B")[2]["count"])  # B's counts are its own


def load(ctx, name, which, loader, model):
    """One job's vocabulary and load.  loader: ("tiles" | "words", layout) -- the byte loads in load_form 1 | 0 -- or
    ("resumed", "weighted"): `model` = (tokens, triples) of the merges to replay."""
    kind, layout = loader
    flat, off, fq = inputs(name, which, layout)
    if kind == "resumed":
        toks, triples = model
        ctx.set_vocab(toks)
        ctx.load_words_resumed(flat, off, fq, triples)
    else:
        ctx.set_option("load_form", 1 if kind == "tiles" else 0)
        ctx.set_vocab(helpers.base_tokens(SP))
        ctx.load_words(flat, off, fq)


def context(id_bits: int):
    from yet_another_bpe import _native

    ctx = _native.Context(0)
    ctx.set_option("verify", 1)
    ctx.set_option("id_bits", id_bits)
    return ctx


def integers(stats: dict) -> dict:
    out = {k: v for k, v in stats.items() if not k.endswith("_ms") and not k.endswith("_ms_sampled")}
    assert all(isinstance(v, int) for v in out.values()) and len(out) < len(stats), stats
    return out


def job_b(ctx, name, loader_b, model):
    """Job 2 / job 3: B loaded and trained to N_MERGES -> (the whole model's id arrays, stats, resume stats)."""
    load(ctx, name, "B", loader_b, model)
    assert ctx.verify_table() == 0
    replayed = FIRST if loader_b[0] == "resumed" else 0
    got = ctx.train(N_MERGES[name] - replayed, 1)
    # (a resumed job returns the merges it learned: in front of them the oracle's first 40, which job 1 was held against)
    whole = tuple(np.concatenate([expected(name, "B")[2][f][:replayed], g]) for f, g in zip(FIELDS, got))
    return whole, integers(ctx.stats()), integers(ctx.resume_stats())


def second_load(name: str, id_bits: int, loader_a, loader_b):
    from yet_another_bpe import _native

    what = (name, id_bits, loader_a, loader_b)
    base = helpers.base_tokens(SP)
    with context(id_bits) as ctx:
        load(ctx, name, "A", loader_a, None)
        first = ctx.train(FIRST, 1)
        assert_equals(first, expected(name, "A"), SP, upto=FIRST, what=what)
        model = _native.merge_triples(base, _native.decode_merges(base, *first[:3])[1])
        same, st_same, rs_same = job_b(ctx, name, loader_b, model)
    with context(id_bits) as ctx:
        fresh, st_fresh, rs_fresh = job_b(ctx, name, loader_b, model)
    print(what, st_fresh, rs_fresh)
    assert_equals(fresh, expected(name, "B"), SP, what=(what, "fresh context"))
    assert_equals(same, expected(name, "B"), SP, what=(what, "same context"))
    assert st_fresh["merges_done"] == N_MERGES[name] - (FIRST if loader_b[0] == "resumed" else 0)
    assert st_fresh["n_words_input"] == len(inputs(name, "B", loader_b[1])[1]) - 1
    assert st_same == st_fresh, (what, {k: (st_same[k], st_fresh[k]) for k in st_same if st_same[k] != st_fresh[k]})
    if loader_b[0] == "resumed" or id_bits == 32:  # (the u16 byte loads leave resume_stats alone)
        assert rs_same == rs_fresh and rs_fresh["tokens"] == st_fresh["tokens_initial"] > 0, (what, rs_same, rs_fresh)
        assert rs_fresh["n_unique"] == st_fresh["n_words"] and rs_fresh["n_long"] == st_fresh["n_long_words"], (what, rs_fresh)
    return st_fresh


def long_words(name: str, loader_b) -> int:
    """Words of B that take the long-word path: 64 tokens and more -- bytes, or what the replay of the first merges leaves."""
    kind, layout = loader_b
    ws = helpers.pooled(corpus(name, "B"))[0] if layout == "weighted" else corpus(name, "B")
    merges = expected(name, "B")[1][:FIRST] if kind == "resumed" else []
    return sum(len(rh.literal_replay(w, merges)) >= 64 for w in ws if len(w) >= 64)


U16_CASES = [(("tiles", "flat"), ("words", "weighted")), (("words", "weighted"), ("tiles", "flat")), (("tiles", "weighted"), ("resumed", "weighted")),
             (("words", "flat"), ("resumed", "weighted"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stems", "en"])
@pytest.mark.parametrize("loader_a,loader_b", U16_CASES, ids=lambda x: "-".join(x))
def test_second_load_u16(name, loader_a, loader_b):
    assert second_load(name, 16, loader_a, loader_b)["n_long_words"] == long_words(name, loader_b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stems", "en"])
@pytest.mark.parametrize("loader_a,loader_b", [(("tiles", "weighted"), ("tiles", "flat")), (("tiles", "flat"), ("resumed", "weighted"))], ids=lambda x: "-".join(x))
def test_second_load_u32(name, loader_a, loader_b):
    assert second_load(name, 32, loader_a, loader_b)["n_long_words"] == long_words(name, loader_b)
