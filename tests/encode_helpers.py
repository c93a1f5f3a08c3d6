"""Shared by the encoder tests: the G9 tokenizer set-ups (as tests/test_tokenizer_golden.py builds them) and random
tie-heavy models."""
from __future__ import annotations

import json
import random
from pathlib import Path

from oracle import oracle
from tests import helpers
from yet_another_bpe.tokenizer import BBPETokenizer
from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig


def _trainer(name: str, golden_dir: Path) -> BBPETrainer:
    if name == "corpus_en_1000":
        t = BBPETrainer(BBPETrainerConfig(vocab_size=1000, min_frequency=1, max_workers=1, special_tokens=["<|endoftext|>"]))
        t._vocab = {bytes.fromhex(k): v for k, v in json.loads((golden_dir / "g1_corpus_en_vocab_1000.json").read_text()).items()}
        t._merges = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")[:743]
        return t
    cfg = BBPETrainerConfig(vocab_size=300, min_frequency=1, max_workers=1)
    t = BBPETrainer(cfg)
    words = [bytes(s) for s in t._preprocess_corpus([golden_dir / "data" / "sample.txt"])]
    t._vocab, t._merges = oracle.merge_loop(words, 300, 1, list(cfg.special_tokens))
    return t


def g9_setups(golden_dir: Path, tmp_path: Path):
    """-> [(model index, set-up name, tokenizer)] for every set-up G9 pins."""
    g9 = json.loads((golden_dir / "g9_tokenizer.json").read_text())
    out = []
    for idx, m in enumerate(g9["models"]):
        t = _trainer(m["name"], golden_dir)
        t.save(tmp_path / f"model{idx}")
        toks = {"from_file": BBPETokenizer.from_file(tmp_path / f"model{idx}"),
                "in_memory": BBPETokenizer(vocab=dict(t._vocab), merges=list(t._merges), special_tokens=list(t.config.special_tokens))}
        if m["name"] == "corpus_en_1000":
            va = dict(t._vocab)
            for s, i in m["longest_first_specials_extra_ids"].items():
                va[s.encode()] = i
            toks["longest_first_specials"] = BBPETokenizer(vocab=va, merges=list(t._merges),
                                                           special_tokens=["<|endoftext|>", "<|x|>", "<|x|><|y|>", "<|y|>"])
        else:
            removed = {bytes.fromhex(h) for h in m["lacking_removed"]}
            lacking = {k: v for k, v in t._vocab.items() if k not in removed}
            toks["lacking_bytes_with_unk"] = BBPETokenizer(vocab=lacking, merges=list(t._merges), special_tokens=list(t.config.special_tokens))
            toks["lacking_bytes_no_unk"] = BBPETokenizer(vocab={k: v for k, v in lacking.items() if k != b"[UNK]"}, merges=list(t._merges),
                                                         special_tokens=[])
        assert set(toks) == set(m["encode"])
        out += [(idx, name, tok) for name, tok in toks.items()]
    return g9, out


def random_model(rng: random.Random, alphabet: str, n_merges: int, specials=(), drop_bytes=False, with_unk=True) -> BBPETokenizer:
    """A tie-heavy model over a tiny alphabet: random merges of existing tokens (duplicates kept: the last rank wins), some
    naming strings that are not in the vocab, and optionally a vocab that lacks some single bytes."""
    toks = [c.encode() for c in alphabet]
    merges = []
    for _ in range(n_merges):
        a, b = rng.choice(toks), rng.choice(toks)
        if rng.random() < 0.1 and merges:
            a, b = rng.choice(merges)  # a duplicate pair
        if rng.random() < 0.05:
            a = b"" if rng.random() < 0.5 else a + b"z"  # names a string the vocab does not hold
        merges.append((a, b))
        if a + b not in toks and len(a + b) < 12:
            toks.append(a + b)
    vocab = {bytes([i]): i for i in range(256)}
    nxt = 256
    for t in toks:
        if t not in vocab:
            vocab[t] = nxt
            nxt += 1
    if drop_bytes:
        for c in rng.sample(alphabet, max(1, len(alphabet) // 2)):
            vocab.pop(c.encode(), None)
        vocab.pop(b" ", None)
    if with_unk:
        vocab[b"[UNK]"] = nxt + 7
    for s in specials:
        if rng.random() < 0.7:
            vocab[s.encode()] = nxt + 100 + len(vocab)
    return BBPETokenizer(vocab=vocab, merges=merges, special_tokens=list(specials))


def lexicon_text(gen, target_bytes: int, seed: int = 11, n_types: int = 30000):
    """synth.text_lexicon text generated on the device: -> (device pointer, n_bytes)."""
    from yet_another_bpe import synth

    lb, lo = synth.text_lexicon(n_types, seed)
    tb, _to, _np, tn = gen.synth_generate_lex(target_bytes, seed, lb, lo)
    return tb, tn


def train_on_device(gen, tb: int, tn: int, n_merges: int, dedup: bool = True):
    """A model trained on the device from the text at tb (one chunk, no specials).  -> (vocab, merges, trained context
    still open for its stream checksum: the caller closes it)."""
    from yet_another_bpe import _native

    base = [bytes([b]) for b in range(256)]
    dt, do, nw = gen.pretokenize(tb, n_bytes=tn)
    ctx = _native.Context()
    ctx.set_vocab(base)
    ctx.load_words_ptr(dt, do, nw, dedup=dedup)
    left, right, merged, _count = ctx.train(n_merges, 1)
    toks, merges = list(base), []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        merges.append((toks[l], toks[r]))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
    return {t: i for i, t in enumerate(toks)}, merges, ctx
