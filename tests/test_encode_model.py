"""CPU: the device encoder's rules (yet-another-bpe_amd/csrc/encode_logic.h + pretok_logic.h, the functions the HIP kernels
call) against BBPETokenizer.encode -- on the G9 set-ups (and G9's pinned ids), on the tokenizer's special-token split with
nesting / overlapping / prefix-sharing specials, and on random tie-heavy models."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest
import regex

from tests import encode_helpers
from yet_another_bpe import _native
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"
GPT2 = r"""'(?:[sdmt]|ll|ve|re)| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libencode_model.so", HM / "encode_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "encode_logic.h", csrc / "pretok_logic.h", csrc / "tile_logic.h", csrc / "unicode_classes.inc"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.encode_model.restype = ctypes.c_int
    return lib


def model_encode(lib, tok: BBPETokenizer, docs: list[bytes]):
    """-> (list of id lists, one per document, error position or -1, checksum triple)"""
    specials = sorted(tok.special_tokens, key=len, reverse=True)
    a = _native.encode_model_arrays(tok._vocab, tok._merges, specials)
    data = b"".join(docs)
    text = np.frombuffer(data or b"\0", dtype=np.uint8).copy()
    starts = np.zeros(max(len(docs), 1), dtype=np.uint64)
    if docs:
        starts[1:] = np.cumsum([len(d) for d in docs])[:-1]
    cap = len(data) + 16
    ids = np.zeros(cap, dtype=np.uint32)
    doc_off = np.zeros(len(starts) + 1, dtype=np.uint64)
    n, err, sums = ctypes.c_uint64(0), ctypes.c_int64(-1), np.zeros(3, dtype=np.uint64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.encode_model(vp(text), ctypes.c_uint64(len(data)), vp(starts), ctypes.c_uint32(len(starts)), vp(a["vb"]), vp(a["vo"]), vp(a["vi"]),
                          ctypes.c_uint32(len(tok._vocab)), vp(a["mb"]), vp(a["mo"]), ctypes.c_uint32(len(tok._merges)), vp(a["sb"]), vp(a["so"]),
                          ctypes.c_uint32(len(specials)), ctypes.c_uint32(tok._vocab.get(b"[UNK]", 0)), vp(ids), ctypes.c_uint64(cap),
                          ctypes.byref(n), vp(doc_off), ctypes.byref(err), vp(sums))
    assert rc == 0, rc
    if err.value >= 0:
        return None, err.value, None
    ids = ids[:n.value].tolist()
    off = doc_off.tolist()
    return [ids[off[d]:off[d + 1]] for d in range(len(docs))], -1, tuple(int(x) for x in sums)


def test_g9_setups_and_pinned_ids(model, golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    assert len(setups) >= 5
    texts = g9["texts"]
    for idx, name, tok in setups:
        got, err, _ = model_encode(model, tok, [t.encode("utf-8") for t in texts])
        assert err == -1
        assert got == tok.encode_batch(texts), name
        assert got == [r["ids"] for r in g9["models"][idx]["encode"][name]], name
        for t in texts[:20]:  # one document per call, too
            assert model_encode(model, tok, [t.encode("utf-8")])[0] == [tok.encode(t)], (name, t)


EDGE_SPECIALS = [["<|x|>", "<|x|><|y|>", "<|y|>"], ["<s>", "<s>x"], ["ab", "abc", "b"], ["a b", " "], ["'s", "it'"], ["x ", " x"],
                 ["<|endoftext|>"], ["<<", "<"], ["aa", "a"], ["\n"], ["''"], ["12", "1"], ["é", "e"], [" 's", "s "]]


def split_pretokens(text: str, specials) -> list[str]:
    """The tokenizer's rule: regex.split on the longest-first alternation, then findall on every text between specials."""
    out = []
    ordered = sorted(specials, key=len, reverse=True)
    parts = regex.compile("(" + "|".join(regex.escape(t) for t in ordered) + ")").split(text) if ordered else [text]
    for p in parts:
        if not p:
            continue
        out += [p] if p in set(specials) else regex.findall(GPT2, p)
    return out


def test_special_split_rule(model):
    """Identity model (no merges, every byte and special its own id): the ids ARE the split, compared with regex."""
    from tests.test_pretok_model import EDGE

    texts = EDGE + ["<|x|><|y|>", "<|x|><|x|><|y|>", "a<|x|><|y|>b", "<|y|><|x|>", "a!<|endoftext|>b", "a  <|endoftext|>", "<s><s>x<s>",
                    "abcab", "a b c", "it's", "x  x x ", "<<<", "aaaa", "\n\nx\n", "1212 121", "éeé", "x's s 's", " 's "]
    for sp in EDGE_SPECIALS:
        vocab = {bytes([i]): i for i in range(256)}
        for k, s in enumerate(sp):
            vocab[s.encode()] = 1000 + k
        tok = BBPETokenizer(vocab=vocab, merges=[], special_tokens=sp)
        for t in texts:
            got, err, _ = model_encode(model, tok, [t.encode("utf-8")])
            assert err == -1
            exp = []
            for p in split_pretokens(t, sp):
                exp += [vocab[p.encode()]] if p in sp else list(p.encode("utf-8"))
            assert got[0] == exp == tok.encode(t), (t, sp)
        for t in texts:  # specials at the start, the end and side by side, inside one batch of documents
            docs = [(sp[0] + t + sp[-1]).encode(), (t + sp[0] + sp[0]).encode(), b"", t.encode()]
            got, err, _ = model_encode(model, tok, docs)
            assert got == [tok.encode(d.decode()) for d in docs], (t, sp)


def test_random_tie_heavy_models(model):
    rng = random.Random(5)
    for trial in range(120):
        alphabet = rng.choice(["ab", "abc", "a b", "xy'", "ab\n"])
        specials = rng.choice([[], ["<s>"], ["ab", "a"], ["aa"], [" b"]])
        tok = encode_helpers.random_model(rng, alphabet, rng.randint(1, 40), specials, drop_bytes=rng.random() < 0.4,
                                          with_unk=rng.random() < 0.5)
        texts = ["".join(rng.choice(alphabet + "a") for _ in range(rng.randint(0, 30))) for _ in range(20)]
        texts += ["a" * rng.randint(1, 80), "ab" * rng.randint(1, 40), " " + "b" * rng.randint(60, 90)]
        got, err, _ = model_encode(model, tok, [t.encode() for t in texts])
        assert err == -1 and got == tok.encode_batch(texts), (trial, alphabet, specials)


def test_invalid_utf8_position(model):
    tok = BBPETokenizer(vocab={bytes([i]): i for i in range(256)}, merges=[], special_tokens=["<s>"])
    for b in [b"\x80", b"a\xc3", b"\xe2\x82<s>", b"<s>\x80", b"ok<s>\xc3\xa9\xa9", b"\xf0\x9f\x98"]:
        with pytest.raises(UnicodeDecodeError) as e:
            b.decode("utf-8")
        assert model_encode(model, tok, [b])[1] == e.value.start, b


def test_checksum_counts_words_and_tokens(model):
    tok = BBPETokenizer(vocab={bytes([i]): i for i in range(256)}, merges=[(b"a", b"b")], special_tokens=["<s>"])
    got, err, sums = model_encode(model, tok, [b"ab ab<s>a"])
    assert got == [tok.encode("ab ab<s>a")] == [[0, ord(" "), 0, ord("a")]]  # "ab" is not in the vocab: unk = 0; "<s>" emits nothing
    assert sums[1] == 1 and sums[2] == 2  # of "ab", " ab", "a" only " ab" keeps 2 tokens (the special is excluded)
