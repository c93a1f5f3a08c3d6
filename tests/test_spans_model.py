"""CPU: the span rules the device encoder shares with its kernels (yet-another-bpe_amd/csrc/encode_logic.h: the token
starts of the heap walk, the lead rule and the lead-byte prefix per granule) run by tests/hostmodel/spans_model.cpp, against
BBPETokenizer.encode_batch_with_offsets in both units."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import encode_helpers
from tests.test_encode_model import EDGE_SPECIALS
from yet_another_bpe import _native
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libspans_model.so", HM / "spans_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "encode_logic.h", csrc / "pretok_logic.h", csrc / "tile_logic.h", csrc / "unicode_classes.inc"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.spans_model.restype = ctypes.c_int
    return lib


def model_spans(lib, tok: BBPETokenizer, docs: list[bytes], unit: str, lead_pad: bytes = b""):
    """-> [(ids, [(start, end)])] per document.  lead_pad: a document in front that is dropped from the result (the
    documents then start mid-buffer)."""
    specials = sorted(tok.special_tokens, key=len, reverse=True)
    a = _native.encode_model_arrays(tok._vocab, tok._merges, specials)
    docs = [lead_pad] + docs if lead_pad else docs
    data = b"".join(docs)
    text = np.frombuffer(data or b"\0", dtype=np.uint8).copy()
    starts = np.zeros(max(len(docs), 1), dtype=np.uint64)
    if docs:
        starts[1:] = np.cumsum([len(d) for d in docs])[:-1]
    cap = len(data) + 16
    ids, spans = np.zeros(cap, dtype=np.uint32), np.zeros(2 * cap, dtype=np.uint64)
    doc_off = np.zeros(len(starts) + 1, dtype=np.uint64)
    n, err = ctypes.c_uint64(0), ctypes.c_int64(-1)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.spans_model(vp(text), ctypes.c_uint64(len(data)), vp(starts), ctypes.c_uint32(len(starts)), vp(a["vb"]), vp(a["vo"]), vp(a["vi"]),
                         ctypes.c_uint32(len(tok._vocab)), vp(a["mb"]), vp(a["mo"]), ctypes.c_uint32(len(tok._merges)), vp(a["sb"]), vp(a["so"]),
                         ctypes.c_uint32(len(specials)), ctypes.c_uint32(tok._vocab.get(b"[UNK]", 0)), ctypes.c_int(unit == "char"), vp(ids),
                         vp(spans), ctypes.c_uint64(cap), ctypes.byref(n), vp(doc_off), ctypes.byref(err))
    assert rc == 0 and err.value == -1, (rc, err.value)
    ids, off = ids[:n.value].tolist(), doc_off.tolist()
    spans = [tuple(p) for p in spans[:2 * n.value].reshape(-1, 2).tolist()]
    out = [(ids[off[d]:off[d + 1]], spans[off[d]:off[d + 1]]) for d in range(len(docs))]
    return out[1:] if lead_pad else out


def check(lib, tok, texts, what=None):
    for unit in ("byte", "char"):
        exp = tok.encode_batch_with_offsets(texts, unit)
        assert model_spans(lib, tok, [t.encode("utf-8") for t in texts], unit) == exp, (what, unit)


def test_g9_setups(model, golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups:
        check(model, tok, g9["texts"], name)
        for t in g9["texts"][:20]:  # one document per call, too
            check(model, tok, [t], (name, t))


def test_special_split_grid(model):
    from tests.test_pretok_model import EDGE

    texts = EDGE + ["<|x|><|y|>", "<|x|><|x|><|y|>", "a<|x|><|y|>b", "<|y|><|x|>", "a!<|endoftext|>b", "a  <|endoftext|>", "<s><s>x<s>",
                    "abcab", "a b c", "it's", "x  x x ", "<<<", "aaaa", "\n\nx\n", "1212 121", "éeé", "x's s 's", " 's "]
    for sp in EDGE_SPECIALS:
        vocab = {bytes([i]): i for i in range(256)}
        for k, s in enumerate(sp):
            if k != 1:  # the second special has no id: a gap
                vocab[s.encode()] = 1000 + k
        tok = BBPETokenizer(vocab=vocab, merges=[(b"\xc3", b"\xa9"), (b"a", b"a")], special_tokens=sp)
        check(model, tok, texts, sp)
        check(model, tok, [sp[0] + t + sp[-1] for t in texts[:12]] + [t + sp[0] + sp[0] for t in texts[12:24]] + ["", texts[-1]], sp)


def test_random_tie_heavy_models(model):
    rng = random.Random(5)
    for trial in range(120):
        alphabet = rng.choice(["ab", "abc", "a b", "xy'", "ab\n", "é中\U0001F600a 1'"])
        specials = rng.choice([[], ["<s>"], ["ab", "a"], ["aa"], [" b"], ["é"]])
        tok = encode_helpers.random_model(rng, alphabet, rng.randint(1, 40), specials, drop_bytes=rng.random() < 0.4,
                                          with_unk=rng.random() < 0.5)
        texts = ["".join(rng.choice(alphabet + "a") for _ in range(rng.randint(0, 30))) for _ in range(20)]
        texts += ["a" * rng.randint(1, 80), "ab" * rng.randint(1, 40), " " + "b" * rng.randint(60, 90)]
        check(model, tok, texts, (trial, alphabet, specials))


def test_both_paths_and_their_boundary(model):
    """Words of 64 bytes (the last of the lane form), 65 (the first of the heap walk) and 80..200."""
    rng = random.Random(9)
    vocab = {bytes([i]): i for i in range(256)}
    merges = [(b"a", b"b"), (b"ab", b"a"), (b"b", b"b"), (b"aba", b"bb"), (b"\xc3", b"\xa9"), (b"\xc3\xa9", b"\xc3\xa9"), (b" ", b" ")]
    for l, r in merges:
        vocab.setdefault(l + r, 256 + len(vocab))
    tok = BBPETokenizer(vocab=vocab, merges=merges)
    lengths = [63, 64, 65, 66] + list(range(80, 201, 7)) + [200]
    texts = ["".join(rng.choice("ab") for _ in range(n)) for n in lengths]
    texts += ["é" * (n // 2) for n in (62, 64, 66, 128, 200)] + ["a" + "é" * 32, " " * 64 + "x", " " * 65, " " * 150 + "ab" * 60]
    check(model, tok, texts)
    check(model, tok, [" ".join(texts)])


def test_empty_documents_and_documents_mid_buffer(model):
    vocab = {bytes([i]): i for i in range(256)}
    tok = BBPETokenizer(vocab={**vocab, b"<s>": 300}, merges=[(b"\xc3", b"\xa9"), (b"a", b"b")], special_tokens=["<s>", "<t>"])
    texts = ["", "", "é中\U0001F600a 1'", "", "ab<s>é<t>ab" * 9, "\U0001F600" * 40, "", "中" * 70 + " x", ""]
    check(model, tok, texts)
    for pad in (b"x", "é".encode() * 7, b"<t>" * 23, ("中" * 50).encode()):  # documents that start at any offset and granule
        for unit in ("byte", "char"):
            got = model_spans(model, tok, [t.encode("utf-8") for t in texts], unit, lead_pad=pad)
            assert got == tok.encode_batch_with_offsets(texts, unit), (pad, unit)


def test_multi_byte_alphabet(model):
    rng = random.Random(3)
    alphabet = "é中\U0001F600a 1'"
    for trial in range(30):
        tok = encode_helpers.random_model(rng, alphabet, rng.randint(0, 30), rng.choice([[], ["中"], ["é中", "é"]]), drop_bytes=trial % 3 == 0)
        texts = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 120))) for _ in range(25)]
        check(model, tok, texts, trial)
