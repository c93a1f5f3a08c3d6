"""Shared by the BPE-dropout tests: documents whose pre-tokens have the lengths at which the device encoder changes its path,
tokenizers with specials, and the ctypes call of the CPU model (tests/hostmodel/dropout_model.cpp)."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

from yet_another_bpe import _native
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"
# pre-token lengths in bytes: one byte (no merge), the 16-lane groups' edge (16 / 17), half a wave (32 / 33), the wave's edge
# (64 / 65: the sequential walk from 65 on) and a few hundred bytes
LENGTHS = [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 66, 130, 300]
LETTERS = "internationalizationthequickbrownfoxjumpsoverthelazydogandtherestofthesentence" * 8
SP, SP_NOID = "<|endoftext|>", "<|noid|>"


def length_text(shift: int = 0) -> str:
    """One pre-token of every length in LENGTHS (a space and letters; the first one a single letter), in a scrambled order."""
    out = ["x"]
    for k, n in enumerate(LENGTHS[1:] + LENGTHS[1:6]):
        at = (7 * k + shift) % 60
        out.append(" " + LETTERS[at:at + n - 1])
    return "".join(out)


def documents(specials=()) -> list[str]:
    """At least 3 documents: an empty one, two identical ones, multi-byte UTF-8 and, with specials, specials next to text and
    to each other."""
    a = length_text(0)
    docs = [a, "", a, "naïve café 中文字 😀😀 It's 42nd…  the the the\n\n  then there", length_text(11), ""]
    if specials:
        s0, s1 = specials[0], specials[-1]
        docs += [s0 + "the" + s1 + s1 + " other" + s0, s0, "the" + s0 + s0 + "the the" + s1 + length_text(3)[:90] + s0]
    return docs


def with_specials(tok: BBPETokenizer) -> BBPETokenizer:
    """tok's model with two specials: one with an id, one without."""
    vocab = dict(tok._vocab)
    vocab[SP.encode()] = max(vocab.values()) + 1
    vocab.pop(SP_NOID.encode(), None)
    return BBPETokenizer(vocab=vocab, merges=list(tok._merges), special_tokens=[SP, SP_NOID])


def per_byte(tok: BBPETokenizer, text: str) -> list[int]:
    """The p = 1 contract: one id per byte of every pre-token, specials as in encode."""
    unk = tok._vocab.get(b"[UNK]", 0)
    out: list[int] = []
    parts = [text] if tok._special_pattern is None else tok._special_pattern.split(text)
    for part in parts:
        if part in tok._special_set:
            out += [tok._vocab[part.encode()]] if part.encode() in tok._vocab else []
        else:
            out += [tok._vocab.get(bytes([b]), unk) for b in part.encode("utf-8")]
    return out


def load_model():
    so, src = HM / "libdropout_model.so", HM / "dropout_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "encode_logic.h", csrc / "pretok_logic.h", csrc / "tile_logic.h", csrc / "unicode_classes.inc"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.dropout_model.restype = ctypes.c_int
    return lib


def model_encode(lib, tok: BBPETokenizer, docs: list[bytes], threshold: int, seed: int):
    """-> (list of id lists, one per document; error position or -1)"""
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
    n, err = ctypes.c_uint64(0), ctypes.c_int64(-1)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.dropout_model(vp(text), ctypes.c_uint64(len(data)), vp(starts), ctypes.c_uint32(len(starts)), vp(a["vb"]), vp(a["vo"]), vp(a["vi"]),
                           ctypes.c_uint32(len(tok._vocab)), vp(a["mb"]), vp(a["mo"]), ctypes.c_uint32(len(tok._merges)), vp(a["sb"]), vp(a["so"]),
                           ctypes.c_uint32(len(specials)), ctypes.c_uint32(tok._vocab.get(b"[UNK]", 0)), ctypes.c_uint64(threshold),
                           ctypes.c_uint64(seed), vp(ids), ctypes.c_uint64(cap), ctypes.byref(n), vp(doc_off), ctypes.byref(err))
    assert rc == 0, rc
    if err.value >= 0:
        return None, err.value
    ids = ids[:n.value].tolist()
    off = doc_off.tolist()
    return [ids[off[d]:off[d + 1]] for d in range(len(docs))], -1
