"""CPU: the device decoder's rules (yet-another-bpe_amd/csrc/decode_logic.h, the functions the HIP kernels call) against
BBPETokenizer.decode and bytes.decode("utf-8", errors="replace") -- every byte string of length 1 to 4 over one byte of each
UTF-8 class, random longer strings, document cuts inside multi-byte sequences, the G9 set-ups and vocabs with id gaps,
duplicate ids, empty tokens and ids above 2^16."""
from __future__ import annotations

import ctypes
import itertools
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import decode_helpers, encode_helpers
from yet_another_bpe import _native
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libdecode_model.so", HM / "decode_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "decode_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.decode_model.restype = ctypes.c_int
    return lib


def model_decode(lib, tok: BBPETokenizer, docs: list[list[int]]):
    """-> (one bytes object per document, counts (unknown, U+FFFD, documents repaired)); or the builder's error code."""
    a = _native.decode_model_arrays(tok._vocab)
    ids = np.asarray([i for d in docs for i in d] or [0], dtype=np.uint32)
    n_ids = sum(len(d) for d in docs)
    starts = np.zeros(max(len(docs), 1), dtype=np.uint64)
    if docs:
        starts[1:] = np.cumsum([len(d) for d in docs])[:-1]
    longest = max((len(t) for t in tok._vocab), default=1)
    cap = 3 * longest * max(n_ids, 1) + 16
    out = np.zeros(cap, dtype=np.uint8)
    doc_off = np.zeros(len(starts) + 1, dtype=np.uint64)
    n, counts = ctypes.c_uint64(0), np.zeros(3, dtype=np.uint64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.decode_model(vp(a["vb"]), vp(a["vo"]), vp(a["vi"]), ctypes.c_uint32(len(tok._vocab)), vp(ids), ctypes.c_uint64(n_ids), vp(starts),
                          ctypes.c_uint32(len(starts)), vp(out), ctypes.c_uint64(cap), ctypes.byref(n), vp(doc_off), vp(counts))
    if rc:
        return rc
    data, off = out[:n.value].tobytes(), doc_off.tolist()
    return [data[off[d]:off[d + 1]] for d in range(len(docs))], tuple(int(x) for x in counts)


def replace(b: bytes) -> bytes:
    return b.decode("utf-8", errors="replace").encode("utf-8")


def test_issue_examples(model):
    tok = decode_helpers.byte_tokenizer()
    cases = {b"\xf0\x80\x80": 3, b"\xf0\x90\x80a": 1, b"\xed\xa0\x80": 3, b"\xe1\x80": 1, b"\xc0\xaf": 2, b"\xf4\x90\x80\x80": 4, b"\xff": 1}
    got, counts = model_decode(model, tok, [list(b) for b in cases])
    for (b, k), g in zip(cases.items(), got):
        assert g == replace(b) and g.count("�".encode()) == k, b
    assert counts == (0, sum(cases.values()), len(cases))


def test_every_short_string_over_the_byte_classes(model):
    tok = decode_helpers.byte_tokenizer()
    docs = [list(s) for n in range(1, 5) for s in itertools.product(decode_helpers.CLASS_BYTES, repeat=n)]
    assert len(docs) > 400_000
    got, counts = model_decode(model, tok, docs)
    exp = [replace(bytes(d)) for d in docs]
    assert got == exp
    assert counts[1] == sum(e.count("�".encode()) for e in exp)


def test_random_long_strings(model):
    tok = decode_helpers.byte_tokenizer()
    rng = random.Random(5)
    docs = [list(decode_helpers.random_bytes(rng, rng.randint(5, 60))) for _ in range(100_000)]
    got, _counts = model_decode(model, tok, docs)
    assert got == [replace(bytes(d)) for d in docs]


def test_document_cuts_inside_sequences(model):
    tok = decode_helpers.byte_tokenizer()
    rng = random.Random(6)
    text = "".join(rng.choice(["a", "é", "中", "\U0001F600", " ", "߿", "￿"]) for _ in range(20_000)).encode("utf-8")
    cuts = sorted(rng.sample(range(1, len(text)), 3000))
    docs = [list(text[a:b]) for a, b in zip([0] + cuts, cuts + [len(text)])]
    assert sum(1 for c in cuts if text[c] & 0xC0 == 0x80) > 500  # most cuts split a character
    got, counts = model_decode(model, tok, docs)
    assert got == [replace(bytes(d)) for d in docs]
    assert counts[2] > 0
    assert b"".join(model_decode(model, tok, [list(text)])[0]) == text  # uncut: no repair at all


def test_g9_setups(model, golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    rng = random.Random(7)
    for idx, name, tok in setups:
        pinned = [r["ids"] for r in g9["models"][idx]["encode"][name]]
        got, _ = model_decode(model, tok, pinned)
        assert [g.decode("utf-8") for g in got] == tok.decode_batch(pinned), name
        rand = [decode_helpers.random_ids(rng, tok, rng.randint(0, 50)) for _ in range(2000)]
        got, counts = model_decode(model, tok, rand)
        assert [g.decode("utf-8") for g in got] == tok.decode_batch(rand), name
        assert counts[0] == sum(1 for d in rand for i in d if i not in tok._vocab_inv)


def test_stress_vocabs(model):
    rng = random.Random(8)
    for name, tok in decode_helpers.stress_tokenizers(rng):
        docs = [decode_helpers.random_ids(rng, tok, rng.randint(0, 40)) for _ in range(3000)] + [[], []]
        got, _ = model_decode(model, tok, docs)
        assert [g.decode("utf-8") for g in got] == tok.decode_batch(docs), name


def test_table_bounds(model):
    assert model_decode(model, BBPETokenizer(vocab={b"a": (1 << 24) - 1}), [[(1 << 24) - 1]])[0] == [b"a"]
    assert model_decode(model, BBPETokenizer(vocab={b"a": 0, b"b": 1 << 24}), [[0]]) == -1
    with pytest.raises(_native.YabpeError) as e:
        _native.decode_model_arrays({b"a": -1})
    assert e.value.code == _native.E_CAPACITY
