"""CPU: the contract of BBPETokenizer.encode_dropout / encode_batch_dropout (plain Python is the definition): p = 0 and
p = 1, the argument checks, the threshold T, the batch form, documents and occurrences that draw on their own, the draws'
distribution, and the fixed-shape forms with dropout against a layout done by hand."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import dropout_helpers as dh
from tests import encode_helpers
from yet_another_bpe import synth
from yet_another_bpe.tokenizer import BBPETokenizer


@pytest.fixture(scope="module")
def tok(golden_dir, tmp_path_factory):
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path_factory.mktemp("g9"))
    return dh.with_specials(next(t for _i, name, t in setups if name == "in_memory"))


DOCS = dh.documents([dh.SP, dh.SP_NOID])


def test_p0_is_encode(tok):
    for d, text in enumerate(DOCS):
        assert tok.encode_dropout(text, 0.0, seed=3, doc=d) == tok.encode(text)
        assert tok.encode_dropout(text, 0) == tok.encode(text)


def test_p1_is_one_id_per_byte_with_specials_kept(tok):
    text = DOCS[-1]
    assert dh.SP in text and dh.SP_NOID in text
    got = tok.encode_dropout(text, 1.0, seed=8)
    assert got == dh.per_byte(tok, text) and got.count(tok._vocab[dh.SP.encode()]) == text.count(dh.SP)
    lacking = BBPETokenizer(vocab={b"a": 1, b"[UNK]": 9, b"ab": 2}, merges=[(b"a", b"b")])
    assert lacking.encode_dropout("ab ab", 1, 0) == [1, 9, 9, 1, 9] and lacking.encode_dropout("ab ab", 0, 0) == [2, 9, 2]


def test_value_errors(tok):
    for p in (-1e-9, 1.0000001, float("nan"), float("inf"), "0.5", None, 1j):
        with pytest.raises(ValueError):
            tok.encode_dropout("the", p)
        with pytest.raises(ValueError):
            tok.encode_batch_dropout(["the"], p)
    for bad in (-1, 1 << 64, 0.0, "1", None):
        with pytest.raises(ValueError):
            tok.encode_dropout("the", 0.5, bad)
        with pytest.raises(ValueError):
            tok.encode_dropout("the", 0.5, 0, doc=bad)
    with pytest.raises(ValueError):
        tok.encode_dropout("", 2.0)  # (checked before the empty text returns)
    assert tok.encode_dropout("the", 0.5, (1 << 64) - 1, doc=(1 << 64) - 1) is not None
    assert tok.encode_dropout("the", np.float32(0.5), np.uint64(5), doc=np.int32(2)) == tok.encode_dropout("the", 0.5, 5, doc=2)


def test_threshold():
    T = BBPETokenizer._dropout_threshold
    assert [T(0), T(2.0 ** -33), T(0.5), T(1), T(1.0)] == [0, 0, 1 << 31, 1 << 32, 1 << 32]
    assert T(2.0 ** -32) == 1 and T(1.0 - 2.0 ** -33) == (1 << 32) - 1


def test_rnd_int_is_rnd():
    rng = np.random.default_rng(1)
    for seed, stream, i in rng.integers(0, 1 << 63, size=(200, 3), dtype=np.uint64).tolist() + [[(1 << 64) - 1, 0x77, (1 << 64) - 1]]:
        assert synth.rnd_int(seed, stream, i) == int(synth.rnd(seed, stream, np.uint64(i)))


def test_batch_form_is_the_per_doc_single_form(tok):
    got = tok.encode_batch_dropout(DOCS, 0.5, 21)
    assert got == [tok.encode_dropout(t, 0.5, 21, doc=d) for d, t in enumerate(DOCS)]
    assert tok.encode_batch_dropout(DOCS[2:4], 0.5, 21)[0] == tok.encode_dropout(DOCS[2], 0.5, 21, doc=0)  # doc is the index in the call
    assert tok.encode_batch_dropout([], 0.5, 21) == []


# Confirmed with the contract itself before it was fixed here: " international" has 6 merges under this model (7 parts of 14
# bytes become 1 id at p = 0), and at p = 0.5 the 64 occurrences below take dozens of different segmentations.
WORD = " international"


def test_equal_documents_of_a_batch_differ(tok):
    assert len(tok.encode(WORD)) <= len(WORD.encode()) - 3  # at least 3 merges
    a, b = tok.encode_batch_dropout([WORD * 8, WORD * 8], 0.5, 2)
    assert a != b and tok.decode(a) == tok.decode(b) == WORD * 8


def test_occurrences_in_one_document_differ(tok):
    ids = tok.encode_dropout(WORD * 64, 0.5, 2)
    assert tok.decode(ids) == WORD * 64
    segs, cur, size = set(), [], 0
    for i in ids:  # cut the ids back into the 64 occurrences by their byte lengths
        cur.append(i)
        size += len(tok._vocab_inv[i])
        if size == len(WORD):
            segs.add(tuple(cur))
            cur, size = [], 0
    assert not cur and len(segs) > 1


def test_draws_are_fair():
    n = 100_000
    kw = synth.rnd_int(synth.rnd_int(77, 0x64, 3), 0x77, 1234)
    t, q = np.divmod(np.arange(n, dtype=np.uint64), np.uint64(50))  # 2,000 steps x 50 positions
    draws = np.concatenate([synth.rnd(kw, int(step), q[t == step]) for step in range(0, n // 50, 1)]) >> np.uint64(32)
    assert len(draws) == n
    for p in (0.1, 0.5):
        frac = float(np.mean(draws < np.uint64(BBPETokenizer._dropout_threshold(p))))
        assert abs(frac - p) <= 4 * math.sqrt(p * (1 - p) / n), (p, frac)


def test_fixed_shape_forms_lay_out_the_dropout_ids(tok):
    docs = tok.encode_batch_dropout(DOCS, 0.5, 6)
    rows, lengths = tok.encode_batch_padded(DOCS, 24, bos_id=1, eos_id=2, pad_id=7, dropout=0.5, seed=6)
    for r, n, ids in zip(rows, lengths, docs):
        keep = min(len(ids), 22)
        assert n == keep + 2 and r == [1] + ids[:keep] + [2] + [7] * (24 - n)
    ids, doc, pos = tok.encode_batch_packed(DOCS, 32, eos_id=2, pad_id=7, dropout=0.5, seed=6)
    stream = [i for d in docs for i in d + [2]]
    flat = [i for r in ids for i in r]
    assert flat[:len(stream)] == stream and set(flat[len(stream):]) <= {7} and len(flat) == -(-len(stream) // 32) * 32
    assert [d for r in doc for d in r][:len(stream)] == [d for d, x in enumerate(docs) for _ in range(len(x) + 1)]
    assert [p for r in pos for p in r][:len(stream)] == [k for x in docs for k in range(len(x) + 1)]
    # the defaults are the forms without dropout
    assert tok.encode_batch_padded(DOCS, 24) == tok.encode_batch_padded(DOCS, 24, dropout=0.0, seed=5)
    assert tok.encode_batch_packed(DOCS, 32) == tok.encode_batch_packed(DOCS, 32, dropout=0.0, seed=5)
    assert tok.encode_batch_padded(DOCS, 24, dropout=0.5, seed=6) != tok.encode_batch_padded(DOCS, 24)
    with pytest.raises(ValueError):
        tok.encode_batch_padded(DOCS, 24, dropout=1.5)
    with pytest.raises(ValueError):
        tok.encode_batch_packed(DOCS, 24, dropout=0.5, seed=-1)
