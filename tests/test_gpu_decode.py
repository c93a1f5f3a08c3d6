"""GPU: BBPETokenizer's device decoder (yabpe_decode) against the plain-Python decode -- G9's set-ups (pinned ids and the
encoder's output), random ids over vocabs full of invalid UTF-8, sequences cut at document and kernel-block edges with
long tokens, the error codes, a 1 GiB encode -> decode round trip that stays in HBM, and 64 MiB of random ids."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import decode_helpers, encode_helpers

pytestmark = pytest.mark.gpu


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    texts = g9["texts"]
    for idx, name, tok in setups:
        pinned = [r["ids"] for r in g9["models"][idx]["encode"][name]]
        assert tok.decode_batch_device(pinned) == tok.decode_batch(pinned), name
        ids, off = tok.encode_array(texts)
        text, toff = tok.decode_array(ids, off)  # no glue: encode_array's layout goes straight in
        assert text.dtype == np.uint8 and toff.dtype == np.uint64 and len(toff) == len(texts) + 1
        exp = tok.decode_batch([ids[off[d]:off[d + 1]].tolist() for d in range(len(texts))])
        assert [text[toff[d]:toff[d + 1]].tobytes().decode("utf-8") for d in range(len(texts))] == exp, name
        if name in ("in_memory", "longest_first_specials"):
            assert exp == texts, name
        one = tok.decode_array(ids)  # doc_off None: one document
        assert one[0].tobytes().decode("utf-8") == tok.decode(ids.tolist()) and one[1].tolist() == [0, len(one[0])]


def test_random_ids_5000_documents():
    rng = random.Random(31)
    toks = [("bytes", decode_helpers.byte_tokenizer())] + decode_helpers.stress_tokenizers(rng)
    for name, tok in toks:
        docs = [decode_helpers.random_ids(rng, tok, rng.choice([0, 1, 2, rng.randint(3, 80)])) for _ in range(5000)]
        docs[17] = [max(tok._vocab.values()) + 1, 1 << 31, (1 << 32) - 1]  # only ids past the table
        assert tok.decode_batch_device(docs) == tok.decode_batch(docs), name


def test_block_and_document_edges():
    """Documents longer than one gather block (2,048 ids) and one check tile (4,096 bytes), cut inside multi-byte sequences;
    tokens of 64 to 300 bytes, so that a block's output overflows its LDS stage many times over."""
    rng = random.Random(32)
    text = "".join(rng.choice(["a", "é", "中", "\U0001F600", " "]) for _ in range(60_000)).encode("utf-8")
    tok = decode_helpers.byte_tokenizer()
    cuts = sorted(rng.sample(range(1, len(text)), 40))
    docs = [list(text[a:b]) for a, b in zip([0] + cuts, cuts + [len(text)])]
    assert tok.decode_batch_device(docs) == tok.decode_batch(docs)
    raw = [list(decode_helpers.random_bytes(rng, rng.randint(3000, 9000))) for _ in range(30)]
    assert tok.decode_batch_device(raw) == tok.decode_batch(raw)
    vocab = {bytes([b]): b for b in range(256)}
    for k in range(200):
        vocab[decode_helpers.random_bytes(rng, rng.randint(64, 300))] = 256 + k
    from yet_another_bpe.tokenizer import BBPETokenizer

    big = BBPETokenizer(vocab=vocab, merges=[])
    docs = [[rng.randrange(456) if rng.random() < 0.8 else rng.randrange(256) for _ in range(rng.randint(1, 6000))] for _ in range(25)]
    docs += [[300] * 4096, [0xE4] + [300] * 2047 + [0xB8, 0xAD]]
    assert big.decode_batch_device(docs) == big.decode_batch(docs)
    ctx = big._device("decode")
    st = ctx.decode_stats()
    assert st["n_docs"] == len(docs) and st["n_replacements"] > 0 and st["n_docs_repaired"] > 0 and st["repair_ms"] > 0


def test_error_codes():
    from yet_another_bpe import _native
    from yet_another_bpe.tokenizer import BBPETokenizer

    with _native.Context() as ctx:
        with pytest.raises(_native.YabpeError) as e:
            ctx.decode(np.asarray([1, 2], np.uint32))
        assert e.value.code == -1  # YABPE_E_INVALID: no model
        with pytest.raises(_native.YabpeError) as e:
            ctx.decode_set_model({b"a": 0, b"b": 1 << 24})
        assert e.value.code == -4 and "2^24" in str(e.value)
        ctx.decode_set_model({b"a": (1 << 24) - 1, b"": 3})
        text, off = ctx.decode_to_host(np.asarray([(1 << 24) - 1, 3, 5, 1 << 24], np.uint32))
        assert text.tobytes() == b"a" and off.tolist() == [0, 1]
        assert ctx.decode_stats()["n_unknown"] == 2
        with pytest.raises(_native.YabpeError) as e:
            ctx.decode(np.asarray([1, 2], np.uint32), doc_starts=[0, 3])
        assert e.value.code == -1
    with pytest.raises(_native.YabpeError) as e:
        BBPETokenizer(vocab={b"a": 1 << 25}).decode_array([0])
    assert e.value.code == -4


def test_round_trip_1gib_in_hbm():
    """Lexicon text and a 32,000-merge model trained on the device; yabpe_encode's device results go straight into
    yabpe_decode, and the text comes back byte for byte with the same document offsets."""
    from yet_another_bpe import _native

    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, 1 << 30)
        vocab, merges, ctx = encode_helpers.train_on_device(gen, tb, tn, 32000)
        ctx.close()
        gen.pretokenize_free()
        text = gen.d2h(tb, tn)
        cut = [0]  # 64 documents, cut at character starts
        for k in range(1, 64):
            p = k * tn // 64
            while text[p] & 0xC0 == 0x80:
                p += 1
            cut.append(p)
        gen.encode_set_model(vocab, merges, [], 0)
        gen.decode_set_model(vocab)
        di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=np.asarray(cut, np.uint64))
        dt, do, nb = gen.decode(di, n_ids=ni, doc_starts=dd, n_docs=64)
        assert nb == tn
        assert gen.d2h(do, 8 * 65, np.uint64).tolist() == cut + [tn]
        assert np.array_equal(gen.d2h(dt, nb), text)
        st = gen.decode_stats()
        assert st["n_ids"] == ni and st["n_unknown"] == 0 and st["n_replacements"] == 0 and st["repair_ms"] == 0


def test_random_ids_64mib():
    """16 M random ids (64 MiB) over all single bytes and some multi-byte tokens: invalid UTF-8 throughout, compared with
    Python's decode per document."""
    from yet_another_bpe.tokenizer import BBPETokenizer

    rng = np.random.default_rng(33)
    vocab = {bytes([b]): b for b in range(256)}
    for k, t in enumerate(["é".encode(), "中".encode(), "\U0001F600".encode(), b" the", b"ing", b"\xe4\xb8"]):
        vocab[t] = 256 + k  # (id 262: not in the vocab)
    tok = BBPETokenizer(vocab=vocab, merges=[])
    n = 16 << 20
    ids = np.where(rng.random(n) < 0.9, rng.integers(0x20, 0x7F, n), rng.integers(0, 263, n)).astype(np.uint32)
    cuts = np.sort(rng.choice(np.arange(1, n), 999, replace=False))
    off = np.concatenate(([0], cuts, [n])).astype(np.uint64)
    text, toff = tok.decode_array(ids, off)
    lst = ids.tolist()
    o = off.tolist()
    data = text.tobytes()
    t = toff.tolist()
    for d in range(len(o) - 1):
        assert data[t[d]:t[d + 1]] == tok.decode(lst[o[d]:o[d + 1]]).encode("utf-8"), d
