"""GPU: BBPETokenizer's device encoder (yabpe_encode) id for id against the plain-Python encode -- G9's set-ups and pinned
ids, random strings with nested / overlapping specials, synthetic text with device-trained models (in memory and through
the lossy from_file reload), the trainer's own segmentation at full size (checksums, no Python in the loop) and a 1 GiB
round trip."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import encode_helpers
from tests.test_gpu_pretok import SPECIALS

pytestmark = pytest.mark.gpu


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    texts = g9["texts"]
    for idx, name, tok in setups:
        exp = [r["ids"] for r in g9["models"][idx]["encode"][name]]
        ids, off = tok.encode_array(texts)  # every text a document of its own, one call
        assert off.dtype == np.uint64 and ids.dtype == np.uint32 and len(off) == len(texts) + 1
        got = [ids[off[d]:off[d + 1]].tolist() for d in range(len(texts))]
        assert got == exp, name
        assert tok.encode_batch_device(texts) == exp == tok.encode_batch(texts), name
        for t in texts[:12]:
            assert tok.encode_array(t.encode("utf-8"))[0].tolist() == tok.encode(t), (name, t)


def test_random_strings(golden_dir, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer

    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    base = next(tok for _i, name, tok in setups if name == "in_memory")
    rng = random.Random(21)
    alphabets = ["ab '", "a1 .'s\n", "'stdmlvre x", " \t\n\r\x0b\x0c\x85  a1.", "<|endoftext|> a's", "<s>x' ", "é中\U0001F600a 1'", "[PAD][UNK] ab",
                 "it's ", "<>", "the quick ", "er in on an "]
    for sp in SPECIALS + [["'s", "'"], ["<", "<<", "<<<"], ["aaa", "aa", "a"], [" ", "  "], ["a'll"], ["<|x|>", "<|x|><|y|>", "<|y|>"]]:
        vocab = dict(base._vocab)
        for k, s in enumerate(sp):
            if k % 2 == 0:
                vocab.setdefault(s.encode(), 5000 + k)
        tok = BBPETokenizer(vocab=vocab, merges=list(base._merges), special_tokens=sp)
        strings = ["".join(rng.choice(al) for _ in range(rng.randint(0, 40))) for al in (rng.choice(alphabets) for _ in range(1500))]
        strings += [" " * rng.randint(60, 200), "the" * rng.randint(20, 90)]
        assert tok.encode_batch_device(strings) == tok.encode_batch(strings), sp


def test_utf8_errors_are_reported():
    from yet_another_bpe import _native
    from yet_another_bpe.tokenizer import BBPETokenizer

    tok = BBPETokenizer(vocab={bytes([i]): i for i in range(256)}, merges=[(b"a", b"b")], special_tokens=["<s>"])
    for b in [b"\x80", b"ab\xc3", b"\xe2\x82<s>", b"<s>\x80", b"ok<s>\xc3\xa9\xa9"]:
        with pytest.raises(UnicodeDecodeError) as e:
            b.decode("utf-8")
        with pytest.raises(_native.Utf8Error) as g:
            tok.encode_array(b)
        assert g.value.position == e.value.start, b
    assert tok.encode_array([])[0].size == 0
    assert tok.encode_batch_device(["", "", "ab", "<s>"]) == tok.encode_batch(["", "", "ab", "<s>"]) == [[], [], [0], []]


def test_lexicon_text_device_model(tmp_path):
    from yet_another_bpe import _native
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, 16 << 20)
        vocab, merges, ctx = encode_helpers.train_on_device(gen, tb, tn, 5000)
        ctx.close()
        data = gen.d2h(tb, tn).tobytes()
    cut = [0]  # 64 documents, cut at character starts
    for k in range(1, 64):
        p = k * tn // 64
        while data[p] & 0xC0 == 0x80:
            p += 1
        cut.append(p)
    docs = [data[a:b].decode("utf-8") for a, b in zip(cut, cut[1:] + [tn])]
    t = BBPETrainer(BBPETrainerConfig(vocab_size=len(vocab)))
    t._vocab, t._merges = vocab, merges
    t.save(tmp_path / "m")
    for tok in (BBPETokenizer(vocab=vocab, merges=merges), BBPETokenizer.from_file(tmp_path / "m")):
        assert tok.encode_batch_device(docs) == tok.encode_batch(docs)


@pytest.mark.parametrize("size_mib,n_merges", [(256, 8000), (1024, 32000)])
def test_trainer_segmentation_checksum(size_mib, n_merges):
    """Flat training on the device vs the encoder with that model, no specials on either side: the same pre-tokens, and
    the encoder's merge order (lowest rank first) is the order training applied them, so the segmentations coincide.
    (A lexicon of 2,000 entries has no 64..300-byte runs: every word stays in the trainer's tile stream, which is what
    yabpe_stream_checksum folds.)"""
    from yet_another_bpe import _native

    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, size_mib << 20, n_types=2000)
        vocab, merges, ctx = encode_helpers.train_on_device(gen, tb, tn, n_merges, dedup=False)
        assert ctx.stats()["n_long_words"] == 0
        trained = ctx.stream_checksum()
        ctx.close()
        gen.pretokenize_free()
        gen.encode_set_model(vocab, merges, [], 0)
        gen.encode(tb, n_bytes=tn)
        assert gen.encode_checksum() == trained
        if size_mib == 1024:  # the round trip: the vocab bytes of the ids, concatenated, are the text
            ids, _off = gen.encode_to_host(tb, n_bytes=tn)
            gen.encode_free()
            text = gen.d2h(tb, tn)
            inv = sorted(vocab.items(), key=lambda kv: kv[1])
            assert [i for _t, i in inv] == list(range(len(inv)))
            tlen = np.asarray([len(t) for t, _i in inv], dtype=np.int64)
            toff = np.zeros(len(inv) + 1, dtype=np.int64)
            toff[1:] = np.cumsum(tlen)
            pool = np.frombuffer(b"".join(t for t, _i in inv), dtype=np.uint8)
            pos, step = 0, 1 << 24
            for a in range(0, len(ids), step):
                chunk = ids[a:a + step].astype(np.int64)
                lens = tlen[chunk]
                starts = np.repeat(toff[chunk] - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(int(lens.sum()))
                got = pool[starts]
                assert np.array_equal(got, text[pos:pos + len(got)]), a
                pos += len(got)
            assert pos == tn
