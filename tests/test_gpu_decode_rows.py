"""GPU: yabpe_decode_rows (BBPETokenizer.decode_rows_array) against the plain-Python contract decode_rows_with_offsets: strings,
kept counts and the character span of every column, at the wave (64 lanes x 4 ids) and 2,048-id block edges of the decoder."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import decode_helpers, encode_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu


def with_specials(tok: BBPETokenizer) -> tuple[BBPETokenizer, int, int, int]:
    """tok's vocab plus three specials -> (tokenizer, eos, pad, sep)"""
    top = max(tok._vocab.values())
    names = ["<eos>", "<pad>", "<sep>"]
    vocab = {**tok._vocab, **{s.encode(): top + 2 + k for k, s in enumerate(names)}}
    return (BBPETokenizer(vocab=vocab, merges=[], special_tokens=names), top + 2, top + 3, top + 4)


@pytest.fixture(scope="module")
def toks():
    stress = dict(decode_helpers.stress_tokenizers(random.Random(41)))
    return {"bytes": with_specials(decode_helpers.byte_tokenizer()), "stress": with_specials(stress["gaps"]),
            "long": with_specials(stress["long_tokens"])}


def random_rows(rng: random.Random, tok, eos, pad, sep, B, T, side, ids_of=None):
    """Random ids with the stop and the specials planted at random columns, padded on `side` -> (rows, window arguments)"""
    rows, lens = [], []
    for _ in range(B):
        n = rng.choice([0, T, rng.randint(0, T)])
        row = ids_of(n) if ids_of else decode_helpers.random_ids(rng, tok, n)
        for tid, share, k in ((sep, 0.5, 3), (pad, 0.3, 2), (eos, 0.6, 1)):  # (4 rows in 10 have no stop)
            for _ in range(min(n, k) if rng.random() < share else 0):
                row[rng.randrange(n)] = tid
        rows.append(row + [pad] * (T - n) if side == "right" else [pad] * (T - n) + row)
        lens.append(n)
    lens = np.asarray(lens, np.uint32)
    return np.asarray(rows, np.int64).reshape(B, T), ({"ends": lens} if side == "right" else {"starts": T - lens})


def check(tok, rows, **kw):
    exp_text, exp_spans, exp_kept = tok.decode_rows_with_offsets(rows, **kw)
    text, toff, kept, spans = tok.decode_rows_array(rows, offsets=True, **kw)
    data, toff = text.tobytes(), toff.tolist()
    got = [data[toff[r]:toff[r + 1]].decode("utf-8") for r in range(len(rows))]
    print(len(data), "bytes,", int(kept.sum()), "kept")
    assert got == exp_text
    assert kept.tolist() == exp_kept
    assert spans.dtype == np.uint32 and np.array_equal(spans, np.asarray(exp_spans, np.uint32).reshape(rows.shape + (2,)))
    assert tok.decode_rows_device(rows, **kw) == exp_text  # without offsets: no character pass


@pytest.mark.parametrize("skip_special_tokens", [True, False])
@pytest.mark.parametrize("include_stop", [False, True])
@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("name", ["bytes", "stress"])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 2049])
def test_rows_equal_the_contract(toks, T, B, name, side, include_stop, skip_special_tokens):
    tok, eos, pad, sep = toks[name]
    rng = random.Random(f"{T} {B} {name} {side}")
    rows, window = random_rows(rng, tok, eos, pad, sep, B, T, side)
    check(tok, rows, stop_ids=[eos], pad_id=pad, include_stop=include_stop, skip_special_tokens=skip_special_tokens, **window)


def test_long_tokens_cross_text_tiles(toks):
    """Tokens of 64 to 300 bytes full of ill-formed UTF-8, and rows of whole multi-byte characters cut into single bytes: every
    row runs over many 4,096-byte text tiles, with characters across their edges and across row ends."""
    tok, eos, pad, sep = toks["long"]
    rng = random.Random(43)
    big = [i for t, i in tok._vocab.items() if len(t) >= 64]
    rows, window = random_rows(rng, tok, eos, pad, sep, 9, 130, "right", lambda n: [rng.choice(big) for _ in range(n)])
    check(tok, rows, stop_ids=[eos], pad_id=pad, **window)
    tok, eos, pad, sep = toks["bytes"]
    text = "".join(rng.choice(["a", "é", "中", "\U0001F600"]) for _ in range(12000)).encode("utf-8")
    T = 2731  # (4,096 is no multiple of it, and it is odd: rows start at every alignment)
    rows = np.frombuffer(text[:T * 7], np.uint8).astype(np.int64).reshape(7, T)
    check(tok, rows)
    check(tok, rows, starts=[3] * 7, ends=[T - 2] * 7, skip_ids=[0x80, 0xA9])


def test_device_pointers_from_the_padded_encoder_and_decode_unchanged():
    """yabpe_layout_pad's device rows and lengths go straight in; yabpe_decode on the same context gives the same bytes before
    and after."""
    rng = random.Random(44)
    tok = encode_helpers.random_model(rng, "abc é", 40, with_unk=False)
    texts = ["".join(rng.choice("abc é") for _ in range(rng.randint(0, 90))) for _ in range(37)]
    ctx = tok._device()
    tok._device("decode")
    ids, off = tok.encode_array(texts)
    before = tok.decode_array(ids, off)
    pad = 1 << 20
    for left in (False, True):
        blob, starts = tok._device_input(texts)
        di, dd, ni = ctx.encode(blob, doc_starts=starts)
        dr, dl, L = ctx.layout_pad(di, ni, dd, len(texts), pad_id=pad, pad_left=left)
        lens = ctx.d2h(dl, 4 * len(texts), np.uint32)
        window = {"starts": L - lens} if left else {"ends": dl}
        text, toff, kept = ctx.decode_rows_to_host(dr, len(texts), L, **window)
        assert [text[a:b].tobytes().decode() for a, b in zip(toff[:-1].tolist(), toff[1:].tolist())] == texts
        assert np.array_equal(kept, lens)
    after = tok.decode_array(ids, off)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_error_codes_and_empty_shapes():
    from yet_another_bpe import _native

    rows = np.arange(12, dtype=np.uint32).reshape(3, 4)
    with _native.Context() as ctx:
        with pytest.raises(_native.YabpeError) as e:
            ctx.decode_rows(rows)
        assert e.value.code == -1  # YABPE_E_INVALID: no model
        ctx.decode_set_model({bytes([65 + b]): b for b in range(12)})
        for window in ({"starts": [0, 3, 0], "ends": [4, 2, 4]}, {"ends": [4, 4, 5]}):
            with pytest.raises(_native.YabpeError) as e:
                ctx.decode_rows(rows, **window)
            assert e.value.code == -1 and "window" in str(e.value)
        for lists in ({"stop_ids": range(65)}, {"skip_ids": range(1025)}):
            with pytest.raises(_native.YabpeError) as e:
                ctx.decode_rows(rows, **lists)
            assert e.value.code == -4  # YABPE_E_CAPACITY
        with pytest.raises(_native.YabpeError) as e:
            ctx.decode_rows(0, 1 << 18, 1 << 18)  # 2^36 ids: refused before anything is read
        assert e.value.code == -4
        text, toff, kept, spans = ctx.decode_rows_to_host(rows, stop_ids=range(64), skip_ids=range(9, 1033), offsets=True)
        assert text.tobytes() == b"" and toff.tolist() == [0] * 4 and kept.tolist() == [0] * 3 and not spans.any()
        for shape in ((0, 0), (0, 7), (3, 0)):
            text, toff, kept, spans = ctx.decode_rows_to_host(np.zeros(shape, np.uint32), offsets=True)
            assert len(text) == 0 and toff.tolist() == [0] * (shape[0] + 1) and kept.tolist() == [0] * shape[0] and spans.shape == shape + (2,)
