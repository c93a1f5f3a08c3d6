"""GPU: digit groups (option "digit_group": \\p{N}+ of the GPT-2 pattern becomes \\p{N}{1,G}) -- yabpe_pretokenize against
regex.findall with the grouped pattern on the lists of the CPU model test and on digit runs against the window edges; the
option read per call; training with the device and the host pre-tokeniser against the CPU oracle on regex's words; every
device encoder of a tokenizer with digit_group=3 against its plain-Python counterpart; the rejection of a special token
that begins with a digit."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import group_helpers as gh

pytestmark = pytest.mark.gpu

SP = ["<|e|>", "<x1", "[UNK]", "[PAD]"]


def device_split(ctx, data: bytes, specials=(), chunk_starts=(0,)):
    dt, do, nw = ctx.pretokenize(data, chunk_starts=list(chunk_starts), special_tokens=specials)
    off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64).tolist()
    ctx.pretokenize_free()
    assert off[-1] == len(data) and (nw == 0 or off[0] == 0)
    return [data[a:b] for a, b in zip(off[:-1], off[1:])]


def batch_check(ctx, strings, G, specials):
    """All strings in ONE buffer, each as a chunk of its own (chunks are separate texts)."""
    blobs = [s.encode("utf-8") for s in strings if s]
    starts = np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]]).tolist()
    data = b"".join(blobs)
    ctx.set_option("digit_group", G)
    got, exp = device_split(ctx, data, specials, starts), gh.regex_split(data, G, specials, starts)
    if got != exp:  # find the first differing string for the message
        for s in strings:
            g = device_split(ctx, s.encode("utf-8"), specials) if s else []
            assert g == gh.regex_split(s.encode("utf-8"), G, specials), (s[:80], G, specials, g[:12])
    assert got == exp


@pytest.mark.parametrize("G", [1, 3])
def test_pretokenize_against_regex(G):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for sp in gh.SPECIALS:
            batch_check(ctx, gh.ALL_EDGE + gh.random_strings(31 + G, 600), G, sp)
        for sp in ([], ["<x1"]):
            batch_check(ctx, gh.window_cases(), G, sp)
        for s in gh.window_cases()[:5]:  # alone: the run's windows are the buffer's windows
            ctx.set_option("digit_group", G)
            assert device_split(ctx, s.encode("utf-8")) == gh.regex_split(s.encode("utf-8"), G), s[-20:]
        # chunk starts inside digit runs
        data = ("9" * (2 * gh.WIN + 7) + " 1234567 " + "٣" * 50).encode("utf-8")
        cuts = [0, 5, gh.WIN, gh.WIN + 1, 2 * gh.WIN + 10, 2 * gh.WIN + 20]
        assert device_split(ctx, data, [], cuts) == gh.regex_split(data, G, [], cuts)


def test_carry_across_many_windows():
    """More windows than one iteration of the carry scan holds (2048 of them, 8 MiB): one digit run over all of them, a
    letter somewhere inside.  The expected starts are computed, not matched: every third digit of each run."""
    from yet_another_bpe import _native

    n, brk = 2048 * gh.WIN + 3 * gh.WIN + 11, 5 * gh.WIN + 2
    text = np.full(n, ord("7"), np.uint8)
    text[brk] = ord("x")
    exp = np.concatenate([np.arange(0, brk, 3), [brk], np.arange(brk + 1, n, 3), [n]]).astype(np.uint64)
    with _native.Context() as ctx:
        ctx.set_option("digit_group", 3)
        _dt, do, nw = ctx.pretokenize(text)
        off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64)
        assert nw + 1 == len(exp) and np.array_equal(off, exp)


@pytest.mark.parametrize("n", gh.TEXT_LENGTHS)
def test_whole_text_lengths(n):
    """Texts of exactly n bytes: the last piece is 1, 15, 16 bytes or one byte into the next; the text ends one byte short of a
    window, on it, one byte behind it; the carry scan has exactly one full tile of 2,048 windows, and one window more.  A digit
    run with one letter in it, as in test_carry_across_many_windows: the starts are computed, and matched with regex where the
    text is short."""
    from yet_another_bpe import _native

    brk = min(5 * gh.WIN + 2, n // 2)
    text = np.full(n, ord("7"), np.uint8)
    text[brk] = ord("x")
    exp = np.concatenate([np.arange(0, brk, 3), [brk], np.arange(brk + 1, n, 3), [n]]).astype(np.uint64)
    if n <= 2 * gh.WIN:
        words = gh.regex_split(text.tobytes(), 3)
        assert exp.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in words])]).tolist()
    with _native.Context() as ctx:
        ctx.set_option("digit_group", 3)
        _dt, do, nw = ctx.pretokenize(text)
        off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64)
        assert nw + 1 == len(exp) and np.array_equal(off, exp)


def test_option_is_read_per_call():
    from tests.test_pretok_model import regex_split as gpt2_split
    from yet_another_bpe import _native

    data = "\n".join(gh.DIGITS + gh.SPECIAL_TEXTS).encode("utf-8")
    with _native.Context() as ctx:
        assert device_split(ctx, data, ["<x1"]) == gpt2_split(data, ["<x1"])
        ctx.set_option("digit_group", 3)
        assert device_split(ctx, data, ["<x1"]) == gh.regex_split(data, 3, ["<x1"]) != gpt2_split(data, ["<x1"])
        ctx.set_option("digit_group", 0)
        assert device_split(ctx, data, ["<x1"]) == gpt2_split(data, ["<x1"])
        for bad in (-1, 256, 1 << 40):
            ctx.set_option("digit_group", bad)
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(data)
            assert e.value.code == -1 and "digit_group" in str(e.value)  # YABPE_E_INVALID


def test_digit_leading_special_is_rejected():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        ctx.set_option("digit_group", 3)
        for tok in ("77", "٣x", "½"):
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(b"123774", special_tokens=["<|e|>", tok])
            assert e.value.code == -1 and "special token 1" in str(e.value)
        assert device_split(ctx, b"123774", ["<7", "s7"]) == [b"123", b"774"]
        ctx.set_option("digit_group", 0)
        assert device_split(ctx, b"123774", ["77"]) == [b"123774"]  # GPT-2: no token starts inside the run


@pytest.mark.parametrize("G", [1, 3])
def test_training_parity(G, golden_dir, tmp_path, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = gh.number_corpus(golden_dir)
    f = tmp_path / "numbers.txt"
    f.write_bytes(data)
    cfg = BBPETrainerConfig(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, digit_group=G, chunk_size_bytes=1 << 14)
    starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
    assert len(starts) > 2
    exp_vocab, exp_merges = oracle.merge_loop(gh.regex_split(data, G, SP, starts), cfg.vocab_size, 2, SP)
    assert len(exp_merges) == 300
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    dev = BBPETrainer(cfg).train([f])
    batched = BBPETrainer(cfg).train([f], batch_bytes=1 << 15)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    host = BBPETrainer(cfg).train([f])
    for m in (dev, batched, host):
        assert m.merges == exp_merges and m.vocab == exp_vocab and m.digit_group == G
    assert max(gh.digits_in(t) for t in dev.vocab if t.decode("utf-8", "ignore") not in SP) <= G
    # without the group the same corpus learns longer digit strings: the option is what made the difference
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    plain = BBPETrainer(BBPETrainerConfig(vocab_size=cfg.vocab_size, min_frequency=2, special_tokens=SP, chunk_size_bytes=1 << 14)).train([f])
    assert plain.digit_group is None and plain.merges != dev.merges


@pytest.fixture(scope="module")
def tokenizer(golden_dir, tmp_path_factory):
    """A model of the CPU oracle on regex's words (G = 3), saved and reloaded: the tokenizer gets its grouping from the file."""
    from oracle import oracle
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = oracle.merge_loop(gh.regex_split(gh.number_corpus(golden_dir), 3, SP), 256 + len(SP) + 300, 2, SP)
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=3))
    tr._vocab, tr._merges = vocab, merges
    d = tmp_path_factory.mktemp("model")
    tr.save_lossless(d)
    tok = BBPETokenizer.from_file_lossless(d)
    assert tok.digit_group == 3
    return tok


def encode_texts():
    rng = random.Random(41)
    runs = [" ".join("".join(rng.choice("0123456789") for _ in range(rng.randint(4, 40))) for _ in range(6)) for _ in range(12)]
    return (runs + ["In 2024 the total was 1,234,567.8901 units", "call 0049301234567 now<|e|>12345<x1234 ١٢٣٤٥٦", " 1234567 and 12's 1234's", "",
             "²³½Ⅷ12 12\n345", "a1234b<|e|><|e|> 123", "<x1<x12345", "7", "x" + "0123456789" * 3] + gh.DIGITS + gh.window_cases("the ")[:4])  # (short words: the plain-Python merge of one 4 KiB word takes seconds)


def test_encode_parity(tokenizer):
    texts = encode_texts()
    ids, off = tokenizer.encode_array(texts)
    assert [ids[a:b].tolist() for a, b in zip(off[:-1].tolist(), off[1:].tolist())] == tokenizer.encode_batch(texts)
    text, toff = tokenizer.decode_array(ids, off)
    raw = text.tobytes()
    assert [raw[a:b].decode("utf-8") for a, b in zip(toff[:-1].tolist(), toff[1:].tolist())] == texts
    for unit in ("byte", "char"):
        assert tokenizer.encode_batch_device_with_offsets(texts, unit) == tokenizer.encode_batch_with_offsets(texts, unit)
    assert tokenizer.encode_batch_device_dropout(texts, 0.1, seed=7) == tokenizer.encode_batch_dropout(texts, 0.1, seed=7)
    rows, lengths = tokenizer.encode_array_padded(texts[:12], max_length=64, bos_id=1, eos_id=2)
    exp_rows, exp_lengths = tokenizer.encode_batch_padded(texts[:12], max_length=64, bos_id=1, eos_id=2)
    assert rows.tolist() == exp_rows and lengths.tolist() == exp_lengths


def test_encode_without_group_is_unchanged(tokenizer):
    """The same model without the grouping, on the same kind of texts: the GPT-2 split, as before."""
    from yet_another_bpe.tokenizer import BBPETokenizer

    plain = BBPETokenizer(tokenizer._vocab, tokenizer._merges, SP)
    texts = encode_texts()
    assert plain.encode_batch_device(texts) == plain.encode_batch(texts)
    assert plain.encode_batch(texts) != tokenizer.encode_batch(texts)  # (the texts can tell the two splits apart)
