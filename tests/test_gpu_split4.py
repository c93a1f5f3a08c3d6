"""GPU: the cl100k split pattern (option "split_pattern" = 1, csrc/split4_logic.h) -- yabpe_pretokenize against regex.findall
with the pattern on the lists of the CPU model test, on runs against the piece and window edges and on whitespace runs longer
than one iteration of the carry kernel; malformed UTF-8; the two refusals; the option read per call; training through the
device, host and batched paths against the CPU oracle on regex's words; every device encoder of a cl100k tokenizer against its
plain-Python twin."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import split4_helpers as sh

pytestmark = pytest.mark.gpu

SP = ["<|e|>", "<a>", "[UNK]", "[PAD]"]


def device_split(ctx, data: bytes, specials=(), chunk_starts=(0,)):
    dt, do, nw = ctx.pretokenize(data, chunk_starts=list(chunk_starts), special_tokens=specials)
    off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64).tolist()
    ctx.pretokenize_free()
    assert off[-1] == len(data) and (nw == 0 or off[0] == 0)
    return [data[a:b] for a, b in zip(off[:-1], off[1:])]


def cl100k(ctx, G: int = 3):
    ctx.set_option("digit_group", G)
    ctx.set_option("split_pattern", 1)
    return ctx


def batch_check(ctx, strings, G, specials):
    """All strings in ONE buffer, each as a chunk of its own (chunks are separate texts)."""
    blobs = [s.encode("utf-8") for s in strings if s]
    starts = np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]]).tolist()
    data = b"".join(blobs)
    cl100k(ctx, G)
    got, exp = device_split(ctx, data, specials, starts), sh.regex_split(data, G, specials, starts)
    if got != exp:  # find the first differing string for the message
        for s in strings:
            g = device_split(ctx, s.encode("utf-8"), specials) if s else []
            assert g == sh.regex_split(s.encode("utf-8"), G, specials), (s[:80], G, specials, g[:12])
    assert got == exp


@pytest.mark.parametrize("G", sh.GS)
def test_pretokenize_against_regex(G):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        batch_check(ctx, sh.EDGE + sh.random_strings(31 + G, 2000), G, [])
        for i, sp in enumerate(sh.SPECIAL_SETS):
            batch_check(ctx, sh.BEHIND_SPECIAL + [s.replace("<>", sp[0]) for s in sh.BEHIND_SPECIAL] + sh.EDGE + sh.dense(sp, 200 + i, 700), G, sp)
        # chunk starts inside whitespace and newline runs (one buffer per case: the cuts are the case)
        cl100k(ctx, G)
        for s, cuts in sh.chunk_cases():
            data = s.encode("utf-8")
            assert device_split(ctx, data, [], cuts) == sh.regex_split(data, G, [], cuts), (s[-20:], cuts)


def test_runs_against_piece_and_window_edges():
    """Every string is a buffer of its own, so its window edge is the kernels' window edge."""
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        cl100k(ctx, 3)
        for s in sh.edge_runs():
            data = s.encode("utf-8")
            assert device_split(ctx, data) == sh.regex_split(data, 3), (len(data), s[sh.WIN - 40:sh.WIN + 60])
            assert device_split(ctx, data, ["<>", "a."]) == sh.regex_split(data, 3, ["<>", "a."])


def test_runs_longer_than_one_carry_iteration():
    """More than 2,048 windows of newlines or of spaces (about 8 MB each): the carry kernel iterates twice in both directions.
    The expected offsets are computed, not matched."""
    from yet_another_bpe import _native

    n = (sh.CARRY + 3) * sh.WIN
    cases = [(b"." + b"\n" * n + b" x", [0, n + 1, n + 3]),                  # the O takes every newline; " x" is a letter run
             (b"\n" + b" " * n + b"\n" + b"x", [0, n + 2, n + 3]),           # \s*[\r\n]+ takes all of it up to the last newline
             (b"\n" + b" " * n + b"x", [0, 1, n, n + 2])]                    # "\n", the spaces but one, " x"
    with _native.Context() as ctx:
        cl100k(ctx, 3)
        for (data, exp), s in zip(cases, sh.long_runs()):
            assert data == s.encode("utf-8")
            _dt, do, nw = ctx.pretokenize(data)
            off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64).tolist()
            ctx.pretokenize_free()
            assert off == exp, (off[:6], exp)


@pytest.mark.parametrize("n", sh.TEXT_LENGTHS)
def test_whole_text_lengths(n):
    """Texts of exactly n bytes (sh.TEXT_LENGTHS).  Short ones: newline and whitespace runs cut to n bytes, against regex.  All of
    them, where they are long enough: the two run kinds of test_runs_longer_than_one_carry_iteration filled to n bytes, offsets
    computed (and matched with regex where the text is short)."""
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        cl100k(ctx, 3)
        if n <= 2 * sh.WIN:
            for p in (".\n" + "\n" * n, "\n" + " " * n, "a\n" + " \n" * n, "ab 12 \n\n  x" * n, "\n \n" * n):
                data = p.encode("utf-8")[:n]
                assert device_split(ctx, data) == sh.regex_split(data, 3), (n, p[:12])
        if n >= 4:
            for data, exp in ((b"." + b"\n" * (n - 3) + b" x", [0, n - 2, n]), (b"\n" + b" " * (n - 2) + b"x", [0, 1, n - 2, n])):
                assert len(data) == n
                if n <= 2 * sh.WIN:
                    words = sh.regex_split(data, 3)
                    assert exp == np.concatenate([[0], np.cumsum([len(w) for w in words])]).tolist()
                _dt, do, nw = ctx.pretokenize(data)
                off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64).tolist()
                ctx.pretokenize_free()
                assert off == exp, (n, off[:6], exp)


def test_malformed_utf8_reports_the_same_position():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for raw in (b"abc\xff def", b"a\n \xc3", b"\n \n" * 2000 + b"\xe2\x82 x", b"ok\xed\xa0\x80", b"'s\x80"):
            try:
                raw.decode("utf-8")
                raise AssertionError("the case must be malformed")
            except UnicodeDecodeError as e:
                want = e.start
            got = []
            for pattern, G in ((0, 0), (1, 3)):
                ctx.set_option("digit_group", G)
                ctx.set_option("split_pattern", pattern)
                with pytest.raises(_native.Utf8Error) as err:
                    ctx.pretokenize(raw)
                got.append(err.value.position)
            assert got == [want, want], (raw[-8:], got, want)


def test_refusals_and_option_values():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        cl100k(ctx, 3)
        for tok, what in ((" x", "\\s"), ("\n", "\\s"), ("　a", "\\s"), ("7x", "\\p{N}"), ("²", "\\p{N}")):
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(b"a x 7x", special_tokens=["<|e|>", tok])
            assert e.value.code == -1 and "special token 1" in str(e.value) and what in str(e.value), str(e.value)
        assert device_split(ctx, b"a x 7x", ["x ", "<7"]) == sh.regex_split(b"a x 7x", 3, ["x ", "<7"])
        ctx.set_option("digit_group", 0)  # the pattern needs a group
        with pytest.raises(_native.YabpeError) as e:
            ctx.pretokenize(b"abc")
        assert e.value.code == -1 and "digit_group" in str(e.value)
        ctx.set_option("digit_group", 3)
        for bad in (-1, 2, 1 << 40):
            ctx.set_option("split_pattern", bad)
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(b"abc")
            assert e.value.code == -1 and "split_pattern" in str(e.value)


def test_option_is_read_per_call_and_gpt2_comes_back():
    from tests import group_helpers as gh
    from yet_another_bpe import _native

    data = "\n".join(sh.EDGE + sh.BEHIND_SPECIAL).encode("utf-8")
    with _native.Context() as ctx:
        before = device_split(ctx, data, ["<>"])
        assert before == gh.regex_split(data, 0, ["<>"])
        cl100k(ctx, 3)
        assert device_split(ctx, data, ["<>"]) == sh.regex_split(data, 3, ["<>"]) != before
        ctx.set_option("split_pattern", 0)
        assert device_split(ctx, data, ["<>"]) == gh.regex_split(data, 3, ["<>"])  # the GPT-2 pattern with the group
        ctx.set_option("digit_group", 0)
        assert device_split(ctx, data, ["<>"]) == before


@pytest.mark.parametrize("G", [None, 1])
def test_training_parity(G, golden_dir, tmp_path, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = sh.multilingual(golden_dir)
    f = tmp_path / "multi.txt"
    f.write_bytes(data)
    cfg = BBPETrainerConfig(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, digit_group=G, pretokenizer="cl100k",
                            chunk_size_bytes=1 << 13)
    starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
    assert len(starts) > 2
    exp_vocab, exp_merges = oracle.merge_loop(sh.regex_split(data, G or 3, SP, starts), cfg.vocab_size, 2, SP)
    assert len(exp_merges) == 300
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    dev = BBPETrainer(cfg).train([f])
    batched = BBPETrainer(cfg).train([f], batch_bytes=1 << 14)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    host = BBPETrainer(cfg).train([f])
    for m in (dev, batched, host):
        assert m.merges == exp_merges and m.vocab == exp_vocab and m.digit_group == (G or 3) and m.pretokenizer == "cl100k"
    # the GPT-2 pattern with the same group learns other merges on this text: the pattern is what made the difference
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    plain = BBPETrainer(BBPETrainerConfig(vocab_size=cfg.vocab_size, min_frequency=2, special_tokens=SP, digit_group=G or 3,
                                          chunk_size_bytes=1 << 13)).train([f])
    assert plain.pretokenizer == "gpt2" and plain.merges != dev.merges


@pytest.fixture(scope="module")
def tokenizer(golden_dir, tmp_path_factory):
    """A model of the CPU oracle on regex's words, saved and reloaded: the tokenizer gets its pattern from the file."""
    from oracle import oracle
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = oracle.merge_loop(sh.regex_split(sh.multilingual(golden_dir), 3, SP), 256 + len(SP) + 300, 2, SP)
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="cl100k"))
    tr._vocab, tr._merges = vocab, merges
    d = tmp_path_factory.mktemp("model")
    tr.save_lossless(d)
    tok = BBPETokenizer.from_file_lossless(d)
    assert tok.pretokenizer == "cl100k" and tok.digit_group == 3
    return tok


def encode_texts():
    rng = random.Random(43)
    sp_texts = ["<|e|>…a<a>😀a", "a<|e|>\n \n x<a>'s", "!\n<|e|>\n a", "<a><a>.a<|e|>", " <|e|> ", "x\n<a>", ".<a>\n\n  y"]
    lines = ["I'M sure THEY'LL say it's fine; we'Ve 12345 of them", "def f(x):\n    return x**2  # ok\n\n\n", "a\r\n  b\r\n\r\n", "Привет, мир! 2024",
             "こんにちは世界。１２３４５", "", " ", "\n", "x" + "\n" * 300 + "  y", ".\n" + " " * 300 + "\nz", "\n" + " " * 5000 + "w"]
    return sp_texts + lines + [s for s in sh.EDGE if s] + sh.random_strings(rng.randrange(1000), 300) + sh.dense(["<|e|>", "<a>"], 5, 200)


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
    rows, lengths = tokenizer.encode_array_padded(texts[:40], max_length=64, bos_id=1, eos_id=2)
    exp_rows, exp_lengths = tokenizer.encode_batch_padded(texts[:40], max_length=64, bos_id=1, eos_id=2)
    assert rows.tolist() == exp_rows and lengths.tolist() == exp_lengths
    packed = tokenizer.encode_array_packed(texts[:40], 48, bos_id=1, eos_id=2)
    assert tuple(a.tolist() for a in packed) == tokenizer.encode_batch_packed(texts[:40], 48, bos_id=1, eos_id=2)


def test_gpt2_tokenizer_of_the_same_model_is_unchanged(tokenizer):
    from yet_another_bpe.tokenizer import BBPETokenizer

    plain = BBPETokenizer(tokenizer._vocab, tokenizer._merges, SP)
    texts = encode_texts()
    assert plain.pretokenizer == "gpt2" and plain.encode_batch_device(texts) == plain.encode_batch(texts)
    assert plain.encode_batch(texts) != tokenizer.encode_batch(texts)  # (the texts can tell the two splits apart)
