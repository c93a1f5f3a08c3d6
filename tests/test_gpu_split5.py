"""GPU: the o200k_base split pattern (option "split_pattern" = 3, csrc/split5_logic.h) -- yabpe_pretokenize against regex.findall
with the pattern on the lists of the CPU model test, on runs against the piece and window edges and on chains longer than one
iteration of the carry kernels; malformed UTF-8; the refusals; the option read per call; training through the device, host and
batched paths against the CPU oracle on regex's words; every device encoder of an o200k_base tokenizer against its plain-Python
twin."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import split5_helpers as sh

pytestmark = pytest.mark.gpu

SP = ["<|e|>", "<a>", "[UNK]", "[PAD]"]


def device_offsets(ctx, data: bytes, specials=(), chunk_starts=(0,)):
    dt, do, nw = ctx.pretokenize(data, chunk_starts=list(chunk_starts), special_tokens=specials)
    off = ctx.d2h(do, (nw + 1) * 8).view(np.uint64).tolist()
    ctx.pretokenize_free()
    assert off[-1] == len(data) and (nw == 0 or off[0] == 0)
    return off


def device_split(ctx, data: bytes, specials=(), chunk_starts=(0,)):
    off = device_offsets(ctx, data, specials, chunk_starts)
    return [data[a:b] for a, b in zip(off[:-1], off[1:])]


def o200k(ctx, G: int = 3):
    ctx.set_option("digit_group", G)
    ctx.set_option("split_pattern", 3)
    return ctx


def batch_check(ctx, strings, G, specials):
    """All strings in ONE buffer, each as a chunk of its own (chunks are separate texts)."""
    blobs = [s.encode("utf-8") for s in strings if s]
    starts = np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]]).tolist()
    data = b"".join(blobs)
    o200k(ctx, G)
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
        batch_check(ctx, sh.EDGE + sh.random_strings(31 + G, 2000) + [s for i, a in enumerate(sh.FOCUS.values()) for s in sh.random_strings(70 + i, 500, 24, a)], G, [])
        for i, sp in enumerate(sh.SPECIAL_SETS):
            batch_check(ctx, sh.BEHIND_SPECIAL + [s.replace("<>", sp[0]) for s in sh.BEHIND_SPECIAL] + sh.EDGE + sh.dense(sp, 200 + i, 700), G, sp)
        # chunk starts inside word, punctuation and whitespace runs (one buffer per case: the cuts are the case)
        o200k(ctx, G)
        for s, cuts in sh.chunk_cases():
            data = s.encode("utf-8")
            assert device_split(ctx, data, [], cuts) == sh.regex_split(data, G, [], cuts), (s[-20:], cuts)


def test_runs_against_piece_and_window_edges():
    """Every string is a chunk that starts at a multiple of the window size (the strings are filled up to it), so its window
    edge is the kernels' window edge."""
    from yet_another_bpe import _native

    blobs = []
    for s in sh.edge_runs():
        b = s.encode("utf-8")
        blobs.append(b + b"a" * (-len(b) % sh.WIN))
    starts = np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]]).tolist()
    assert all(a % sh.WIN == 0 for a in starts)
    data = b"".join(blobs)
    with _native.Context() as ctx:
        o200k(ctx, 3)
        for sp in ([], ["<>", "a."]):
            got, exp = device_offsets(ctx, data, sp, starts)[:-1], sh.offsets(sh.regex_split(data, 3, sp, starts))[:-1]
            if got != exp:
                k = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
                raise AssertionError((sp, k, got[k - 2:k + 3], exp[k - 2:k + 3], data[exp[k] - 40:exp[k] + 20]))
            assert len(got) == len(exp)


def test_chains_longer_than_one_carry_iteration():
    """A run of each chain kind over more than 2,048 windows (just over 8 MiB each): both carry kernels iterate twice.  The
    expected offsets are computed, not matched (tests/test_split5_model.py compares them with regex at a small size)."""
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        o200k(ctx, 3)
        for s, exp in sh.long_runs():
            data = s.encode("utf-8")
            assert len(data) > sh.CARRY * sh.WIN
            off = device_offsets(ctx, data)
            assert len(off) == len(exp) + 1 and off[:-1] == exp, (s[:12], off[:6], exp[:6], off[-4:], exp[-3:])


@pytest.mark.parametrize("n", sh.TEXT_LENGTHS)
def test_whole_text_lengths(n):
    """Texts of exactly n bytes (sh.TEXT_LENGTHS), for the backward look-ahead scan and the forward function scan.  Short ones:
    chains of each kind cut to n bytes, against regex.  All of them, where they are long enough: three run kinds of sh.long_runs
    filled to n bytes, offsets computed (and matched with regex where the text is short)."""
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        o200k(ctx, 3)
        if n <= 2 * sh.WIN:
            for p in ("aA" + "A" * n, "\n" + " " * n, "a" + "'s" * n, "!" + "\n/" * n, "AB ab's 12345 !?\n\n  x" * n, "a\n" + " \n" * n, "Ab" * n):
                data = p.encode("utf-8")[:n]
                assert device_split(ctx, data) == sh.regex_split(data, 3), (n, p[:12])
        if n >= 6:
            for s, exp in (("a" + "A" * (n - 2) + "b", [0, 1]), ("\n" + " " * (n - 2) + "x", [0, 1, n - 2]), (". " + "!" * (n - 5) + "\n/a", [0, 1, n - 1])):
                data = s.encode("utf-8")
                assert len(data) == n
                if n <= 2 * sh.WIN:
                    assert exp == sh.offsets(sh.regex_split(data, 3))[:-1]
                off = device_offsets(ctx, data)
                assert off == exp + [n], (n, s[:6], off[:6], exp)


def test_malformed_utf8_reports_the_same_position():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for raw in (b"abc\xff def", b"a\n \xc3", b"\n \n" * 2000 + b"\xe2\x82 x", b"ok\xed\xa0\x80", b"'s\x80", b"AB\xc3", b"A" * 5000 + b"\xf0\x9f\x98 b", b"\x80abc", b"a'\xc5"):
            try:
                raw.decode("utf-8")
                raise AssertionError("the case must be malformed")
            except UnicodeDecodeError as e:
                want = e.start
            got = []
            for pattern, G in ((0, 0), (3, 3)):
                ctx.set_option("digit_group", G)
                ctx.set_option("split_pattern", pattern)
                with pytest.raises(_native.Utf8Error) as err:
                    ctx.pretokenize(raw)
                got.append(err.value.position)
            assert got == [want, want], (raw[-8:], got, want)
        # a chunk start in the middle of a sequence: both halves are malformed, the first is reported
        o200k(ctx, 3)
        with pytest.raises(_native.Utf8Error) as err:
            ctx.pretokenize("aア".encode(), chunk_starts=[0, 2])
        assert err.value.position == 1


def test_refusals_and_option_values():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        o200k(ctx, 3)
        for tok, what in ((" x", "\\s"), ("\n", "\\s"), ("　a", "\\s"), ("7x", "\\p{N}"), ("²", "\\p{N}")):
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(b"a x 7x", special_tokens=["<|e|>", tok])
            assert e.value.code == -1 and "special token 1" in str(e.value) and what in str(e.value), str(e.value)
        for sp, why in sh.REFUSED_SETS:
            if why in ("contains", "suffix"):
                with pytest.raises(_native.YabpeError) as e:
                    ctx.pretokenize(b"a x 7x", special_tokens=sp)
                assert e.value.code == -1 and "special token" in str(e.value) and ("contains" if why == "contains" else "begins") in str(e.value), str(e.value)
                assert all(t in str(e.value) for t in sp if len(sp) == 2)  # both specials are named
        for sp in sh.ACCEPTED_SETS:
            data = ("a x 7x " + " ".join(sp) + "".join(sp)).encode()
            assert device_split(ctx, data, sp) == sh.regex_split(data, 3, sp)
        ctx.set_option("split_pattern", 1)  # the cl100k pattern takes overlapping specials as before
        assert ctx.pretokenize(b"a x 7x", special_tokens=["<a>", "a"])[2] > 0
        ctx.pretokenize_free()
        o200k(ctx, 3)
        ctx.set_option("digit_group", 0)  # the pattern needs a group
        with pytest.raises(_native.YabpeError) as e:
            ctx.pretokenize(b"abc")
        assert e.value.code == -1 and "digit_group" in str(e.value)
        ctx.set_option("digit_group", 3)
        for bad in (-1, 2, 4, 1 << 40):
            ctx.set_option("split_pattern", bad)
            with pytest.raises(_native.YabpeError) as e:
                ctx.pretokenize(b"abc")
            assert e.value.code == -1 and "split_pattern" in str(e.value)


def test_option_is_read_per_call_and_the_other_patterns_come_back():
    from tests import group_helpers as gh
    from tests import split4_helpers as s4
    from yet_another_bpe import _native

    data = "\n".join(sh.EDGE + sh.BEHIND_SPECIAL).encode("utf-8")
    with _native.Context() as ctx:
        before = device_split(ctx, data, ["<>"])
        assert before == gh.regex_split(data, 0, ["<>"])
        ctx.set_option("digit_group", 3)
        ctx.set_option("split_pattern", 1)
        before1 = device_split(ctx, data, ["<>"])
        assert before1 == s4.regex_split(data, 3, ["<>"])
        o200k(ctx, 3)
        mine = device_split(ctx, data, ["<>"])
        assert mine == sh.regex_split(data, 3, ["<>"]) and mine != before and mine != before1
        ctx.set_option("split_pattern", 1)
        assert device_split(ctx, data, ["<>"]) == before1
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
    cfg = BBPETrainerConfig(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, digit_group=G, pretokenizer="o200k_base",
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
        assert m.merges == exp_merges and m.vocab == exp_vocab and m.digit_group == (G or 3) and m.pretokenizer == "o200k_base"
    # train_from continues a model of the pattern: the first 200 merges, then 100 more on the device
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    head_vocab, head_merges = oracle.merge_loop(sh.regex_split(data, G or 3, SP, starts), cfg.vocab_size - 100, 2, SP)
    from yet_another_bpe.trainer import BBPEModel

    cont = BBPETrainer(cfg).train_from(BBPEModel(head_vocab, head_merges, SP, G, "o200k_base"), [f])
    assert cont.merges == exp_merges and cont.vocab == exp_vocab and cont.pretokenizer == "o200k_base"
    # the cl100k pattern with the same group learns other merges on this text: the pattern is what made the difference
    other = BBPETrainer(BBPETrainerConfig(vocab_size=cfg.vocab_size, min_frequency=2, special_tokens=SP, digit_group=G, pretokenizer="cl100k",
                                          chunk_size_bytes=1 << 13)).train([f])
    assert other.pretokenizer == "cl100k" and other.merges != dev.merges


@pytest.fixture(scope="module")
def tokenizer(golden_dir, tmp_path_factory):
    """A model of the CPU oracle on regex's words, saved and reloaded: the tokenizer gets its pattern from the file."""
    from oracle import oracle
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = oracle.merge_loop(sh.regex_split(sh.multilingual(golden_dir), 3, SP), 256 + len(SP) + 300, 2, SP)
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="o200k_base"))
    tr._vocab, tr._merges = vocab, merges
    d = tmp_path_factory.mktemp("model")
    tr.save_lossless(d)
    tok = BBPETokenizer.from_file_lossless(d)
    assert tok.pretokenizer == "o200k_base" and tok.digit_group == 3
    return tok


def encode_texts(golden_dir):
    rng = random.Random(43)
    sp_texts = ["<|e|>…a<a>😀a", "a<|e|>\n \n x<a>'s", "!\n<|e|>\n/a", "<a><a>.a<|e|>", " <|e|> ", "x\n<a>", ".<a>\n\n  y", "AB<a>Cd", "it<|e|>'s", "a'<a>s"]
    page = sh.multilingual(golden_dir, 6000).decode("utf-8")
    lines = ["", " ", "\n", "x" + "\n" * 300 + "  y", ".\n" + " " * 300 + "\nz", "\n" + " " * 5000 + "w", "a" + "A" * 5000 + "b", "Aア" * 1500 + "B", "a" + "'s" * 2500, "!" + "\n/" * 2500]
    return [page] + sp_texts + page.split("\n")[:120] + lines + [s for s in sh.EDGE if s] + sh.random_strings(rng.randrange(1000), 300) + sh.dense(["<|e|>", "<a>"], 5, 200)


def test_encode_parity(tokenizer, golden_dir):
    texts = encode_texts(golden_dir)
    ids, off = tokenizer.encode_array(texts)
    assert [ids[a:b].tolist() for a, b in zip(off[:-1].tolist(), off[1:].tolist())] == tokenizer.encode_batch(texts)
    text, toff = tokenizer.decode_array(ids, off)
    raw = text.tobytes()
    assert [raw[a:b].decode("utf-8") for a, b in zip(toff[:-1].tolist(), toff[1:].tolist())] == texts
    for unit in ("byte", "char"):
        assert tokenizer.encode_batch_device_with_offsets(texts, unit) == tokenizer.encode_batch_with_offsets(texts, unit)
    assert tokenizer.encode_batch_device_dropout(texts, 0.1, seed=7) == tokenizer.encode_batch_dropout(texts, 0.1, seed=7)
    short = texts[1:41]
    rows, lengths = tokenizer.encode_array_padded(short, max_length=64, bos_id=1, eos_id=2)
    exp_rows, exp_lengths = tokenizer.encode_batch_padded(short, max_length=64, bos_id=1, eos_id=2)
    assert rows.tolist() == exp_rows and lengths.tolist() == exp_lengths
    packed = tokenizer.encode_array_packed(short, 48, bos_id=1, eos_id=2)
    assert tuple(a.tolist() for a in packed) == tokenizer.encode_batch_packed(short, 48, bos_id=1, eos_id=2)


def test_tokenizers_of_the_other_patterns_are_unchanged(tokenizer, golden_dir):
    from yet_another_bpe.tokenizer import BBPETokenizer

    texts = encode_texts(golden_dir)
    for name in ("gpt2", "cl100k"):
        other = BBPETokenizer(tokenizer._vocab, tokenizer._merges, SP, pretokenizer=name)
        assert other.pretokenizer == name and other.encode_batch_device(texts) == other.encode_batch(texts)
        assert other.encode_batch(texts) != tokenizer.encode_batch(texts)  # (the texts can tell the splits apart)
