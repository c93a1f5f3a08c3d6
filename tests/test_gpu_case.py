"""GPU: lower-casing (yabpe_lowercase, csrc/yabpe_case_kernels.h) against str.lower() of this interpreter -- the lists of the CPU
model test as parts of one buffer (bytes and offsets), every changing code point as a part of its own, the path each kind of
text takes, the same pointer back for lower-case text, whole-text lengths around a piece, a window and the carry tile, runs of
a mebibyte of ignorables on either side of a sigma, empty text and parts, malformed UTF-8 at the position pretokenize reports,
the life of the results; training with lowercase=True through the device, batched and host routes against the CPU oracle on
regex's words of the lowered chunks; every device encoder of a lower-casing tokenizer against its plain-Python twin."""
from __future__ import annotations

import unicodedata as ud

import numpy as np
import pytest

from tests import case_helpers as ch

pytestmark = pytest.mark.gpu


def check_parts(ctx, strings):
    """the strings as parts of one buffer against str.lower(): bytes and offsets -> the call's stats"""
    buf, starts = ch.pack(strings)
    text, off = ctx.lowercase_to_host(buf, part_starts=starts)
    stats = ctx.lowercase_stats()
    exp, exp_off = ch.reference(buf.tobytes(), starts if len(starts) else [0])
    got, off = text.tobytes(), off.tolist()
    if got != exp or off != exp_off:  # name the first part that differs
        for k, s in enumerate(strings):
            assert got[off[k]:off[k + 1]] == exp[exp_off[k]:exp_off[k + 1]], (k, [hex(ord(c)) for c in s][:40], got[off[k]:off[k + 1]][:60])
        assert off == exp_off
    assert stats["n_bytes_in"] == len(buf) and stats["n_bytes_out"] == len(exp) and stats["n_parts"] == max(len(strings), 1)
    assert stats["n_final_sigma"] == exp.count(ch.FINAL.encode()) - buf.tobytes().count(ch.FINAL.encode())
    return stats


def test_lists_of_the_model_test():
    from yet_another_bpe import _native

    strings = ch.model_strings()
    ch.assert_kinds(strings, ch.part_cases())
    with _native.Context() as ctx:
        stats = check_parts(ctx, strings)
        assert stats["path"] == 2 and stats["n_resized"] > 100 and stats["n_sigma"] > 100 and 0 < stats["n_final_sigma"] < stats["n_sigma"]
        check_parts(ctx, ["".join(strings[lo:lo + 100]) for lo in range(0, 3000, 100)])
        a = ch.class_alphabet()
        check_parts(ctx, [x + ch.SIGMA + y for x in a for y in a])
        for s in ch.SIGMAS + ch.GROW + ch.SHRINK + ch.edge_cases()[::7]:
            check_parts(ctx, [s])
        for data, starts in ch.part_cases():
            text, off = ctx.lowercase_to_host(data, part_starts=starts)
            exp, exp_off = ch.reference(data, starts)
            assert text.tobytes() == exp and off.tolist() == exp_off, (data, starts)


def test_every_changing_code_point():
    from yet_another_bpe import _native

    changing = ch.classes()[0]
    with _native.Context() as ctx:
        stats = check_parts(ctx, [chr(cp) for cp in changing])
        assert stats["n_changed"] == len(changing) == 1393 and stats["n_resized"] == 25 and stats["n_sigma"] == 1 and stats["n_final_sigma"] == 0
        same = [chr(cp) for cp in changing if cp not in ch.resized() and cp != 0x3A3]
        stats = check_parts(ctx, same)
        assert stats["path"] == 1 and stats["n_changed"] == len(same)


def test_path_of_each_kind_of_text():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for text, path in (("plain lower case, caf\u00e9 \u4e2d\u6587 \U0001f600 " * 400, 0), ("Hello, World! " * 700, 1),
                           ("\u041f\u0420\u0418\u0412\u0415\u0422 \u039a\u0391\u039b\u0397 \u00c9t\u00e9 \U00010400 " * 300, 1),
                           ("\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 " * 500, 2), ("lower " * 900 + ch.KELVIN, 2), ("x" * 5000 + ch.DOTTED_I, 2),
                           ("lower " * 900 + ch.SIGMA, 2)):
            stats = check_parts(ctx, [text])
            assert stats["path"] == path, (text[:20], stats)
            assert stats["n_copied"] == (0 if path == 0 else stats["n_bytes_out"])


def test_ascii_pieces_on_the_general_path():
    """Text that is ASCII but for a few code points that send the call down path 2: the write pass lowers a 16-byte ASCII piece
    in registers and puts it into its window's stage at whatever byte the output has reached -- every alignment mod 4 (U+0130
    moves what follows by +1, U+212A by -2), behind window bases that are no multiple of 16, as one part and as several."""
    from yet_another_bpe import _native

    word = "The Quick BROWN Fox, 0123456789 @AZ[ `az{ ~\n"
    texts = []
    for pre in ("", ch.DOTTED_I, ch.DOTTED_I * 2, ch.DOTTED_I * 3, ch.KELVIN, ch.SIGMA):
        texts.append(word * 40 + pre + ch.SIGMA + word * 300 + pre + word * 7 + "A" + ch.SIGMA)
    with _native.Context() as ctx:
        for s in texts:
            stats = check_parts(ctx, [s])
            assert stats["path"] == 2 and stats["n_bytes_in"] > 3 * ch.WIN
        check_parts(ctx, texts)
        check_parts(ctx, ["x" + texts[1][:5000], "", texts[4], "Q" * 33])


def test_lower_case_device_text_comes_back_as_it_is():
    from yet_another_bpe import _native

    line = "the quick brown fox. na\u00efve caf\u00e9 \u4e2d\u6587 \ud55c\uad6d\uc5b4 \U0001f600 \u03c3\u03c2\n".encode()
    text = line * 3000
    starts = [0, 10, 10, 70 * len(line)]
    with _native.Context() as ctx:
        dt, _do, _nw = ctx.pretokenize(text)  # (a device copy of the text to pass in)
        ptr, off_ptr, nb = ctx.lowercase(dt, n_bytes=len(text), part_starts=starts)
        stats = ctx.lowercase_stats()
        assert ptr == dt and nb == len(text)
        assert stats["path"] == 0 and stats["n_changed"] == 0 and stats["n_copied"] == 0 and stats["n_bytes_out"] == len(text)
        assert ctx.d2h(off_ptr, 8 * 5, np.uint64).tolist() == starts + [len(text)]
        # host memory: the result is the staged copy
        out, off = ctx.lowercase_to_host(text, part_starts=starts)
        assert out.tobytes() == text and off.tolist() == starts + [len(text)] and ctx.lowercase_stats()["n_copied"] == 0
        # a device address that is not 16-byte aligned: lowered all the same
        out, off = ctx.lowercase_to_host(dt + 1, n_bytes=len(text) - 1)
        assert out.tobytes() == text[1:] and off.tolist() == [0, len(text) - 1]


@pytest.mark.parametrize("n", ch.TEXT_LENGTHS)
def test_whole_text_lengths(n):
    """Texts of exactly n bytes (ch.TEXT_LENGTHS): a length-changing code point and a sigma at the last byte and at the first."""
    from yet_another_bpe import _native

    strings = [s for s in ch.length_cases() if len(s.encode()) == n]
    assert len(strings) >= 2
    with _native.Context() as ctx:
        for s in strings:
            assert check_parts(ctx, [s])["path"] == (2 if n > 1 else s != s.lower())


def test_carry_edge():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for s in ch.carry_cases():
            check_parts(ctx, [s])


def test_runs_of_ignorables():
    """sigma + 1 MiB of apostrophes + a cased letter (or a space), and the same from the front: exact results; no lane walks
    the run (a piece is 16 bytes whatever it holds)."""
    from yet_another_bpe import _native

    runs = ch.ignorable_runs(1 << 20)
    assert [s.lower().count(ch.FINAL) for s in runs] == [0, 1, 1, 0]
    with _native.Context() as ctx:
        for s in runs:
            stats = check_parts(ctx, [s])
            assert stats["n_sigma"] == 1 and stats["path"] == 2


def test_empty_text_and_empty_parts():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        out, off = ctx.lowercase_to_host(b"")
        assert out.size == 0 and off.tolist() == [0, 0]
        out, off = ctx.lowercase_to_host(b"", part_starts=[0, 0])
        assert out.size == 0 and off.tolist() == [0, 0, 0]
        assert ctx.lowercase_stats()["path"] == 0
        data = (ch.KELVIN + "A" + ch.SIGMA).encode()
        out, off = ctx.lowercase_to_host(data, part_starts=[0, 0, 3, 3, 4, 6, 6])
        assert (out.tobytes(), off.tolist()) == ch.reference(data, [0, 0, 3, 3, 4, 6, 6])


def test_malformed_utf8_reports_the_same_position():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for raw in (b"abc\xff def", b"E\xcc", b"\n \n" * 2000 + b"\xe2\x82 x", b"OK\xed\xa0\x80", b"e\xcc\x81\x80", b"A" * 5000 + b"\xf0\x9f\x98 b", b"\x80abc",
                    ch.SIGMA.encode() * 3000 + b"\xc5", ch.KELVIN.encode()[:2], b"x" * 4095 + b"\xce"):
            try:
                raw.decode("utf-8")
                raise AssertionError("the case must be malformed")
            except UnicodeDecodeError as e:
                want = e.start
            got = []
            for call in (ctx.pretokenize, ctx.lowercase):
                with pytest.raises(_native.Utf8Error) as err:
                    call(raw)
                got.append(err.value.position)
            assert got == [want, want], (raw[-8:], got, want)
        # a part start in the middle of a sequence: both halves are malformed, the first is reported
        with pytest.raises(_native.Utf8Error) as err:
            ctx.lowercase("A\u30a2".encode(), part_starts=[0, 2])
        assert err.value.position == 1


def test_results_are_released_and_replaced():
    from yet_another_bpe import _native

    a, b = "Stra\u00dfe " * 1000, (ch.KELVIN + ch.SIGMA + " ") * 3000
    with _native.Context() as ctx:
        p1, _o1, n1 = ctx.lowercase(a.encode())
        assert ctx.d2h(p1, n1).tobytes() == a.lower().encode()
        p2, _o2, n2 = ctx.lowercase(b.encode())  # replaces the first result
        assert ctx.d2h(p2, n2).tobytes() == b.lower().encode()
        ctx.lowercase_free()
        ctx.lowercase_free()  # (nothing left: a no-op)
        p3, _o3, n3 = ctx.lowercase(a.encode())
        assert ctx.d2h(p3, n3).tobytes() == a.lower().encode()
        # the lowered text goes straight on to the normaliser and the pre-tokeniser: device pointer and new part starts
        text = ("CAF" + "E\u0301 " + ch.DOTTED_I + "\u0316 12 ") * 50
        starts = [0, len(("CAF" + "E\u0301 ").encode())]
        dt, do, nb = ctx.lowercase(text.encode(), part_starts=starts)
        cur = ctx.d2h(do, 8 * 3, np.uint64).tolist()
        dt, do, nb = ctx.normalize(dt, n_bytes=nb, part_starts=cur[:-1])
        new_starts = ctx.d2h(do, 8 * 3, np.uint64).tolist()
        _wt, wo, nw = ctx.pretokenize(dt, n_bytes=nb, chunk_starts=new_starts[:-1])
        off = ctx.d2h(wo, 8 * (nw + 1), np.uint64).tolist()
        norm = ctx.d2h(dt, nb).tobytes()
        raw = text.encode()
        parts = [ud.normalize("NFC", raw[x:y].decode().lower()).encode() for x, y in zip(starts, starts[1:] + [len(raw)])]
        assert norm == b"".join(parts) and new_starts == [0, len(parts[0]), len(norm)]
        from tests.test_pretok_model import regex_split
        assert [norm[x:y] for x, y in zip(off[:-1], off[1:])] == regex_split(norm, [], new_starts[:-1])


SP = ["<|e|>", "<a>", "[unk]", "[pad]"]


def _splitter(name, G):
    from tests import group_helpers as gh
    from tests import split4_helpers as s4

    if name == "cl100k":
        return lambda b, st: s4.regex_split(b, G or 3, SP, st)
    return lambda b, st: gh.regex_split(b, G or 0, SP, st)


@pytest.mark.parametrize("name,G,normalizer", [("gpt2", None, None), ("cl100k", 1, "nfc")])
def test_training_parity(name, G, normalizer, golden_dir, tmp_path, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    data = ch.training_text(golden_dir)
    f = tmp_path / "multi.txt"
    f.write_bytes(data)
    kw = dict(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, digit_group=G, pretokenizer=name, chunk_size_bytes=1 << 13,
              normalizer=normalizer)
    cfg = BBPETrainerConfig(lowercase=True, **kw)
    starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
    assert len(starts) > 2
    words = ch.lowered_words(data, starts, _splitter(name, G), nfc=normalizer == "nfc")
    exp_vocab, exp_merges = oracle.merge_loop(words, cfg.vocab_size, 2, SP)
    assert len(exp_merges) == 300
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    dev = BBPETrainer(cfg).train([f])
    batched = BBPETrainer(cfg).train([f], batch_bytes=1 << 14)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    host = BBPETrainer(cfg).train([f])
    for m in (dev, batched, host):
        assert m.merges == exp_merges and m.vocab == exp_vocab and m.lowercase is True and m.normalizer == normalizer and m.pretokenizer == name
    # train_from continues a lower-casing model: the first 200 merges, then 100 more on the device
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    head_vocab, head_merges = oracle.merge_loop(words, cfg.vocab_size - 100, 2, SP)
    cont = BBPETrainer(cfg).train_from(BBPEModel(head_vocab, head_merges, SP, G, name, normalizer=normalizer, lowercase=True), [f])
    assert cont.merges == exp_merges and cont.vocab == exp_vocab and cont.lowercase is True
    # the control: without lowercase the same file teaches other merges
    other = BBPETrainer(BBPETrainerConfig(**kw)).train([f])
    assert other.lowercase is False and other.merges != dev.merges
    if normalizer is None:
        assert other.merges == oracle.merge_loop(_splitter(name, G)(data, starts), cfg.vocab_size, 2, SP)[1]


def test_training_reports_file_and_position(tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    cfg = BBPETrainerConfig(vocab_size=300, special_tokens=SP, lowercase=True, chunk_size_bytes=1 << 12)
    f = tmp_path / "bad.txt"
    f.write_bytes("\u00c9 OK ".encode() * 2000 + b"\xff tail")
    with pytest.raises(ValueError, match=rf"{f.name} contains invalid UTF-8 at position {6 * 2000}\."):
        BBPETrainer(cfg).train([f])
    # ... and repaired in front of the lower-casing
    cfg = BBPETrainerConfig(vocab_size=300, special_tokens=SP, lowercase=True, errors="replace", chunk_size_bytes=1 << 12)
    tr = BBPETrainer(cfg)
    tr.train([f])
    assert tr.utf8_replaced == 1


@pytest.fixture(scope="module")
def tokenizers(golden_dir, tmp_path_factory):
    """A model of the CPU oracle on regex's words of the lowered, normalised training text (cl100k, G = 1), saved and
    reloaded: the tokenizer gets both settings from the file.  -> (lower-casing, the same model without the setting)"""
    from oracle import oracle
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = oracle.merge_loop(ch.lowered_words(ch.training_text(golden_dir), [0], _splitter("cl100k", 1), nfc=True), 256 + len(SP) + 300, 2, SP)
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="cl100k", digit_group=1, normalizer="nfc", lowercase=True))
    tr._vocab, tr._merges = vocab, merges
    d = tmp_path_factory.mktemp("model")
    tr.save_lossless(d)
    tok = BBPETokenizer.from_file_lossless(d)
    assert tok.lowercase is True and tok.normalizer == "nfc" and tok.pretokenizer == "cl100k" and tok.digit_group == 1
    return tok, BBPETokenizer(vocab, merges, SP, digit_group=1, pretokenizer="cl100k", normalizer="nfc")


def encode_texts(golden_dir):
    page = ch.training_text(golden_dir, 3000).decode("utf-8")
    return [page] + ch.ENCODE_TEXTS + page.split("\n")[:150] + ch.SIGMAS + ch.GROW + ch.SHRINK + ch.random_strings(47, 300) + ["X" * 5000 + "\u03a3" * 700, ""]


def test_encode_parity(tokenizers, golden_dir):
    tok, _plain = tokenizers
    texts = encode_texts(golden_dir)
    norm = [ud.normalize("NFC", t.lower()) for t in texts]
    assert sum(a != b for a, b in zip(texts, norm)) > 100
    assert all(tok.normalize(n) == n for n in norm)  # lower-then-NFC is idempotent
    ids, off = tok.encode_array(texts)
    assert [ids[a:b].tolist() for a, b in zip(off[:-1].tolist(), off[1:].tolist())] == tok.encode_batch(texts) == tok.encode_batch(norm)
    text, toff = tok.decode_array(ids, off)
    raw = text.tobytes()
    # decoding gives the lowered, normalised texts (all of SP have an id)
    assert [raw[a:b].decode("utf-8") for a, b in zip(toff[:-1].tolist(), toff[1:].tolist())] == norm
    ntext, noff = tok.normalize_array(texts)
    nraw = ntext.tobytes()
    assert [nraw[a:b].decode("utf-8") for a, b in zip(noff[:-1].tolist(), noff[1:].tolist())] == norm == [tok.normalize(t) for t in texts]
    for unit in ("byte", "char"):
        assert tok.encode_batch_device_with_offsets(texts, unit) == tok.encode_batch_with_offsets(texts, unit)
    assert tok.encode_batch_device_dropout(texts, 0.1, seed=7) == tok.encode_batch_dropout(texts, 0.1, seed=7)
    short = texts[1:41]
    rows, lengths = tok.encode_array_padded(short, max_length=64, bos_id=1, eos_id=2)
    exp_rows, exp_lengths = tok.encode_batch_padded(short, max_length=64, bos_id=1, eos_id=2)
    assert rows.tolist() == exp_rows and lengths.tolist() == exp_lengths
    packed = tok.encode_array_packed(short, 48, bos_id=1, eos_id=2, dropout=0.2, seed=9)
    assert tuple(a.tolist() for a in packed) == tok.encode_batch_packed(short, 48, bos_id=1, eos_id=2, dropout=0.2, seed=9)
    # windows and pairs, ids and both span units
    from tests import test_gpu_encode_pairs as tp
    from tests import test_gpu_encode_windows as tw
    tw.tok_check(tok, short, "lowercase")
    tp.tok_check(tok, short[:20], short[20:40], "lowercase")
    # a special is matched in the lowered text: its upper-case spelling is the special too, on the device as in Python
    e = tok._vocab[b"<|e|>"]
    assert tok.encode_batch_device(["<|E|>", "<|e|>"]) == [[e], [e]] == tok.encode_batch(["<|E|>", "<|e|>"])
    # one bytes buffer is one document; malformed UTF-8 keeps its position, or is repaired in front of the lower-casing
    assert tok.encode_array(texts[0].encode())[0].tolist() == tok.encode(texts[0])
    from yet_another_bpe import _native
    with pytest.raises(_native.Utf8Error) as err:
        tok.encode_array(b"E\xcc\x81 OK \xff")
    assert err.value.position == 7
    assert tok.encode_array(b"E\xcc\x81 OK \xff", errors="replace")[0].tolist() == tok.encode("E\u0301 OK \ufffd")
    assert tok.encode_batch_device(["", ""]) == [[], []] and tok.encode_array([])[0].size == 0


def test_a_tokenizer_without_the_setting_is_unchanged(tokenizers, golden_dir):
    tok, plain = tokenizers
    texts = encode_texts(golden_dir)
    assert plain.lowercase is False and plain.encode_batch_device(texts) == plain.encode_batch(texts)
    assert plain.encode_batch(texts) != tok.encode_batch(texts)  # (the texts can tell the two apart)
    ntext, noff = plain.normalize_array(texts[:20])
    assert ntext.tobytes() == "".join(ud.normalize("NFC", t) for t in texts[:20]).encode() and noff[-1] == len(ntext)
    for unit in ("byte", "char"):
        assert plain.encode_batch_device_with_offsets(texts, unit) == plain.encode_batch_with_offsets(texts, unit)
