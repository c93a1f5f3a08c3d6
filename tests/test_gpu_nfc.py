"""GPU: NFC normalisation (yabpe_normalize, csrc/yabpe_norm_kernels.h) against unicodedata.normalize("NFC", part) of this
interpreter -- the lists of the CPU model test as parts of one buffer (bytes and offsets), the clean path (same pointer back,
nothing copied), one clean segment of 4 MiB, a dirty segment at the cap and one over it, malformed UTF-8 at the position
pretokenize reports, the form argument, the life of the results; training with normalizer="nfc" through the device, batched
and host routes against the CPU oracle on regex's words of unicodedata-normalised chunks; every device encoder of an "nfc"
tokenizer against its plain-Python twin."""
from __future__ import annotations

import unicodedata as ud

import numpy as np
import pytest

from tests import nfc_helpers as nh

pytestmark = pytest.mark.gpu


def check_parts(ctx, strings):
    """the strings as parts of one buffer against unicodedata: bytes and offsets -> the call's stats"""
    buf, starts = nh.pack(strings)
    text, off = ctx.normalize_to_host(buf, part_starts=starts)
    stats = ctx.normalize_stats()
    exp, exp_off = nh.reference(buf.tobytes(), starts if len(starts) else [0])
    got, off = text.tobytes(), off.tolist()
    if got != exp or off != exp_off:  # name the first part that differs
        for k, s in enumerate(strings):
            assert got[off[k]:off[k + 1]] == exp[exp_off[k]:exp_off[k + 1]], (k, [hex(ord(c)) for c in s][:40], got[off[k]:off[k + 1]][:60])
        assert off == exp_off
    assert stats["n_bytes_in"] == len(buf) and stats["n_bytes_out"] == len(exp) and stats["n_parts"] == max(len(strings), 1)
    return stats


def test_lists_of_the_model_test():
    from yet_another_bpe import _native

    strings = nh.random_strings(23, 200_000)
    nh.assert_kinds(strings)
    with _native.Context() as ctx:
        stats = check_parts(ctx, strings)
        assert stats["n_dirty"] > 50_000 and stats["n_copied"] > 0
        check_parts(ctx, ["".join(strings[lo:lo + 100]) for lo in range(0, 20_000, 100)])
        check_parts(ctx, nh.DIRTY)
        stats = check_parts(ctx, [ud.normalize("NFD", chr(cp)) for cp in range(0xAC00, 0xAC00 + 11172)])
        assert stats["n_dirty"] == 11172
        cps = nh.code_points()
        assert check_parts(ctx, [chr(cp) for cp in cps[::7]])["n_dirty"] > 100
        check_parts(ctx, nh.edge_cases())
        for s in nh.edge_cases()[::5]:
            check_parts(ctx, [s])
        stats = check_parts(ctx, nh.length_cases())
        assert stats["n_dirty_long"] >= 8
        for n, long in ((nh.SHORT - 1, 0), (nh.SHORT, 0), (nh.SHORT + 1, 1)):
            assert check_parts(ctx, ["a" + "\u0301" * (n - 1)])["n_dirty_long"] == long
            assert check_parts(ctx, ["\u1e09" + "\u0323" * (n - 3)])["n_dirty_long"] == long
        for data, starts in nh.part_cases():
            text, off = ctx.normalize_to_host(data, part_starts=starts)
            exp, exp_off = nh.reference(data, starts)
            assert text.tobytes() == exp and off.tolist() == exp_off, (data, starts)


def test_carry_edge():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for s in nh.carry_cases():
            assert check_parts(ctx, [s])["n_dirty"] == 12


@pytest.mark.parametrize("n", nh.TEXT_LENGTHS)
def test_whole_text_lengths(n):
    """Texts of exactly n bytes (nh.TEXT_LENGTHS) against unicodedata: a train of 4-byte dirty segments up to the last byte, as in
    nh.carry_cases (short texts are nothing but the train), and the same text with a dirty segment at its first byte."""
    from yet_another_bpe import _native

    unit = "e\u0301y"  # 4 bytes, not NFC
    tail = unit * 12 + "z" if n >= 64 else "x" * (n % 4) + unit * (n // 4)
    strings = ["x" * (n - len(tail.encode())) + tail]
    if n >= 64:
        strings.append(unit + strings[0][4:])
    with _native.Context() as ctx:
        for s in strings:
            assert len(s.encode()) == n
            assert check_parts(ctx, [s])["n_dirty"] == s.count(unit)


def test_clean_path_returns_the_input():
    from yet_another_bpe import _native

    line = "The quick brown fox. na\u00efve caf\u00e9 \u4e2d\u6587 \ud55c\uad6d\uc5b4 \U0001f600\n".encode()
    text = line * 3000
    starts = [0, 10, 10, 70 * len(line)]
    with _native.Context() as ctx:
        dt, _do, nw = ctx.pretokenize(text)  # (a device copy of the text to pass in)
        ptr, off_ptr, nb = ctx.normalize(dt, n_bytes=len(text), part_starts=starts)
        stats = ctx.normalize_stats()
        assert ptr == dt and nb == len(text)
        assert stats["n_suspects"] == 0 and stats["n_dirty"] == 0 and stats["n_copied"] == 0 and stats["n_bytes_out"] == len(text)
        assert ctx.d2h(off_ptr, 8 * 5, np.uint64).tolist() == starts + [len(text)]
        # host memory: the result is the staged copy
        out, off = ctx.normalize_to_host(text, part_starts=starts)
        assert out.tobytes() == text and off.tolist() == starts + [len(text)] and ctx.normalize_stats()["n_copied"] == 0
        # an empty text, empty parts
        out, off = ctx.normalize_to_host(b"", part_starts=[0, 0])
        assert out.size == 0 and off.tolist() == [0, 0, 0]


def test_one_clean_segment_of_4_mib():
    from yet_another_bpe import _native

    data = "\u0591".encode() * (2 << 20)  # ccc 220, quick-check Yes: nothing starts a segment behind the first
    with _native.Context() as ctx:
        out, off = ctx.normalize_to_host(data)
        stats = ctx.normalize_stats()
        assert out.tobytes() == data and off.tolist() == [0, len(data)]
        assert stats["n_suspects"] == 0 and stats["n_dirty"] == 0 and stats["n_copied"] == 0


def test_cap():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        at = "a" + "\u0301\u0323" * ((nh.CAP - 1) // 2) + "\u0300"  # CAP code points in one dirty segment
        assert len(at) == nh.CAP
        stats = check_parts(ctx, ["xy", at, "z"])
        assert stats["n_dirty"] == 1 and stats["n_dirty_long"] == 1
        over = ("xy" + "a" + "\u0301" * nh.CAP + "z").encode()
        with pytest.raises(_native.SegmentTooLong) as e:
            ctx.normalize(over)
        assert e.value.position == 2 and str(nh.CAP) in str(e.value)
        # the C ABI's code
        import ctypes
        buf = np.frombuffer(over, dtype=np.uint8)
        dt, do, nb, bad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_int64(-1)
        rc = _native.lib().yabpe_normalize(ctx._h, buf.ctypes.data, len(buf), None, 0, 1, ctypes.byref(dt), ctypes.byref(do), ctypes.byref(nb), ctypes.byref(bad))
        assert rc == _native.E_CAPACITY and bad.value == 2


def test_malformed_utf8_reports_the_same_position():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for raw in (b"abc\xff def", b"e\xcc", b"\n \n" * 2000 + b"\xe2\x82 x", b"ok\xed\xa0\x80", b"e\xcc\x81\x80", b"A" * 5000 + b"\xf0\x9f\x98 b", b"\x80abc",
                    "e\u0301".encode() * 3000 + b"\xc5"):
            try:
                raw.decode("utf-8")
                raise AssertionError("the case must be malformed")
            except UnicodeDecodeError as e:
                want = e.start
            got = []
            for call in (ctx.pretokenize, ctx.normalize):
                with pytest.raises(_native.Utf8Error) as err:
                    call(raw)
                got.append(err.value.position)
            assert got == [want, want], (raw[-8:], got, want)
        # a part start in the middle of a sequence: both halves are malformed, the first is reported
        with pytest.raises(_native.Utf8Error) as err:
            ctx.normalize("a\u30a2".encode(), part_starts=[0, 2])
        assert err.value.position == 1


def test_form_argument():
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for form in (0, 2):
            with pytest.raises(_native.YabpeError) as e:
                ctx.normalize(b"abc", form=form)
            assert e.value.code == -1
        assert ctx.normalize_to_host(b"abc", form=_native.NORM_NFC)[0].tobytes() == b"abc"


def test_results_are_released_and_replaced():
    from yet_another_bpe import _native

    a, b = "e\u0301" * 1000, "\u1100\u1161" * 3000
    with _native.Context() as ctx:
        p1, _o1, n1 = ctx.normalize(a.encode())
        assert ctx.d2h(p1, n1).tobytes() == nh.nfc(a).encode()
        p2, _o2, n2 = ctx.normalize(b.encode())  # replaces the first result
        assert ctx.d2h(p2, n2).tobytes() == nh.nfc(b).encode()
        ctx.normalize_free()
        ctx.normalize_free()  # (nothing left: a no-op)
        p3, _o3, n3 = ctx.normalize(a.encode())
        assert ctx.d2h(p3, n3).tobytes() == nh.nfc(a).encode()
        # pre-tokenising the normalised text in place: the device pointer and the new part starts go straight on
        text = ("caf" + "e\u0301 " + "\u1112\u1161\u11ab 12 ") * 50
        starts = [0, len(("caf" + "e\u0301 ").encode())]
        dt, do, nb = ctx.normalize(text.encode(), part_starts=starts)
        new_starts = ctx.d2h(do, 8 * 3, np.uint64).tolist()
        _wt, wo, nw = ctx.pretokenize(dt, n_bytes=nb, chunk_starts=new_starts[:-1])
        off = ctx.d2h(wo, 8 * (nw + 1), np.uint64).tolist()
        norm = ctx.d2h(dt, nb).tobytes()
        exp, exp_off = nh.reference(text.encode(), starts)
        assert norm == exp and new_starts == exp_off
        from tests.test_pretok_model import regex_split
        assert [norm[x:y] for x, y in zip(off[:-1], off[1:])] == regex_split(norm, [], new_starts[:-1])


SP = ["<|e|>", "<a>", "[UNK]", "[PAD]"]


def _splitter(name, G):
    from tests import group_helpers as gh
    from tests import split4_helpers as s4

    if name == "cl100k":
        return lambda b, st: s4.regex_split(b, G or 3, SP, st)
    return lambda b, st: gh.regex_split(b, G or 0, SP, st)


@pytest.mark.parametrize("name,G", [("gpt2", None), ("cl100k", 1)])
def test_training_parity(name, G, golden_dir, tmp_path, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    data = nh.training_text(golden_dir)
    f = tmp_path / "multi.txt"
    f.write_bytes(data)
    kw = dict(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, digit_group=G, pretokenizer=name, chunk_size_bytes=1 << 13)
    cfg = BBPETrainerConfig(normalizer="nfc", **kw)
    starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
    assert len(starts) > 2
    words = nh.normalized_words(data, starts, _splitter(name, G))
    exp_vocab, exp_merges = oracle.merge_loop(words, cfg.vocab_size, 2, SP)
    assert len(exp_merges) == 300
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    dev = BBPETrainer(cfg).train([f])
    batched = BBPETrainer(cfg).train([f], batch_bytes=1 << 14)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    host = BBPETrainer(cfg).train([f])
    for m in (dev, batched, host):
        assert m.merges == exp_merges and m.vocab == exp_vocab and m.normalizer == "nfc" and m.pretokenizer == name
    # train_from continues a model of the normaliser: the first 200 merges, then 100 more on the device
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    head_vocab, head_merges = oracle.merge_loop(words, cfg.vocab_size - 100, 2, SP)
    cont = BBPETrainer(cfg).train_from(BBPEModel(head_vocab, head_merges, SP, G, name, normalizer="nfc"), [f])
    assert cont.merges == exp_merges and cont.vocab == exp_vocab and cont.normalizer == "nfc"
    # the control: without the normaliser the same file teaches other merges
    other = BBPETrainer(BBPETrainerConfig(**kw)).train([f])
    assert other.normalizer is None and other.merges != dev.merges
    assert other.merges == oracle.merge_loop(_splitter(name, G)(data, starts), cfg.vocab_size, 2, SP)[1]


def test_training_reports_file_and_position(tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    cfg = BBPETrainerConfig(vocab_size=300, special_tokens=SP, normalizer="nfc", chunk_size_bytes=1 << 12)
    f = tmp_path / "bad.txt"
    f.write_bytes("e\u0301 ok ".encode() * 2000 + b"\xff tail")
    with pytest.raises(ValueError, match=rf"{f.name} contains invalid UTF-8 at position {7 * 2000}\."):
        BBPETrainer(cfg).train([f])
    g = tmp_path / "long.txt"
    g.write_bytes(b"fine " * 1000 + "a".encode() + "\u0301".encode() * (nh.CAP + 5) + b" tail")
    cfg = BBPETrainerConfig(vocab_size=300, special_tokens=SP, normalizer="nfc", chunk_size_bytes=1 << 20)
    with pytest.raises(ValueError, match=rf"{g.name} holds a run .* at position 5000: .*{nh.CAP}"):
        BBPETrainer(cfg).train([g])


@pytest.fixture(scope="module")
def tokenizers(golden_dir, tmp_path_factory):
    """A model of the CPU oracle on regex's words of the normalised training text (cl100k, G = 1: the Qwen2 front end), saved
    and reloaded: the tokenizer gets its normaliser from the file.  -> (with the normaliser, the same model without it)"""
    from oracle import oracle
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = oracle.merge_loop(nh.normalized_words(nh.training_text(golden_dir), [0], _splitter("cl100k", 1)), 256 + len(SP) + 300, 2, SP)
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="cl100k", digit_group=1, normalizer="nfc"))
    tr._vocab, tr._merges = vocab, merges
    d = tmp_path_factory.mktemp("model")
    tr.save_lossless(d)
    tok = BBPETokenizer.from_file_lossless(d)
    assert tok.normalizer == "nfc" and tok.pretokenizer == "cl100k" and tok.digit_group == 1
    return tok, BBPETokenizer(vocab, merges, SP, digit_group=1, pretokenizer="cl100k")


def encode_texts(golden_dir):
    page = nh.training_text(golden_dir, 3000).decode("utf-8")
    return [page] + nh.ENCODE_TEXTS + page.split("\n")[:150] + nh.DIRTY + nh.random_strings(47, 300) + ["x" * 5000 + "e\u0301" * 700, ""]


def test_encode_parity(tokenizers, golden_dir):
    tok, _plain = tokenizers
    texts = encode_texts(golden_dir)
    norm = [ud.normalize("NFC", t) for t in texts]
    assert sum(a != b for a, b in zip(texts, norm)) > 100
    ids, off = tok.encode_array(texts)
    assert [ids[a:b].tolist() for a, b in zip(off[:-1].tolist(), off[1:].tolist())] == tok.encode_batch(texts)
    text, toff = tok.decode_array(ids, off)
    raw = text.tobytes()
    # decoding gives the normalised texts (minus the specials without an id: all of SP have one)
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
    # a special followed by U+0338 is no special in the normalised text, on the device as in Python
    e = tok._vocab[b"<|e|>"]
    assert e not in tok.encode_batch_device(["<|e|>\u0338"])[0] and tok.encode_batch_device(["<|e|>"]) == [[e]]
    # one bytes buffer is one document; malformed UTF-8 keeps its position
    assert tok.encode_array(texts[0].encode())[0].tolist() == tok.encode(texts[0])
    from yet_another_bpe import _native
    with pytest.raises(_native.Utf8Error) as err:
        tok.encode_array(b"e\xcc\x81 ok \xff")
    assert err.value.position == 7
    assert tok.encode_batch_device(["", ""]) == [[], []] and tok.encode_array([])[0].size == 0


def test_a_tokenizer_without_a_normaliser_is_unchanged(tokenizers, golden_dir):
    tok, plain = tokenizers
    texts = encode_texts(golden_dir)
    assert plain.normalizer is None and plain.encode_batch_device(texts) == plain.encode_batch(texts)
    assert plain.encode_batch(texts) != tok.encode_batch(texts)  # (the texts can tell the two apart)
    ntext, noff = plain.normalize_array(texts[:20])
    assert ntext.tobytes() == "".join(texts[:20]).encode() and noff[-1] == len(ntext)
    for unit in ("byte", "char"):
        assert plain.encode_batch_device_with_offsets(texts, unit) == plain.encode_batch_with_offsets(texts, unit)
