"""GPU: errors="replace" / "ignore" on raw text (yabpe_utf8_repair, csrc/yabpe_utf8_kernels.h) against
bytes.decode("utf-8", errors=mode).encode() of this interpreter -- the lists of the CPU model test as parts of one call each,
host and device input, the valid path (same pointer back after one pass), edge texts of 3 tiles + 5 bytes, the mode argument and
the life of the results; training on the damaged corpus through the device, batched and resumed routes against the CPU oracle
on regex's words of chunk.decode(errors=mode); the device encoders of a bytes buffer against their plain-Python twins."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import utf8_helpers as uh

pytestmark = pytest.mark.gpu


def device_copy(ctx, buf: np.ndarray) -> int:
    """buf in device memory: the staged text of a pretokenize call over as many letters (the context's until pretokenize_free)"""
    dt, _do, _nw = ctx.pretokenize(b"x" * len(buf))
    ctx.h2d(dt, buf)
    return dt


def check_packed(ctx, buf, starts, expected, mode, device=False):
    """one buffer of parts against what CPython gave for it (uh.reference): bytes, offsets, counts -> the call's stats"""
    src = device_copy(ctx, buf) if device else buf
    text, off = ctx.utf8_repair_to_host(src, len(buf), part_starts=starts, mode=uh.MODES[mode])
    stats = ctx.utf8_repair_stats()
    exp, exp_off, n_sub, first = expected
    got, off = text.tobytes(), off.tolist()
    if got != exp or off != exp_off:  # name the first part that differs
        for k in range(len(exp_off) - 1):
            assert got[off[k]:off[k + 1]] == exp[exp_off[k]:exp_off[k + 1]], (k, got[off[k]:off[k + 1]][:60], exp[exp_off[k]:exp_off[k + 1]][:60])
        assert off == exp_off
    assert stats["n_bytes_in"] == len(buf) and stats["n_bytes_out"] == len(exp) and stats["n_parts"] == len(exp_off) - 1
    assert stats["n_subparts"] == n_sub and stats["first_bad_pos"] == first
    if device:
        ctx.pretokenize_free()
    return stats


def check_parts(ctx, parts, mode, device=False):
    """the byte strings as parts of one buffer"""
    buf, starts = uh.pack(parts)
    return check_packed(ctx, buf, starts, uh.reference(buf.tobytes(), starts if len(starts) else [0], mode), mode, device)


LISTS = {"short": uh.short_strings, "random": uh.random_strings, "random_joined": lambda: [b"".join(uh.random_strings(3000))],
         "piece_edge": lambda: uh.edge_cases(uh.PIECE, uh.ill_formed_sequences()), "tile_edge": lambda: uh.edge_cases(uh.TILE, uh.ill_formed_sequences()),
         "tile_edge_joined": lambda: [b"".join(uh.edge_cases(uh.TILE, uh.ill_formed_sequences()[:700]))]}


@pytest.fixture(scope="module")
def lists():
    """name, mode -> (buffer, part starts, CPython's result): each list of the model test packed and repaired once, for the
    host and the device case alike; dropped with the module."""
    packed, expected = {}, {}

    def get(name, mode):
        if name not in packed:
            packed[name] = uh.pack(LISTS[name]())
        if (name, mode) not in expected:
            expected[name, mode] = uh.reference(packed[name][0].tobytes(), packed[name][1], mode)
        return (*packed[name], expected[name, mode])
    return get


@pytest.fixture(scope="module")
def tile():
    """The tile size, from the CPU model of the header the kernels are built from."""
    import subprocess
    from pathlib import Path

    hm = Path(__file__).resolve().parent / "hostmodel"
    so = hm / "libutf8_model.so"
    if not so.exists():
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(hm / "utf8_model.cpp")])
    sizes = np.zeros(3, np.uint32)
    ctypes.CDLL(str(so)).utf8_model_sizes(ctypes.c_void_p(sizes.ctypes.data))
    assert int(sizes[1]) == uh.TILE
    return int(sizes[1])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", list(uh.MODES))
def test_lists_of_the_model_test(mode, device, lists):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        stats = check_packed(ctx, *lists("short", mode), mode, device)  # 406,900 parts, one launch sequence
        assert stats["n_parts"] > 400_000 and stats["n_subparts"] > 400_000
        for name in ("random", "random_joined", "piece_edge"):
            check_packed(ctx, *lists(name, mode), mode, device)
        for text, starts in uh.cut_cases():
            out, off = ctx.utf8_repair_to_host(text, part_starts=starts, mode=uh.MODES[mode])
            exp, exp_off, n_sub, first = uh.reference(text, starts, mode)
            assert out.tobytes() == exp and off.tolist() == exp_off, (text, starts)
            stats = ctx.utf8_repair_stats()
            assert (stats["n_subparts"], stats["first_bad_pos"]) == (n_sub, first)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", list(uh.MODES))
def test_sequences_around_a_tile_edge(mode, device, lists, tile):
    """Every ill-formed sequence at offsets -3 .. +3 around a tile edge: a part of a tile's length each, cut mid-tile."""
    from yet_another_bpe import _native

    assert tile == uh.TILE
    with _native.Context() as ctx:
        stats = check_packed(ctx, *lists("tile_edge", mode), mode, device)
        assert stats["n_parts"] == 7 * len(uh.ill_formed_sequences()) + 1
        check_packed(ctx, *lists("tile_edge_joined", mode), mode, device)  # one part: nothing is clipped at the edges


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_valid_path_returns_the_input(mode, golden_dir):
    from tests import nfc_helpers
    from yet_another_bpe import _native

    m = uh.MODES[mode]
    texts = [b"plain ASCII, " * 3000, (golden_dir / "corpus.en").read_bytes(), nfc_helpers.training_text(golden_dir)]
    with _native.Context() as ctx:
        for text in texts:
            cut = len(text) // 2
            while text[cut] & 0xC0 == 0x80:
                cut -= 1
            starts = [0, 10, 10, cut]
            dt, _do, _nw = ctx.pretokenize(text)  # (a device copy of the text to pass in)
            ptr, off_ptr, nb = ctx.utf8_repair(dt, n_bytes=len(text), part_starts=starts, mode=m)
            stats = ctx.utf8_repair_stats()
            assert ptr == dt and nb == len(text)
            assert stats["n_subparts"] == 0 and stats["first_bad_pos"] == -1 and stats["n_bytes_out"] == len(text) and stats["write_ms"] == 0
            assert ctx.d2h(off_ptr, 8 * 5, np.uint64).tolist() == starts + [len(text)]
            # host memory: the result is the staged copy
            out, off = ctx.utf8_repair_to_host(text, part_starts=starts, mode=m)
            assert out.tobytes() == text and off.tolist() == starts + [len(text)] and ctx.utf8_repair_stats()["n_subparts"] == 0
            ctx.pretokenize_free()
        # an empty text, empty parts
        out, off = ctx.utf8_repair_to_host(b"", part_starts=[0, 0], mode=m)
        assert out.size == 0 and off.tolist() == [0, 0, 0] and ctx.utf8_repair_stats()["n_subparts"] == 0
        ptr, _off_ptr, nb = ctx.utf8_repair(b"", mode=m)
        assert (ptr, nb) == (0, 0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_edge_texts(device, tile):
    from yet_another_bpe import _native

    n = 3 * tile + 5
    with _native.Context() as ctx:
        cuts = [0, 1, tile - 1, tile, tile + 2, 2 * tile, n - 1]
        for starts in ([0], cuts):
            parts = [b"\x80" * (b - a) for a, b in zip(starts, starts[1:] + [n])]
            stats = check_parts(ctx, parts, "replace", device)
            assert stats["n_bytes_out"] == 3 * n and stats["n_subparts"] == n and stats["first_bad_pos"] == 0
            stats = check_parts(ctx, parts, "ignore", device)
            assert stats["n_bytes_out"] == 0 and stats["n_subparts"] == n
            _text, off = ctx.utf8_repair_to_host(np.frombuffer(b"".join(parts), np.uint8), part_starts=starts, mode=uh.MODES["ignore"])
            assert off.tolist() == [0] * (len(starts) + 1)  # every part is empty
        lead = (b"\xf0\x9f\x98" * (n // 3 + 1))[:n]
        ascii_bad = bytearray(b"abcdefgh" * (n // 8 + 1))[:n]
        ascii_bad[n - 2] = 0xFF
        for mode in uh.MODES:
            stats = check_parts(ctx, [lead], mode, device)
            assert stats["n_subparts"] == (n + 2) // 3
            check_parts(ctx, [lead[a:b] for a, b in zip(cuts, cuts[1:] + [n])], mode, device)
            stats = check_parts(ctx, [bytes(ascii_bad)], mode, device)
            assert stats["n_subparts"] == 1 and stats["first_bad_pos"] == n - 2
            # empty parts between parts, at the start, at a tile edge and at the end
            pieces = [b"", b"", lead[:tile], b"", b"", bytes(ascii_bad[tile:2 * tile]), b"", b"\x80" * (tile + 5), b"", b""]
            check_parts(ctx, pieces, mode, device)


def test_unaligned_device_input(tile):
    """A device address that is no multiple of 16 (a rank's slice of a text): the pieces are then loaded byte by byte."""
    from yet_another_bpe import _native

    parts = uh.random_strings(2000) + [b"plain " * 1500, b"\xe2\x82"]
    buf, starts = uh.pack(parts)
    with _native.Context() as ctx:
        dt = device_copy(ctx, buf)
        for k in (1, 2, 3, 7):  # the text from part k on
            base = int(starts[k])
            assert base % 16
            sub_starts = (starts[k:] - np.uint64(base)).astype(np.uint64)
            for mode in uh.MODES:
                text, off = ctx.utf8_repair_to_host(dt + base, len(buf) - base, part_starts=sub_starts, mode=uh.MODES[mode])
                exp, exp_off, n_sub, first = uh.reference(buf[base:].tobytes(), sub_starts, mode)
                assert text.tobytes() == exp and off.tolist() == exp_off
                stats = ctx.utf8_repair_stats()
                assert (stats["n_subparts"], stats["first_bad_pos"]) == (n_sub, first)
        # the valid path hands the same address back, aligned or not
        valid = np.frombuffer(("naïve café " * 2000).encode(), np.uint8)
        ctx.h2d(dt, valid)
        ptr, _off, nb = ctx.utf8_repair(dt + 5, n_bytes=len(valid) - 5, mode=1)
        assert (ptr, nb) == (dt + 5, len(valid) - 5) and ctx.utf8_repair_stats()["n_subparts"] == 0


def test_modes_and_lifetime():
    from yet_another_bpe import _native

    data = np.frombuffer(b"a\xffb\xe2\x82", np.uint8)
    with _native.Context() as ctx:
        for mode in (0, 3, 7, 2**32 - 1):
            dt, do, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
            rc = _native.lib().yabpe_utf8_repair(ctx._h, data.ctypes.data, len(data), None, 0, mode, ctypes.byref(dt), ctypes.byref(do), ctypes.byref(nb))
            assert rc == -1 and "mode" in _native.lib().yabpe_last_error(ctx._h).decode()  # YABPE_E_INVALID
            with pytest.raises(_native.YabpeError):
                ctx.utf8_repair(data, mode=mode)
        # part_off == NULL: one part
        dt, do, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
        rc = _native.lib().yabpe_utf8_repair(ctx._h, data.ctypes.data, len(data), None, 0, 1, ctypes.byref(dt), ctypes.byref(do), ctypes.byref(nb))
        assert rc == 0 and ctx.d2h(dt.value, nb.value).tobytes() == "a�b�".encode()
        assert ctx.d2h(do.value, 16, np.uint64).tolist() == [0, nb.value]
        # the results stay while other calls run, until the next repair or the free
        ptr, off_ptr, nb = ctx.utf8_repair(data, part_starts=[0, 2], mode=2)
        ctx.pretokenize(b"other work " * 1000)
        ctx.normalize("é".encode() * 1000)
        assert ctx.d2h(ptr, nb).tobytes() == b"ab" and ctx.d2h(off_ptr, 24, np.uint64).tolist() == [0, 1, 2]
        ctx.utf8_repair_free()
        ctx.utf8_repair_free()
        with pytest.raises(_native.YabpeError):
            ctx.utf8_repair(data, part_starts=[1, 2])
        with pytest.raises(_native.YabpeError):
            ctx.utf8_repair(data, part_starts=[0, 9])


# ---------------------------------------------------------------- training
SP = ["<|e|>", "<a>", "[UNK]", "[PAD]"]
SETUPS = {"gpt2": dict(), "nfc": dict(normalizer="nfc"), "cl100k": dict(pretokenizer="cl100k")}


def _splitter(name):
    from tests import group_helpers as gh
    from tests import split4_helpers as s4

    if name == "cl100k":
        return lambda b, st: s4.regex_split(b, 3, SP, st)
    return lambda b, st: gh.regex_split(b, 0, SP, st)


def _corpus(name, golden_dir) -> bytes:
    """The damaged corpus of tests/test_utf8_api.py; for the normaliser with damage next to combining marks behind it: a mark
    cut in two, a bad byte between a base and its mark, a mark behind a truncated lead."""
    if name != "nfc":
        return uh.damaged_corpus(golden_dir)
    marks = "é".encode() + b"e\xcc a\xff\xcc\x81 a\xcc\xa3\xff\xcc\x81 \xe2\x82\xcc\x81o\xcc\x88\x80 q\xcc\x87\xcc\xa3\xc3 "
    return uh.damaged_corpus(golden_dir, extra=("café café 각 ".encode() + marks) * 150)


@pytest.mark.parametrize("name", list(SETUPS))
@pytest.mark.parametrize("mode", list(uh.MODES))
def test_training_parity(mode, name, golden_dir, tmp_path, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    data = _corpus(name, golden_dir)
    f = tmp_path / "damaged.txt"
    f.write_bytes(data)
    kw = dict(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, chunk_size_bytes=uh.CHUNK, **SETUPS[name])
    cfg = BBPETrainerConfig(errors=mode, **kw)
    starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
    assert len(starts) > 30
    words = uh.chunk_words(data, starts, mode, _splitter(name), nfc=name == "nfc")
    exp_vocab, exp_merges = oracle.merge_loop(words, cfg.vocab_size, 2, SP)
    assert len(exp_merges) == 300
    n_sub = uh.reference(data, starts, mode)[2]
    assert n_sub > 200
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    runs = {"device": BBPETrainer(cfg), "batched": BBPETrainer(cfg), "resumed": BBPETrainer(cfg)}
    models = {"device": runs["device"].train([f]), "batched": runs["batched"].train([f], batch_bytes=1 << 13)}
    # train_from continues a model of the same reading of the file: the first half of the merges, then the rest on the device
    head_vocab, head_merges = oracle.merge_loop(words, cfg.vocab_size - 150, 2, SP)
    head = BBPEModel(head_vocab, head_merges, SP, pretokenizer=kw.get("pretokenizer", "gpt2"), normalizer=kw.get("normalizer"),
                     digit_group=3 if name == "cl100k" else None)
    models["resumed"] = runs["resumed"].train_from(head, [f])
    for route, m in models.items():
        assert m.merges == exp_merges and m.vocab == exp_vocab, route
        assert runs[route].utf8_replaced == n_sub, route
        assert not hasattr(m, "errors")
    # strict still raises the reference's message, with the position of the first ill-formed byte
    first = uh.reference(data, starts, mode)[3]
    strict = BBPETrainer(BBPETrainerConfig(**kw))
    with pytest.raises(ValueError, match=rf"File .*{f.name} contains invalid UTF-8 at position {first}\."):
        strict.train([f])
    with pytest.raises(ValueError, match=rf"File .*{f.name} contains invalid UTF-8 at position {first}\."):
        strict.train([f], batch_bytes=1 << 13)
    assert strict.utf8_replaced == 0


def test_training_on_a_valid_file_and_errors(golden_dir, tmp_path, monkeypatch):
    from tests import nfc_helpers
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    kw = dict(vocab_size=256 + len(SP) + 100, special_tokens=SP, chunk_size_bytes=1 << 13)
    f = golden_dir / "corpus.en"
    plain = BBPETrainer(BBPETrainerConfig(**kw)).train([f])
    for mode in uh.MODES:
        tr = BBPETrainer(BBPETrainerConfig(errors=mode, **kw))
        m = tr.train([f])
        assert (m.merges, m.vocab) == (plain.merges, plain.vocab) and tr.utf8_replaced == 0
    # a file of nothing but stray bytes: "ignore" leaves no word, the base vocabulary comes back
    g = tmp_path / "stray.txt"
    g.write_bytes(b"\x80" * 10_000)
    tr = BBPETrainer(BBPETrainerConfig(errors="ignore", **kw))
    assert tr.train([g]).merges == [] and tr.utf8_replaced == 10_000
    tr = BBPETrainer(BBPETrainerConfig(errors="ignore", normalizer="nfc", **kw))
    assert tr.train([g], batch_bytes=1 << 12).merges == [] and tr.utf8_replaced == 10_000
    # a run over the normaliser's cap behind a repair: the file, the chunk's range, the position in the repaired chunk
    h = tmp_path / "long.txt"
    h.write_bytes(b"fine \xff" * 1000 + b"a" + "́".encode() * (nfc_helpers.CAP + 5) + b" tail")
    cfg = BBPETrainerConfig(errors="replace", normalizer="nfc", **{**kw, "chunk_size_bytes": 1 << 20})
    with pytest.raises(ValueError, match=rf"{h.name} holds a run .* bytes 0 to {h.stat().st_size}, at position 8000 of that chunk after .*{nfc_helpers.CAP}"):
        BBPETrainer(cfg).train([h])
    cfg = BBPETrainerConfig(errors="ignore", normalizer="nfc", **{**kw, "chunk_size_bytes": 1 << 20})
    with pytest.raises(ValueError, match=rf"{h.name} holds a run .* at position 5000 of that chunk after"):
        BBPETrainer(cfg).train([h])


def test_sharded_driver_of_one_rank(golden_dir, tmp_path):
    from oracle import oracle
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = uh.damaged_corpus(golden_dir)
    f = tmp_path / "damaged.txt"
    f.write_bytes(data)
    for mode in uh.MODES:
        cfg = BBPETrainerConfig(errors=mode, vocab_size=256 + len(SP) + 120, min_frequency=2, special_tokens=SP, chunk_size_bytes=uh.CHUNK)
        starts = [a for a, _ in BBPETrainer(cfg)._chunk_ranges(f)]
        exp_vocab, exp_merges = oracle.merge_loop(uh.chunk_words(data, starts, mode, _splitter("gpt2")), cfg.vocab_size, 2, SP)
        m = train_text_sharded(_native.Context, [f], cfg, 0, 1)
        assert m.merges == exp_merges and m.vocab == exp_vocab


# ---------------------------------------------------------------- encoding
@pytest.fixture(scope="module")
def tokenizers(golden_dir):
    """Models of the CPU oracle on the repaired corpus -> (a GPT-2 tokenizer, a cl100k one with the normaliser)"""
    from oracle import oracle
    from tests import nfc_helpers
    from yet_another_bpe.tokenizer import BBPETokenizer

    data = uh.damaged_corpus(golden_dir)
    v1, m1 = oracle.merge_loop(uh.chunk_words(data, [0], "replace", _splitter("gpt2")), 256 + len(SP) + 300, 2, SP)
    text = nfc_helpers.training_text(golden_dir)
    v2, m2 = oracle.merge_loop(nfc_helpers.normalized_words(text, [0], _splitter("cl100k")), 256 + len(SP) + 300, 2, SP)
    return BBPETokenizer(v1, m1, SP), BBPETokenizer(v2, m2, SP, pretokenizer="cl100k", normalizer="nfc")


def encode_buffers(golden_dir):
    from tests import nfc_helpers

    damaged = uh.damaged_corpus(golden_dir)
    multi = bytearray(nfc_helpers.training_text(golden_dir, 6000))
    for i in range(7, len(multi), 97):
        multi[i] = uh.HIGH[i % len(uh.HIGH)]
    return [damaged, bytes(multi), b"", b"\x80\x80\x80", b"a<|e|>\xffb<a>\xe2\x82", b"e\xcc a\xff\xcc\x81 <|e|>\xcc\xb8", b"plain and valid",
            "café café".encode(), b"\xf0\x9f\x98" * 2000, b"x" * 4090 + b"\xe2\x82\xac\xe2\x82" + b"y" * 10]


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_encode_parity(mode, tokenizers, golden_dir):
    from yet_another_bpe import _native

    for tok in tokenizers:
        inv = {i: t for t, i in tok._vocab.items()}
        for buf in encode_buffers(golden_dir):
            doc = buf.decode("utf-8", mode)
            ids, off = tok.encode_array(buf, errors=mode)
            assert ids.tolist() == tok.encode(doc) and off.tolist() == [0, len(ids)]
            ntext, noff = tok.normalize_array(buf, errors=mode)
            assert ntext.tobytes().decode("utf-8") == tok.normalize(doc) and noff.tolist() == [0, len(ntext)]
            for unit in ("byte", "char"):
                ids2, off2, spans = tok.encode_array_with_offsets(buf, unit, errors=mode)
                assert ids2.tolist() == ids.tolist() and off2.tolist() == off.tolist()
                assert [tuple(p) for p in spans.tolist()] == tok.encode_with_offsets(doc, unit)[1]
            _ids, _off, spans = tok.encode_array_with_offsets(buf, "byte", errors=mode)
            raw = ntext.tobytes()
            assert [raw[a:b] for a, b in spans.tolist()] == [inv[i] for i in ids.tolist()]
        # the default is strict: the position of the first ill-formed byte, as before
        with pytest.raises(_native.Utf8Error) as err:
            tok.encode_array(b"ok \xe2\x82 ok")
        assert err.value.position == 3
        with pytest.raises(_native.Utf8Error):
            tok.encode_array_with_offsets(b"ok \xff", errors="strict")
        # str documents cannot hold ill-formed UTF-8: the option changes nothing
        texts = ["café �", "", "é <|e|>"]
        assert [x.tolist() for x in tok.encode_array(texts, errors=mode)] == [x.tolist() for x in tok.encode_array(texts)]
