"""CPU: errors="strict" | "replace" | "ignore" through the Python interface -- validation, the option leaves pretokenizer.json,
BBPEModel and train_from's checks alone, the host pre-tokeniser under both modes against regex on chunk.decode(errors=mode),
chunk by chunk, utf8_replaced against a recording error handler, and the inputs of the GPU test (tests/test_gpu_utf8.py): the
damaged corpus, where strict raises, a chunk that ends inside a sequence, and three different models of the C oracle.
No GPU: the models come from the CPU oracle."""
from __future__ import annotations

import pytest

from tests import group_helpers as gh
from tests import utf8_helpers as uh

SP = ["<|e|>", "<a>", "[UNK]", "[PAD]"]
KW = dict(vocab_size=256 + len(SP) + 300, min_frequency=2, special_tokens=SP, chunk_size_bytes=uh.CHUNK)


def split(b, st):
    return gh.regex_split(b, 0, SP, st)


@pytest.fixture(scope="module")
def corpus(golden_dir, tmp_path_factory):
    """(path, damaged bytes, chunk starts of a trainer with chunk_size_bytes = uh.CHUNK)"""
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = uh.damaged_corpus(golden_dir)
    f = tmp_path_factory.mktemp("utf8") / "damaged.txt"
    f.write_bytes(data)
    return f, data, [a for a, _ in BBPETrainer(BBPETrainerConfig(**KW))._chunk_ranges(f)]


def test_validation(tmp_path):
    from yet_another_bpe import trainer as T
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.tokenizer import BBPETokenizer

    assert T.ERRORS == ("strict", "replace", "ignore") and [T.check_errors(n) for n in T.ERRORS] == [0, 1, 2]
    assert T.BBPETrainerConfig().errors == "strict" and T.BBPETrainer().utf8_replaced == 0
    assert T.device_options(T.BBPETrainerConfig(errors="replace")) == {}  # (the repair is a call, not an option)
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    tok = BBPETokenizer({bytes([b]): b for b in range(256)}, [], [])
    for bad in ("Replace", "surrogateescape", "", None, 1, True):
        cfg = T.BBPETrainerConfig(errors=bad)
        for call in (lambda: T.BBPETrainer(cfg).train([f]), lambda: T.BBPETrainer(cfg).train_from(T.BBPEModel({}, [], cfg.special_tokens), [f]),
                     lambda: train_text_sharded(None, [f], cfg, 0, 1), lambda: T.BBPETrainer(cfg)._pretokenize([]),
                     lambda: tok.encode_array([], errors=bad), lambda: tok.encode_array_with_offsets([], errors=bad),
                     lambda: tok.normalize_array(["a"], errors=bad)):
            with pytest.raises(ValueError, match="'strict', 'replace', 'ignore'"):
                call()
    with pytest.raises(FileNotFoundError):  # a good value gets as far as the files
        train_text_sharded(None, [f], T.BBPETrainerConfig(errors="ignore"), 0, 1)
    assert tok.encode_array([], errors="replace")[0].size == 0


def test_the_option_is_no_part_of_the_model(tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab = {bytes([b]): b for b in range(256)}
    vocab.update({t.encode(): 256 + i for i, t in enumerate(SP)})
    vocab[b"ab"] = 260
    files = {}
    for mode in ("strict", "replace", "ignore"):
        for kw in (dict(), dict(pretokenizer="cl100k", normalizer="nfc")):
            tr = BBPETrainer(BBPETrainerConfig(errors=mode, **KW, **kw))
            tr._vocab, tr._merges = dict(vocab), [(b"a", b"b")]
            for name, save in (("plain", tr.save), ("lossless", tr.save_lossless)):
                d = tmp_path / f"{mode}-{len(kw)}-{name}"
                save(d)
                got = {p.name: p.read_bytes() for p in sorted(d.iterdir())}
                assert files.setdefault((len(kw), name), got) == got and all(b"errors" not in v and mode.encode() not in v for v in got.values())
            model = tr._model(tr._vocab, tr._merges)
            assert not hasattr(model, "errors") and "errors" not in vars(model)
    # train_from does not compare it: a model of a strict trainer continues under "replace" (zero budget: no file is read)
    cfg = BBPETrainerConfig(errors="replace", **{**KW, "vocab_size": 261})
    f = tmp_path / "some.txt"
    f.write_bytes(b"ab ab \xff")
    cont = BBPETrainer(cfg).train_from(BBPEModel(vocab, [(b"a", b"b")], SP), [f])
    assert cont.merges == [(b"a", b"b")] and cont.vocab == vocab


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_host_pretokenize_repairs_every_chunk(mode, corpus, golden_dir):
    from tests import split4_helpers as s4
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    f, data, starts = corpus
    assert len(starts) > 30
    tr = BBPETrainer(BBPETrainerConfig(errors=mode, **KW))
    got = [t.encode("utf-8") for t in tr._pretokenize([f])]
    assert got == uh.chunk_words(data, starts, mode, split)
    # utf8_replaced: what a recording error handler sees, chunk by chunk
    cuts = starts + [len(data)]
    seen = sum(len(uh.subparts(data[a:b])) for a, b in zip(cuts[:-1], cuts[1:]))
    assert tr.utf8_replaced == seen == uh.reference(data, starts, mode)[2] > len(data) // uh.DAMAGE_RATE // 2
    assert tr.utf8_replaced != len(uh.subparts(data))  # (the chunk cuts count: read as one text there are fewer)
    # with the other pattern and the normaliser behind it
    tr = BBPETrainer(BBPETrainerConfig(errors=mode, pretokenizer="cl100k", normalizer="nfc", **KW))
    assert [t.encode("utf-8") for t in tr._pretokenize([f])] == uh.chunk_words(data, starts, mode, lambda b, st: s4.regex_split(b, 3, SP, st), nfc=True)
    assert tr.utf8_replaced == seen
    # a valid file: nothing is counted, the words are the strict ones
    clean = golden_dir / "corpus.en"
    tr = BBPETrainer(BBPETrainerConfig(errors=mode, **KW))
    assert tr._pretokenize([clean]) == BBPETrainer(BBPETrainerConfig(**KW))._pretokenize([clean]) and tr.utf8_replaced == 0


def test_inputs_of_the_gpu_test(corpus, golden_dir, monkeypatch):
    from oracle import oracle
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    f, data, starts = corpus
    assert len(data) == 134_042 and sum(a != b for a, b in zip(data, (golden_dir / "corpus.en").read_bytes())) > 200
    # strict raises at the first damaged position
    first = uh.reference(data, starts, "replace")[3]
    assert 0 <= first < 2 * uh.DAMAGE_RATE * 4 and uh.ill_formed(data[:first + 1]) and not uh.ill_formed(data[:first])
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    tr = BBPETrainer(BBPETrainerConfig(**KW))
    with pytest.raises(ValueError, match=rf"File .*{f.name} contains invalid UTF-8 at position {first}\."):
        tr.train([f])
    assert tr.utf8_replaced == 0
    # some chunk ends inside a sequence: its tail is ill-formed only because the chunk ends there
    cuts = starts + [len(data)]
    inside = 0
    for a, b in zip(cuts[:-2], cuts[1:-1]):
        bad = uh.subparts(data[a:b])
        inside += bool(bad) and data[a + bad[-1]:b] in (b"\xe2\x82", b"\xf0\x9f\x98", b"\xc3")
    assert inside >= 4
    # the three models differ: replace / ignore / the undamaged corpus (damage rate 1 in uh.DAMAGE_RATE)
    models = {mode: oracle.merge_loop(uh.chunk_words(data, starts, mode, split), KW["vocab_size"], 2, SP) for mode in uh.MODES}
    clean = (golden_dir / "corpus.en").read_bytes()
    clean_starts = [a for a, _ in BBPETrainer(BBPETrainerConfig(**KW))._chunk_ranges(golden_dir / "corpus.en")]
    models["clean"] = oracle.merge_loop(split(clean, clean_starts), KW["vocab_size"], 2, SP)
    assert all(len(m[1]) == 300 for m in models.values())
    assert models["replace"][1] != models["ignore"][1] != models["clean"][1] != models["replace"][1]
    assert any("�".encode() in l + r for l, r in models["replace"][1]) and not any("�".encode() in l + r for l, r in models["ignore"][1])
