"""CPU: normalizer="nfc" through the Python interface -- validation (names, a special that is not NFC), the host pre-tokeniser
against regex on unicodedata-normalised chunks, pretokenizer.json through save / from_file / from_file_lossless and the files
of models without a normaliser byte for byte as before, train_from's mismatch error, the plain-Python tokenizer:
encode(x) == encode(normalize(x)), other ids on NFD text without the normaliser, spans that refer to the normalised text.
No GPU: the model the tokenizer tests use comes from the CPU oracle."""
from __future__ import annotations

import json
import unicodedata as ud

import pytest

from tests import group_helpers as gh
from tests import nfc_helpers as nh
from tests import split4_helpers as s4

SP = ["<|e|>", "<a>", "[UNK]"]


@pytest.fixture(scope="module")
def trained(golden_dir):
    """(vocab, merges) of the CPU oracle on the NFC of the training text, pre-tokenised by regex with the GPT-2 pattern."""
    from oracle import oracle

    data = nh.training_text(golden_dir)
    return oracle.merge_loop(nh.normalized_words(data, [0], lambda b, st: gh.regex_split(b, 0, SP, st)), 256 + len(SP) + 300, 2, SP)


def test_validation(tmp_path):
    from yet_another_bpe import trainer as T
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.tokenizer import BBPETokenizer

    assert T.NORMALIZERS == (None, "nfc") and [T.check_normalizer(n) for n in T.NORMALIZERS] == [0, 1]
    assert T.BBPETrainerConfig().normalizer is None and T.BBPEModel({}, [], []).normalizer is None
    assert T.BBPEModel({}, [], [], normalizer="nfc").normalizer == "nfc"
    cfg = T.BBPETrainerConfig(normalizer="nfc", pretokenizer="cl100k", digit_group=1)
    assert T.pretokenizer(cfg) == (1, 1)
    assert T.device_options(cfg) == {"digit_group": 1, "split_pattern": 1}  # (the normaliser is a call, not an option)
    assert T.device_options(T.BBPETrainerConfig(normalizer="nfc")) == {}
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    for bad in ("NFC", "nfd", "nfkc", "", 1, True):
        with pytest.raises(ValueError, match="normalizer"):
            T.BBPETrainer(T.BBPETrainerConfig(normalizer=bad)).train([f])
        with pytest.raises(ValueError, match="normalizer"):
            T.BBPEModel({}, [], [], normalizer=bad)
        with pytest.raises(ValueError, match="normalizer"):
            BBPETokenizer({}, [], [], normalizer=bad)
    # a special token must itself be NFC
    for tok in ("<e\u0301>", "\u212b", "<\u1100\u1161>"):
        cfg = T.BBPETrainerConfig(normalizer="nfc", special_tokens=["<|e|>", tok])
        for call in (lambda: T.BBPETrainer(cfg).train([f]), lambda: T.BBPETrainer(cfg).train_from(T.BBPEModel({}, [], cfg.special_tokens, normalizer="nfc"), [f]),
                     lambda: train_text_sharded(None, [f], cfg, 0, 1), lambda: BBPETokenizer({}, [], ["<|e|>", tok], normalizer="nfc")):
            with pytest.raises(ValueError, match="not in NFC"):
                call()
        assert T.BBPETrainer(T.BBPETrainerConfig(special_tokens=[tok]))._split_pattern()  # without a normaliser it is taken as before
        assert BBPETokenizer({}, [], [tok]).special_tokens == [tok]
    assert T.BBPETrainer(T.BBPETrainerConfig(normalizer="nfc", special_tokens=["<\u00e9>", "<|e|>"]))._split_pattern()


def test_host_pretokenize_normalises_every_chunk(tmp_path, golden_dir):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = nh.training_text(golden_dir)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    for kw, split in ((dict(), lambda b, st: gh.regex_split(b, 0, SP, st)), (dict(pretokenizer="cl100k", digit_group=1), lambda b, st: s4.regex_split(b, 1, SP, st))):
        tr = BBPETrainer(BBPETrainerConfig(normalizer="nfc", special_tokens=SP, chunk_size_bytes=1 << 12, **kw))
        starts = [a for a, _ in tr._chunk_ranges(f)]
        assert len(starts) > 4
        got = [t.encode("utf-8") for t in tr._pretokenize([f])]
        assert got == nh.normalized_words(data, starts, split)
        plain = BBPETrainer(BBPETrainerConfig(special_tokens=SP, chunk_size_bytes=1 << 12, **kw))
        assert [t.encode("utf-8") for t in plain._pretokenize([f])] == split(data, starts) != got
    # a chunk cut between a base and its mark: the mark starts its chunk and stays a mark
    f.write_bytes("e\u0301".encode() * 40)
    tr = BBPETrainer(BBPETrainerConfig(normalizer="nfc", special_tokens=[], chunk_size_bytes=31))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    assert any(f.read_bytes()[a:a + 2] == "\u0301".encode() for a in starts)
    assert [t.encode() for t in tr._pretokenize([f])] == nh.normalized_words(f.read_bytes(), starts, lambda b, st: gh.regex_split(b, 0, (), st))


def test_save_and_reload(trained, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig, read_normalizer, read_pretokenizer

    vocab, merges = trained
    cases = ((dict(), {"normalizer": "nfc"}), (dict(digit_group=3), {"digit_group": 3, "normalizer": "nfc"}),
             (dict(pretokenizer="cl100k", digit_group=1), {"pattern": "cl100k", "digit_group": 1, "normalizer": "nfc"}))
    for k, (kw, want) in enumerate(cases):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, normalizer="nfc", **kw))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"text_{k}", tmp_path / f"hex_{k}"
        tr.save(a)
        tr.save_lossless(b)
        assert json.loads((a / "pretokenizer.json").read_text()) == want == json.loads((b / "pretokenizer.json").read_text())
        assert read_normalizer(a) == "nfc" and read_pretokenizer(a) == (kw.get("pretokenizer", "gpt2"), kw.get("digit_group"))
        for tok in (BBPETokenizer.from_file(a), BBPETokenizer.from_file_lossless(b)):
            assert tok.normalizer == "nfc" and tok.pretokenizer == kw.get("pretokenizer", "gpt2") and tok.digit_group == kw.get("digit_group")
        model = BBPEModel.from_file_lossless(b)
        assert model.normalizer == "nfc" and model.vocab == vocab and model.merges == merges
    # saving a model without a normaliser over one with it leaves no stale setting behind
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP))
    tr._vocab, tr._merges = dict(vocab), list(merges)
    tr.save_lossless(tmp_path / "hex_0")
    assert not (tmp_path / "hex_0" / "pretokenizer.json").exists()
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_0").normalizer is None and read_normalizer(tmp_path / "hex_0") is None
    (tmp_path / "hex_0" / "pretokenizer.json").write_text('{"normalizer": "nfkc"}')
    with pytest.raises(ValueError, match="normalizer"):
        BBPETokenizer.from_file_lossless(tmp_path / "hex_0")


def test_files_without_a_normaliser_are_written_as_before(trained, tmp_path):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig, read_normalizer

    vocab, merges = trained
    cases = ((dict(), None), (dict(digit_group=3), b'{"digit_group": 3}'), (dict(pretokenizer="cl100k"), b'{"pattern": "cl100k", "digit_group": 3}'),
             (dict(pretokenizer="o200k_base", digit_group=1), b'{"pattern": "o200k_base", "digit_group": 1}'))
    for k, (kw, pre_json) in enumerate(cases):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, **kw))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"t{k}", tmp_path / f"h{k}"
        tr.save(a)
        tr.save_lossless(b)
        extra = [] if pre_json is None else ["pretokenizer.json"]
        assert sorted(p.name for p in a.iterdir()) == sorted(["merges.txt", "special_tokens.json", "vocab.json"] + extra)
        assert sorted(p.name for p in b.iterdir()) == sorted(["merges.hex", "special_tokens.json", "vocab.hex.json"] + extra)
        if pre_json is not None:
            assert (a / "pretokenizer.json").read_bytes() == pre_json == (b / "pretokenizer.json").read_bytes()
        assert read_normalizer(a) is None


def test_train_from_refuses_another_normaliser(trained, tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    f = tmp_path / "more.txt"
    f.write_text("12345 more text 678")
    with pytest.raises(ValueError, match="normalizer = None"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, normalizer="nfc", vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP), [f])
    with pytest.raises(ValueError, match="normalizer = 'nfc'"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP, normalizer="nfc"), [f])
    # the same normaliser and no budget left: the model comes back unchanged, normaliser included (no device call)
    same = BBPETrainer(BBPETrainerConfig(special_tokens=SP, normalizer="nfc", vocab_size=len(vocab))).train_from(BBPEModel(vocab, merges, SP, normalizer="nfc"), [f])
    assert same.normalizer == "nfc" and same.merges == merges and same.vocab == vocab


def test_tokenizer_plain_python(trained):
    from yet_another_bpe.tokenizer import BBPETokenizer

    vocab, merges = trained
    tok, plain = BBPETokenizer(vocab, merges, SP, normalizer="nfc"), BBPETokenizer(vocab, merges, SP)
    assert tok.normalizer == "nfc" and plain.normalizer is None
    differs = 0
    for text in nh.ENCODE_TEXTS:
        norm = ud.normalize("NFC", text)
        assert tok.normalize(text) == norm and plain.normalize(text) == text
        ids = tok.encode(text)
        assert ids == tok.encode(norm) == plain.encode(norm)
        differs += plain.encode(text) != ids
        assert tok.encode_dropout(text, 0.0, seed=5) == ids
        assert tok.encode_dropout(text, 0.3, seed=5) == plain.encode_dropout(norm, 0.3, seed=5)
        for unit in ("byte", "char"):  # the spans refer to the normalised document
            got_ids, spans = tok.encode_with_offsets(text, unit)
            assert (got_ids, spans) == plain.encode_with_offsets(norm, unit) and got_ids == ids
            if spans:
                assert spans[-1][1] <= (len(norm.encode()) if unit == "byte" else len(norm))
    assert differs >= 5  # (NFD text, jamo and singletons encode to other ids without the normaliser)
    nfd = ud.normalize("NFD", "caf\u00e9 d\u00e9j\u00e0")
    assert plain.encode(nfd) != plain.encode(ud.normalize("NFC", nfd)) and tok.encode(nfd) == tok.encode(ud.normalize("NFC", nfd))
    # a special followed by U+0338 is no special after normalisation
    e = vocab["<|e|>".encode()]
    assert tok.encode("<|e|>") == [e] and e not in tok.encode("<|e|>\u0338") and e in plain.encode("<|e|>\u0338")
    assert tok.encode_batch(nh.ENCODE_TEXTS) == [plain.encode(ud.normalize("NFC", t)) for t in nh.ENCODE_TEXTS]
    short = nh.ENCODE_TEXTS[:6]
    assert tok.encode_batch_padded(short, 16, bos_id=1) == plain.encode_batch_padded([ud.normalize("NFC", t) for t in short], 16, bos_id=1)
    assert tok.encode_batch_packed(short, 24, eos_id=2, dropout=0.2, seed=3) == plain.encode_batch_packed([ud.normalize("NFC", t) for t in short], 24, eos_id=2, dropout=0.2, seed=3)
