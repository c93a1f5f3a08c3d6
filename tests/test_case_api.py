"""CPU: lowercase=True through the Python interface -- validation (a bool and nothing else, a special that is not lower case, the
default specials), the host pre-tokeniser against regex on lowered chunks, alone and with "nfc" and errors="replace",
pretokenizer.json through save / from_file / from_file_lossless and the files of models without the setting byte for byte as
before, train_from's mismatch error, the plain-Python tokenizer: encode(x) == encode(normalize(x)), spans that refer to the
lowered text.  No GPU: the model the tokenizer tests use comes from the CPU oracle."""
from __future__ import annotations

import json
import unicodedata as ud

import pytest

from tests import case_helpers as ch
from tests import group_helpers as gh
from tests import split4_helpers as s4

SP = ["<|e|>", "<a>", "[unk]"]


@pytest.fixture(scope="module")
def trained(golden_dir):
    """(vocab, merges) of the CPU oracle on the lowered training text, pre-tokenised by regex with the GPT-2 pattern."""
    from oracle import oracle

    data = ch.training_text(golden_dir)
    return oracle.merge_loop(ch.lowered_words(data, [0], lambda b, st: gh.regex_split(b, 0, SP, st)), 256 + len(SP) + 300, 2, SP)


def test_validation(tmp_path):
    from yet_another_bpe import trainer as T
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.tokenizer import BBPETokenizer

    assert T.BBPETrainerConfig().lowercase is False and T.BBPEModel({}, [], []).lowercase is False and BBPETokenizer().lowercase is False
    assert T.BBPEModel({}, [], [], None, "gpt2", None, True).lowercase is True  # (the keyword after normalizer)
    assert T.NORMALIZERS == (None, "nfc")  # (the normaliser's list did not grow: lowercase is a setting of its own)
    cfg = T.BBPETrainerConfig(lowercase=True, special_tokens=SP, pretokenizer="cl100k", digit_group=1)
    assert T.pretokenizer(cfg) == (1, 1)
    assert T.device_options(cfg) == {"digit_group": 1, "split_pattern": 1}  # (the step is a call, not an option)
    assert T.device_options(T.BBPETrainerConfig(lowercase=True, special_tokens=SP)) == {} == T.device_options(T.BBPETrainerConfig())
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    for bad in (1, 0, "true", "", None):
        with pytest.raises(ValueError, match="lowercase must be True or False"):
            T.BBPETrainer(T.BBPETrainerConfig(lowercase=bad, special_tokens=SP)).train([f])
        with pytest.raises(ValueError, match="lowercase"):
            T.BBPEModel({}, [], [], lowercase=bad)
        with pytest.raises(ValueError, match="lowercase"):
            BBPETokenizer({}, [], [], lowercase=bad)
        with pytest.raises(ValueError, match="lowercase"):
            train_text_sharded(None, [f], T.BBPETrainerConfig(lowercase=bad, special_tokens=SP), 0, 1)
    # a special token must itself be lower case; the error names it and says what to do about the default ones
    for tok in ("<|E|>", "[UNK]", "<\u00c9>", "<\u03a3>", "\u0130"):
        cfg = T.BBPETrainerConfig(lowercase=True, special_tokens=["<|e|>", tok])
        for call in (lambda: T.BBPETrainer(cfg).train([f]), lambda: T.BBPETrainer(cfg).train_from(T.BBPEModel({}, [], cfg.special_tokens, lowercase=True), [f]),
                     lambda: train_text_sharded(None, [f], cfg, 0, 1), lambda: BBPETokenizer({}, [], ["<|e|>", tok], lowercase=True)):
            with pytest.raises(ValueError, match="not lower case") as e:
                call()
            assert repr(tok) in str(e.value) and "[PAD], [UNK], [BOS], [EOS]" in str(e.value) and "lower-case ones" in str(e.value)
        assert T.BBPETrainer(T.BBPETrainerConfig(special_tokens=[tok]))._split_pattern()  # without the setting it is taken as before
        assert BBPETokenizer({}, [], [tok]).special_tokens == [tok]
    with pytest.raises(ValueError, match=r"'\[PAD\]' is not lower case"):  # the default specials
        T.BBPETrainer(T.BBPETrainerConfig(lowercase=True)).train([f])
    assert T.BBPETrainer(T.BBPETrainerConfig(lowercase=True, special_tokens=["[pad]", "<\u00e9>", "\u03c2"]))._split_pattern()
    # with "nfc" the existing check applies too
    with pytest.raises(ValueError, match="not in NFC"):
        T.BBPETrainer(T.BBPETrainerConfig(lowercase=True, normalizer="nfc", special_tokens=["<e\u0301>"])).train([f])
    assert T.lowercase_text("\u0130A", True) == "i\u0307a" and T.lowercase_text("\u0130A", False) == "\u0130A"


def test_host_pretokenize_lowers_every_chunk(tmp_path, golden_dir):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = ch.training_text(golden_dir)
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    for kw, split in ((dict(), lambda b, st: gh.regex_split(b, 0, SP, st)), (dict(pretokenizer="cl100k", digit_group=1), lambda b, st: s4.regex_split(b, 1, SP, st))):
        for normalizer in (None, "nfc"):
            tr = BBPETrainer(BBPETrainerConfig(lowercase=True, normalizer=normalizer, special_tokens=SP, chunk_size_bytes=1 << 12, **kw))
            starts = [a for a, _ in tr._chunk_ranges(f)]
            assert len(starts) > 4
            got = [t.encode("utf-8") for t in tr._pretokenize([f])]
            assert got == ch.lowered_words(data, starts, split, nfc=normalizer == "nfc")
            plain = BBPETrainer(BBPETrainerConfig(normalizer=normalizer, special_tokens=SP, chunk_size_bytes=1 << 12, **kw))
            assert [t.encode("utf-8") for t in plain._pretokenize([f])] != got
    # a chunk cut behind a sigma: final by the chunk's end, whatever the next chunk begins with
    f.write_bytes(("\u0391\u03a3" * 70).encode())
    tr = BBPETrainer(BBPETrainerConfig(lowercase=True, special_tokens=[], chunk_size_bytes=28))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    raw = f.read_bytes()
    assert any(raw[a - 2:a] == ch.SIGMA.encode() and raw[a:a + 2] == "\u0391".encode() for a in starts[1:])
    got = [t.encode() for t in tr._pretokenize([f])]
    assert got == ch.lowered_words(raw, starts, lambda b, st: gh.regex_split(b, 0, (), st))
    assert b"".join(got) != raw.decode().lower().encode()  # (lowered as one text, those sigmas are not final)
    # errors="replace" in front of it: the repaired chunk is lowered
    f.write_bytes("\u00c9\u03a3 OK ".encode() * 50 + b"\xff\xc3 TAIL\xce")
    tr = BBPETrainer(BBPETrainerConfig(lowercase=True, normalizer="nfc", errors="replace", special_tokens=SP, chunk_size_bytes=64))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    raw = f.read_bytes()
    cuts = starts + [len(raw)]
    exp = [ud.normalize("NFC", raw[a:b].decode("utf-8", "replace").lower()) for a, b in zip(cuts[:-1], cuts[1:])]
    assert "".join(tr._pretokenize([f])) == "".join(exp) and tr.utf8_replaced == 3


def test_save_and_reload(trained, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig, read_lowercase, read_normalizer, read_pretokenizer

    vocab, merges = trained
    cases = ((dict(), {"lowercase": True}), (dict(digit_group=3), {"digit_group": 3, "lowercase": True}),
             (dict(normalizer="nfc"), {"normalizer": "nfc", "lowercase": True}),
             (dict(pretokenizer="cl100k", digit_group=1, normalizer="nfc"), {"pattern": "cl100k", "digit_group": 1, "normalizer": "nfc", "lowercase": True}))
    for k, (kw, want) in enumerate(cases):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, lowercase=True, **kw))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"text_{k}", tmp_path / f"hex_{k}"
        tr.save(a)
        tr.save_lossless(b)
        assert json.loads((a / "pretokenizer.json").read_text()) == want == json.loads((b / "pretokenizer.json").read_text())
        assert '"lowercase": true' in (a / "pretokenizer.json").read_text()
        assert read_lowercase(a) is True and read_normalizer(a) == kw.get("normalizer")
        assert read_pretokenizer(a) == (kw.get("pretokenizer", "gpt2"), kw.get("digit_group"))
        for tok in (BBPETokenizer.from_file(a), BBPETokenizer.from_file_lossless(b)):
            assert tok.lowercase is True and tok.normalizer == kw.get("normalizer") and tok.pretokenizer == kw.get("pretokenizer", "gpt2")
        model = BBPEModel.from_file_lossless(b)
        assert model.lowercase is True and model.vocab == vocab and model.merges == merges
    # saving a model without the setting over one with it leaves no stale setting behind
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP))
    tr._vocab, tr._merges = dict(vocab), list(merges)
    tr.save_lossless(tmp_path / "hex_0")
    assert not (tmp_path / "hex_0" / "pretokenizer.json").exists()
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_0").lowercase is False and read_lowercase(tmp_path / "hex_0") is False
    # anything but a JSON boolean there is refused by every reader
    for bad in ('1', '"true"', 'null', '0'):
        for d, loaders in ((tmp_path / "hex_0", (BBPETokenizer.from_file_lossless, BBPEModel.from_file_lossless)), (tmp_path / "text_0", (BBPETokenizer.from_file,))):
            (d / "pretokenizer.json").write_text('{"lowercase": %s}' % bad)
            for load in loaders:
                with pytest.raises(ValueError, match="lowercase"):
                    load(d)
    (tmp_path / "hex_0" / "pretokenizer.json").write_text('{"lowercase": false}')
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_0").lowercase is False


def test_files_without_the_setting_are_written_as_before(trained, tmp_path):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig, read_lowercase

    vocab, merges = trained
    cases = ((dict(), None), (dict(digit_group=3), b'{"digit_group": 3}'), (dict(pretokenizer="cl100k"), b'{"pattern": "cl100k", "digit_group": 3}'),
             (dict(pretokenizer="o200k_base", digit_group=1), b'{"pattern": "o200k_base", "digit_group": 1}'),
             (dict(normalizer="nfc"), b'{"normalizer": "nfc"}'), (dict(digit_group=2, normalizer="nfc"), b'{"digit_group": 2, "normalizer": "nfc"}'))
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
        assert read_lowercase(a) is False


def test_train_from_refuses_another_setting(trained, tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    f = tmp_path / "more.txt"
    f.write_text("12345 More Text 678")
    with pytest.raises(ValueError, match="cannot continue from this model: it was trained with lowercase = False, the trainer's is True"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, lowercase=True, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP), [f])
    with pytest.raises(ValueError, match="cannot continue from this model: it was trained with lowercase = True, the trainer's is False"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP, lowercase=True), [f])
    # the same setting and no budget left: the model comes back unchanged, setting included (no device call)
    same = BBPETrainer(BBPETrainerConfig(special_tokens=SP, lowercase=True, vocab_size=len(vocab))).train_from(BBPEModel(vocab, merges, SP, lowercase=True), [f])
    assert same.lowercase is True and same.merges == merges and same.vocab == vocab


def test_tokenizer_plain_python(trained):
    from yet_another_bpe.tokenizer import BBPETokenizer

    vocab, merges = trained
    tok, plain = BBPETokenizer(vocab, merges, SP, lowercase=True), BBPETokenizer(vocab, merges, SP)
    both = BBPETokenizer(vocab, merges, SP, normalizer="nfc", lowercase=True)
    assert tok.lowercase is True and plain.lowercase is False
    differs = 0
    for text in ch.ENCODE_TEXTS + ch.SIGMAS + ch.GROW + ch.SHRINK:
        low = text.lower()
        assert tok.normalize(text) == low and plain.normalize(text) == text and both.normalize(text) == ud.normalize("NFC", low)
        assert both.normalize(both.normalize(text)) == both.normalize(text)  # lower-then-NFC is idempotent
        ids = tok.encode(text)
        assert ids == tok.encode(low) == plain.encode(low)
        assert both.encode(text) == both.encode(both.normalize(text)) == plain.encode(ud.normalize("NFC", low))
        differs += plain.encode(text) != ids
        assert tok.encode_dropout(text, 0.0, seed=5) == ids
        assert tok.encode_dropout(text, 0.3, seed=5) == plain.encode_dropout(low, 0.3, seed=5)
        for unit in ("byte", "char"):  # the spans refer to the lowered document
            got_ids, spans = tok.encode_with_offsets(text, unit)
            assert (got_ids, spans) == plain.encode_with_offsets(low, unit) and got_ids == ids
            if spans:
                assert spans[-1][1] <= (len(low.encode()) if unit == "byte" else len(low))
    assert differs >= 10
    # a special is matched in the lowered text; the b"[UNK]" lookup stays as it is
    e = vocab["<|e|>".encode()]
    assert tok.encode("<|E|>") == [e] == tok.encode("<|e|>") and plain.encode("<|E|>") != [e]
    assert tok.encode_batch(ch.ENCODE_TEXTS) == [plain.encode(t.lower()) for t in ch.ENCODE_TEXTS]
    short = ch.ENCODE_TEXTS[:6]
    assert tok.encode_batch_padded(short, 16, bos_id=1) == plain.encode_batch_padded([t.lower() for t in short], 16, bos_id=1)
    assert tok.encode_batch_packed(short, 24, eos_id=2, dropout=0.2, seed=3) == plain.encode_batch_packed([t.lower() for t in short], 24, eos_id=2, dropout=0.2, seed=3)
    assert tok.decode(tok.encode("Hello \u0130")) == "hello i\u0307"  # decoding is untouched: it gives the lowered text
