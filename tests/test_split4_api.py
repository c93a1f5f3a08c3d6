"""CPU: pretokenizer="cl100k" through the Python interface -- BBPETrainerConfig validation and the two refusals, the host
pre-tokeniser and the plain-Python tokenizer against regex.findall with the pattern, pretokenizer.json through save /
from_file / from_file_lossless, GPT-2 models saved byte for byte as before, and train_from's mismatch error.  No GPU: the
model the tokenizer tests use comes from the CPU oracle."""
from __future__ import annotations

import json

import pytest
import regex

from tests import group_helpers as gh
from tests import split4_helpers as sh

SP = ["<|e|>", "<a>", "[UNK]"]
TEXTS = ["I'M sure THEY'LL say it's fine; we'Ve 12345 of them", "def f(x):\n    return x**2  # ok\n\n\n", "a\r\n  b<|e|>\n \n x<a>'s", "…a<a>😀a .a ..a\ta a",
         " 12 1234567", ".\n\n \nx", "\n\n \n x", "no change here", "x", ""]


@pytest.fixture(scope="module")
def trained(golden_dir):
    """(vocab, merges) of the CPU oracle on the multilingual text, pre-tokenised by regex with the cl100k pattern, G = 3."""
    from oracle import oracle

    return oracle.merge_loop(sh.regex_split(sh.multilingual(golden_dir), 3, SP), 256 + len(SP) + 300, 2, SP)


def test_config_validation(tmp_path):
    from yet_another_bpe import trainer as T

    assert T.BBPETrainerConfig().pretokenizer == "gpt2" and T.pretokenizer(T.BBPETrainerConfig()) == (0, 0)
    assert T.pretokenizer(T.BBPETrainerConfig(pretokenizer="cl100k")) == (1, 3) == (1, T.digit_group(T.BBPETrainerConfig(pretokenizer="cl100k")))
    assert T.pretokenizer(T.BBPETrainerConfig(pretokenizer="cl100k", digit_group=1)) == (1, 1)
    assert T.pretokenizer(T.BBPETrainerConfig(pretokenizer="gpt2", digit_group=2)) == (0, 2)
    assert T.split_pattern(3, "cl100k") == T.split_pattern(None, "cl100k") == sh.pattern(3) and T.split_pattern(1, "cl100k") == sh.pattern(1)
    assert T.split_pattern() == gh.grouped_pattern(0) and T.split_pattern(3) == gh.grouped_pattern(3)
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    for bad in ("CL100K", "gpt4", "", None, 1, b"cl100k"):
        with pytest.raises(ValueError, match="pretokenizer"):
            T.BBPETrainer(T.BBPETrainerConfig(pretokenizer=bad)).train([f])
        with pytest.raises(ValueError, match="pretokenizer"):
            T.BBPETrainer(T.BBPETrainerConfig(pretokenizer=bad))._split_pattern()
        with pytest.raises(ValueError, match="pretokenizer"):
            T.BBPEModel({}, [], [], pretokenizer=bad)
    for bad in (0, 256, True):
        with pytest.raises(ValueError, match="digit_group"):
            T.BBPETrainer(T.BBPETrainerConfig(pretokenizer="cl100k", digit_group=bad)).train([f])


def test_the_two_refusals(tmp_path):
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    f = tmp_path / "never_read.txt"
    for tok, what in ((" x", "whitespace"), ("\nx", "whitespace"), ("　", "whitespace"), (" a", "whitespace"), ("7x", "digit"), ("²", "digit")):
        cfg = BBPETrainerConfig(pretokenizer="cl100k", special_tokens=["<|e|>", tok])
        with pytest.raises(ValueError, match=what):
            BBPETrainer(cfg).train([f])
        with pytest.raises(ValueError, match=what):
            BBPETrainer(cfg).train_from(BBPEModel({}, [], cfg.special_tokens, 3, "cl100k"), [f])
        with pytest.raises(ValueError, match=what):
            train_text_sharded(None, [f], cfg, 0, 1)
    assert BBPETrainer(BBPETrainerConfig(special_tokens=[" x", "\nx"]))._split_pattern()  # the GPT-2 pattern: as before
    for tok in ("x ", "<7", "<\n>", "'s", "…"):
        assert BBPETrainer(BBPETrainerConfig(pretokenizer="cl100k", special_tokens=[tok]))._split_pattern()


def test_host_pretokenize_against_regex(tmp_path, golden_dir):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = sh.multilingual(golden_dir) + "\n".join(sh.EDGE + sh.BEHIND_SPECIAL).encode("utf-8")
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    for G in (None, 1, 3):
        for sp in ([], ["<>", "<a>", "'s"]):
            tr = BBPETrainer(BBPETrainerConfig(pretokenizer="cl100k", digit_group=G, special_tokens=sp))
            got = tr._pretokenize([f])
            assert [t.encode("utf-8") for t in got] == sh.regex_split(data, G or 3, sp)
            assert tr._preprocess_corpus([f]) == [list(t.encode("utf-8")) for t in got]
    f.write_bytes(b"a\n  \n  b " * 30)  # chunks are texts of their own: a cut inside a whitespace run starts anew
    tr = BBPETrainer(BBPETrainerConfig(pretokenizer="cl100k", special_tokens=[], chunk_size_bytes=61))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    assert len(starts) == 5 and [t.encode() for t in tr._pretokenize([f])] == sh.regex_split(b"a\n  \n  b " * 30, 3, (), starts)


def _reference_encode(tok, text: str, G: int):
    """encode restated: the special split, regex.findall with the pattern, the tokenizer's own word merge"""
    pat = regex.compile(sh.pattern(G))
    sp = sorted(tok.special_tokens, key=len, reverse=True)
    parts = regex.split("(" + "|".join(regex.escape(t) for t in sp) + ")", text) if sp else [text]
    ids, pieces = [], []
    for part in parts:
        if part in sp:
            ids.append(tok._vocab[part.encode("utf-8")])
            pieces.append(part.encode("utf-8"))
        else:
            for pre in pat.findall(part):
                ids += tok._encode_word(pre)
                pieces.append(pre.encode("utf-8"))
    return ids, pieces


def test_tokenizer_plain_python(trained):
    from yet_another_bpe.tokenizer import BBPETokenizer

    vocab, merges = trained
    plain = BBPETokenizer(vocab, merges, SP)
    assert plain.pretokenizer == "gpt2" and plain.digit_group is None
    differs = 0
    for G in (None, 1):
        tok = BBPETokenizer(vocab, merges, SP, digit_group=G, pretokenizer="cl100k")
        assert tok.pretokenizer == "cl100k" and tok.digit_group == (G or 3)
        for text in TEXTS:
            ids, pieces = _reference_encode(tok, text, G or 3)
            assert tok.encode(text) == ids and tok.decode(ids) == text
            differs += tok.encode(text) != plain.encode(text)
            data = text.encode("utf-8")
            got_ids, spans = tok.encode_with_offsets(text, unit="byte")  # the spans tile the text, no token crosses a pre-token cut
            assert got_ids == ids and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))
            assert not data or (spans[0][0] == 0 and spans[-1][1] == len(data))
            cuts, pos = set(), 0
            for p in pieces:
                cuts.add(pos)
                pos += len(p)
            assert all(not any(s < c < e for c in cuts) for s, e in spans)
            char_ids, char_spans = tok.encode_with_offsets(text, unit="char")
            assert char_ids == ids and (not text or (char_spans[0][0] == 0 and char_spans[-1][1] == len(text)))
            assert tok.encode_dropout(text, 0.0, seed=5) == ids
            every_byte = [i for p in pieces for i in ([vocab[p]] if p.decode() in SP else [vocab[bytes([b])] for b in p])]
            assert tok.encode_dropout(text, 1.0, seed=5) == every_byte
        rows, lengths = tok.encode_batch_padded(TEXTS[:3])
        assert [r[:n] for r, n in zip(rows, lengths)] == [tok.encode(t) for t in TEXTS[:3]]
    assert differs  # (the pattern changes the ids of these texts: the tests above are not vacuous)
    for bad in ("gpt4", None, 1):
        with pytest.raises(ValueError, match="pretokenizer"):
            BBPETokenizer(vocab, merges, SP, pretokenizer=bad)


def test_save_and_reload(trained, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    for G in (None, 1):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=G, pretokenizer="cl100k"))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"text_{G}", tmp_path / f"hex_{G}"
        tr.save(a)
        tr.save_lossless(b)
        want = {"pattern": "cl100k", "digit_group": G or 3}
        assert json.loads((a / "pretokenizer.json").read_text()) == want == json.loads((b / "pretokenizer.json").read_text())
        for tok in (BBPETokenizer.from_file(a), BBPETokenizer.from_file_lossless(b)):
            assert tok.pretokenizer == "cl100k" and tok.digit_group == (G or 3)
        model = BBPEModel.from_file_lossless(b)
        assert model.pretokenizer == "cl100k" and model.digit_group == (G or 3) and model.vocab == vocab and model.merges == merges
        tok = BBPETokenizer.from_file_lossless(b)
        for text in TEXTS:
            assert tok.encode(text) == BBPETokenizer(vocab, merges, SP, digit_group=G, pretokenizer="cl100k").encode(text)
    # a file that names the pattern alone means three digits; one that names an unknown pattern is refused
    (tmp_path / "hex_1" / "pretokenizer.json").write_text('{"pattern": "cl100k"}')
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_1").digit_group == 3
    (tmp_path / "hex_1" / "pretokenizer.json").write_text('{"pattern": "o200k", "digit_group": 3}')
    with pytest.raises(ValueError, match="pretokenizer"):
        BBPETokenizer.from_file_lossless(tmp_path / "hex_1")
    # saving a GPT-2 model over a cl100k one leaves no stale file behind
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP))
    tr._vocab, tr._merges = dict(vocab), list(merges)
    tr.save_lossless(tmp_path / "hex_None")
    tok = BBPETokenizer.from_file_lossless(tmp_path / "hex_None")
    assert tok.pretokenizer == "gpt2" and tok.digit_group is None


def test_gpt2_models_are_saved_byte_for_byte_as_before(trained, tmp_path):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    for G, pre_json in ((None, None), (3, b'{"digit_group": 3}')):
        dirs = []
        for k, cfg in enumerate((BBPETrainerConfig(special_tokens=SP, digit_group=G), BBPETrainerConfig(special_tokens=SP, digit_group=G, pretokenizer="gpt2"))):
            tr = BBPETrainer(cfg)
            tr._vocab, tr._merges = dict(vocab), list(merges)
            a, b = tmp_path / f"t{G}{k}", tmp_path / f"h{G}{k}"
            tr.save(a)
            tr.save_lossless(b)
            dirs.append((a, b))
        extra = [] if pre_json is None else ["pretokenizer.json"]
        for a, b in dirs:
            assert sorted(p.name for p in a.iterdir()) == sorted(["merges.txt", "special_tokens.json", "vocab.json"] + extra)
            assert sorted(p.name for p in b.iterdir()) == sorted(["merges.hex", "special_tokens.json", "vocab.hex.json"] + extra)
            if pre_json is not None:  # the file's bytes as the digit-group release wrote them
                assert (a / "pretokenizer.json").read_bytes() == pre_json == (b / "pretokenizer.json").read_bytes()
        for x, y in zip(dirs[0], dirs[1]):
            for p in x.iterdir():
                assert p.read_bytes() == (y / p.name).read_bytes()


def test_train_from_refuses_another_pattern(trained, tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    f = tmp_path / "more.txt"
    f.write_text("12345 more text 678")

    class Bare:  # anything with .vocab, .merges, .special_tokens: no pretokenizer means "gpt2"
        def __init__(self):
            self.vocab, self.merges, self.special_tokens = vocab, merges, SP

    cl = BBPETrainerConfig(special_tokens=SP, pretokenizer="cl100k", vocab_size=2000)
    with pytest.raises(ValueError, match="pretokenizer"):
        BBPETrainer(cl).train_from(BBPEModel(vocab, merges, SP, 3), [f])
    with pytest.raises(ValueError, match="pretokenizer"):
        BBPETrainer(cl).train_from(Bare(), [f])
    with pytest.raises(ValueError, match="pretokenizer"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=3, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP, 3, "cl100k"), [f])
    with pytest.raises(ValueError, match="digit_group"):
        BBPETrainer(cl).train_from(BBPEModel(vocab, merges, SP, 1, "cl100k"), [f])
    # the same pattern and no budget left: the model comes back unchanged, pattern included (no device call)
    same = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="cl100k", vocab_size=len(vocab))).train_from(BBPEModel(vocab, merges, SP, None, "cl100k"), [f])
    assert same.pretokenizer == "cl100k" and same.digit_group == 3 and same.merges == merges and same.vocab == vocab
