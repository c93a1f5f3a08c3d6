"""CPU: pretokenizer="o200k_base" through the Python interface -- names, defaults and validation, the special refusals, the
host pre-tokeniser and the plain-Python tokenizer against regex.findall with the pattern, pretokenizer.json through save /
from_file / from_file_lossless, GPT-2 and cl100k models saved as before, and train_from's mismatch error.  No GPU: the model
the tokenizer tests use comes from the CPU oracle."""
from __future__ import annotations

import json

import pytest
import regex

from tests import group_helpers as gh
from tests import split4_helpers as s4
from tests import split5_helpers as sh

SP = ["<|e|>", "<a>", "[UNK]"]
TEXTS = ["I'M sure THEY'LL say it's fine; we'Ve 12345 of them", "def fooBar(x):\n    return XMLHttpRequest(x)**2  # ok\n\n\n", "a\r\n  b<|e|>\n \n x<a>'s", "…a<a>😀a .a ..a\ta a",
         " 12 1234567", "see https://example.org/a/b.html\n//c\n/p", "HTTPServer fooBar FOObarBAZ ab's's's", "ABCアDE don'tknow 'tis", "no change here", "x", ""]


@pytest.fixture(scope="module")
def trained(golden_dir):
    """(vocab, merges) of the CPU oracle on the multilingual text, pre-tokenised by regex with the o200k_base pattern, G = 3."""
    from oracle import oracle

    return oracle.merge_loop(sh.regex_split(sh.multilingual(golden_dir), 3, SP), 256 + len(SP) + 300, 2, SP)


def test_names_defaults_and_validation(tmp_path):
    from yet_another_bpe import trainer as T

    assert T.PRETOKENIZERS == ("gpt2", "cl100k", "o200k_base")
    assert [T.check_pretokenizer(n) for n in T.PRETOKENIZERS] == [0, 1, 3]  # 2 is reserved: the library refuses it
    cfg = T.BBPETrainerConfig(pretokenizer="o200k_base")
    assert T.pretokenizer(cfg) == (3, 3) == (3, T.digit_group(cfg))
    assert T.pretokenizer(T.BBPETrainerConfig(pretokenizer="o200k_base", digit_group=1)) == (3, 1)
    assert T.device_options(cfg) == {"digit_group": 3, "split_pattern": 3}
    assert T.device_options(T.BBPETrainerConfig(pretokenizer="cl100k")) == {"digit_group": 3, "split_pattern": 1}
    assert T.device_options(T.BBPETrainerConfig()) == {}
    assert T.split_pattern(3, "o200k_base") == T.split_pattern(None, "o200k_base") == sh.pattern(3) and T.split_pattern(1, "o200k_base") == sh.pattern(1)
    assert T.split_pattern(None, "cl100k") == s4.pattern(3) and T.split_pattern() == gh.grouped_pattern(0) and T.split_pattern(3) == gh.grouped_pattern(3)
    m = T.BBPEModel({}, [], [], pretokenizer="o200k_base")
    assert m.pretokenizer == "o200k_base" and m.digit_group == 3
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    for bad in ("o200k", "O200K_BASE", "o200k-base", "gpt4", "gpt4o", 3, 2):
        with pytest.raises(ValueError, match="pretokenizer"):
            T.BBPETrainer(T.BBPETrainerConfig(pretokenizer=bad)).train([f])
        with pytest.raises(ValueError, match="pretokenizer"):
            T.BBPEModel({}, [], [], pretokenizer=bad)
    for bad in (0, 256, True):
        with pytest.raises(ValueError, match="digit_group"):
            T.BBPETrainer(T.BBPETrainerConfig(pretokenizer="o200k_base", digit_group=bad)).train([f])


def test_the_special_refusals(tmp_path):
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    f = tmp_path / "never_read.txt"
    what = {"contains": "contains", "suffix": "begins special token", "whitespace": "whitespace", "digit": "digit"}
    for sp, why in sh.REFUSED_SETS:
        cfg = BBPETrainerConfig(pretokenizer="o200k_base", special_tokens=["<|e|>"] + sp)
        with pytest.raises(ValueError, match=what[why]):
            BBPETrainer(cfg).train([f])
        with pytest.raises(ValueError, match=what[why]):
            BBPETrainer(cfg).train_from(BBPEModel({}, [], cfg.special_tokens, 3, "o200k_base"), [f])
        with pytest.raises(ValueError, match=what[why]):
            train_text_sharded(None, [f], cfg, 0, 1)
        if why in ("contains", "suffix"):  # the other two patterns take such sets as before
            assert BBPETrainer(BBPETrainerConfig(pretokenizer="cl100k", special_tokens=sp))._split_pattern()
            assert BBPETrainer(BBPETrainerConfig(special_tokens=sp))._split_pattern()
    for sp in sh.ACCEPTED_SETS:
        assert BBPETrainer(BBPETrainerConfig(pretokenizer="o200k_base", special_tokens=sp))._split_pattern()
    assert BBPETrainer(BBPETrainerConfig(pretokenizer="o200k_base"))._split_pattern()  # the default specials pass


def test_host_pretokenize_against_regex(tmp_path, golden_dir):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = sh.multilingual(golden_dir) + "\n".join(sh.EDGE + sh.BEHIND_SPECIAL).encode("utf-8")
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    for G in (None, 1, 3):
        for sp in ([], ["<>", "<a>", "'s"]):
            tr = BBPETrainer(BBPETrainerConfig(pretokenizer="o200k_base", digit_group=G, special_tokens=sp))
            got = tr._pretokenize([f])
            assert [t.encode("utf-8") for t in got] == sh.regex_split(data, G or 3, sp)
            assert tr._preprocess_corpus([f]) == [list(t.encode("utf-8")) for t in got]
    f.write_bytes(b"fooBarBAZ's\n/x " * 30)  # chunks are texts of their own: a cut inside a word starts anew
    tr = BBPETrainer(BBPETrainerConfig(pretokenizer="o200k_base", special_tokens=[], chunk_size_bytes=61))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    assert len(starts) > 4 and [t.encode() for t in tr._pretokenize([f])] == sh.regex_split(b"fooBarBAZ's\n/x " * 30, 3, (), starts)


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
    others = [BBPETokenizer(vocab, merges, SP), BBPETokenizer(vocab, merges, SP, pretokenizer="cl100k")]
    differs = [0, 0]
    for G in (None, 1):
        tok = BBPETokenizer(vocab, merges, SP, digit_group=G, pretokenizer="o200k_base")
        assert tok.pretokenizer == "o200k_base" and tok.digit_group == (G or 3)
        for text in TEXTS:
            ids, pieces = _reference_encode(tok, text, G or 3)
            assert tok.encode(text) == ids and tok.decode(ids) == text
            for k, other in enumerate(others):
                differs[k] += tok.encode(text) != other.encode(text)
            got_ids, spans = tok.encode_with_offsets(text, unit="byte")  # the spans tile the text, no token crosses a pre-token cut
            assert got_ids == ids and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))
            cuts, pos = set(), 0
            for p in pieces:
                cuts.add(pos)
                pos += len(p)
            assert all(not any(s < c < e for c in cuts) for s, e in spans)
            assert tok.encode_dropout(text, 0.0, seed=5) == ids
        rows, lengths = tok.encode_batch_padded(TEXTS[:3])
        assert [r[:n] for r, n in zip(rows, lengths)] == [tok.encode(t) for t in TEXTS[:3]]
    assert all(differs)  # (the pattern changes the ids of these texts against both other patterns)
    for bad in ("o200k", "gpt4", 3):
        with pytest.raises(ValueError, match="pretokenizer"):
            BBPETokenizer(vocab, merges, SP, pretokenizer=bad)


def test_save_and_reload(trained, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    for G in (None, 1):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=G, pretokenizer="o200k_base"))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"text_{G}", tmp_path / f"hex_{G}"
        tr.save(a)
        tr.save_lossless(b)
        want = {"pattern": "o200k_base", "digit_group": G or 3}
        assert json.loads((a / "pretokenizer.json").read_text()) == want == json.loads((b / "pretokenizer.json").read_text())
        for tok in (BBPETokenizer.from_file(a), BBPETokenizer.from_file_lossless(b)):
            assert tok.pretokenizer == "o200k_base" and tok.digit_group == (G or 3)
        model = BBPEModel.from_file_lossless(b)
        assert model.pretokenizer == "o200k_base" and model.digit_group == (G or 3) and model.vocab == vocab and model.merges == merges
        tok = BBPETokenizer.from_file_lossless(b)
        for text in TEXTS:
            assert tok.encode(text) == BBPETokenizer(vocab, merges, SP, digit_group=G, pretokenizer="o200k_base").encode(text)
    (tmp_path / "hex_1" / "pretokenizer.json").write_text('{"pattern": "o200k_base"}')  # the pattern alone means three digits
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_1").digit_group == 3
    # saving a GPT-2 model over an o200k_base one leaves no stale file behind
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP))
    tr._vocab, tr._merges = dict(vocab), list(merges)
    tr.save_lossless(tmp_path / "hex_None")
    tok = BBPETokenizer.from_file_lossless(tmp_path / "hex_None")
    assert tok.pretokenizer == "gpt2" and tok.digit_group is None


def test_gpt2_and_cl100k_files_are_written_as_before(trained, tmp_path):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    cases = ((dict(), None), (dict(digit_group=3), b'{"digit_group": 3}'), (dict(pretokenizer="cl100k"), b'{"pattern": "cl100k", "digit_group": 3}'),
             (dict(pretokenizer="cl100k", digit_group=1), b'{"pattern": "cl100k", "digit_group": 1}'))
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


def test_train_from_refuses_another_pattern(trained, tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    f = tmp_path / "more.txt"
    f.write_text("12345 more text 678")
    o2 = BBPETrainerConfig(special_tokens=SP, pretokenizer="o200k_base", vocab_size=2000)
    for other in (BBPEModel(vocab, merges, SP, 3), BBPEModel(vocab, merges, SP, 3, "cl100k")):
        with pytest.raises(ValueError, match="pretokenizer"):
            BBPETrainer(o2).train_from(other, [f])
    for name in ("gpt2", "cl100k"):
        with pytest.raises(ValueError, match="pretokenizer"):
            BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=3, pretokenizer=name, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP, 3, "o200k_base"), [f])
    with pytest.raises(ValueError, match="digit_group"):
        BBPETrainer(o2).train_from(BBPEModel(vocab, merges, SP, 1, "o200k_base"), [f])
    # the same pattern and no budget left: the model comes back unchanged, pattern included (no device call)
    same = BBPETrainer(BBPETrainerConfig(special_tokens=SP, pretokenizer="o200k_base", vocab_size=len(vocab))).train_from(BBPEModel(vocab, merges, SP, None, "o200k_base"), [f])
    assert same.pretokenizer == "o200k_base" and same.digit_group == 3 and same.merges == merges and same.vocab == vocab
