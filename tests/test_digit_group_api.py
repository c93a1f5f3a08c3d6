"""CPU: digit_group through the Python interface -- BBPETrainerConfig validation, the rejection of a special token that
begins with a digit, the host pre-tokeniser and the plain-Python tokenizer against regex.findall with the grouped pattern,
pretokenizer.json through save / from_file / from_file_lossless, and train_from's mismatch error.  No GPU: the model the
tokenizer tests use comes from the CPU oracle."""
from __future__ import annotations

import json

import pytest
import regex

from tests import group_helpers as gh

SP = ["<|e|>", "<x1", "[UNK]"]
TEXTS = ["In 2024 the total was 1,234,567.8901 units", "call 0049301234567 now<|e|>12345<x1234 ١٢٣٤٥٦", " 1234567 and 12's 1234's", "²³½Ⅷ12 12\n345",
         "a1234b<|e|><|e|> 123", "no digits here", "7", ""]


@pytest.fixture(scope="module")
def trained(golden_dir):
    """(vocab, merges) of the CPU oracle on the number corpus, pre-tokenised by regex with \\p{N}{1,3}."""
    from oracle import oracle

    words = gh.regex_split(gh.number_corpus(golden_dir), 3, SP)
    return oracle.merge_loop(words, 256 + len(SP) + 300, 2, SP)


def test_config_validation(tmp_path):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig, digit_group

    assert BBPETrainerConfig().digit_group is None and digit_group(BBPETrainerConfig()) == 0
    for ok in (1, 3, 255):
        assert digit_group(BBPETrainerConfig(digit_group=ok)) == ok
    f = tmp_path / "never_read.txt"  # (does not exist: the value is rejected before any file is looked at)
    for bad in (0, -1, 256, 3.0, "3", True, False):
        with pytest.raises(ValueError, match="digit_group"):
            BBPETrainer(BBPETrainerConfig(digit_group=bad)).train([f])
        with pytest.raises(ValueError, match="digit_group"):
            BBPETrainer(BBPETrainerConfig(digit_group=bad))._split_pattern()


def test_digit_leading_special_is_rejected(tmp_path):
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    f = tmp_path / "never_read.txt"
    for tok in ("77", "1st", "٣x", "½"):
        cfg = BBPETrainerConfig(digit_group=3, special_tokens=["<|e|>", tok])
        with pytest.raises(ValueError, match="begins with a digit"):
            BBPETrainer(cfg).train([f])
        with pytest.raises(ValueError, match="begins with a digit"):
            BBPETrainer(cfg).train_from(BBPEModel({}, [], cfg.special_tokens, 3), [f])
        with pytest.raises(ValueError, match="begins with a digit"):
            train_text_sharded(None, [f], cfg, 0, 1)
        assert BBPETrainer(BBPETrainerConfig(special_tokens=["<|e|>", tok]))._split_pattern()  # without a group: as before
    for tok in ("<7", " 7", "s1", "x12"):
        assert BBPETrainer(BBPETrainerConfig(digit_group=3, special_tokens=[tok]))._split_pattern()


def test_host_pretokenize_against_regex(tmp_path, golden_dir):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    data = gh.number_corpus(golden_dir) + "\n".join(gh.DIGITS + gh.SPECIAL_TEXTS).encode("utf-8")
    f = tmp_path / "corpus.txt"
    f.write_bytes(data)
    for G in (None, 1, 2, 3, 4):
        for sp in ([], ["<x1", "<|7|>", "s1"]):
            tr = BBPETrainer(BBPETrainerConfig(digit_group=G, special_tokens=sp))
            got = tr._pretokenize([f])
            assert [t.encode("utf-8") for t in got] == gh.regex_split(data, G or 0, sp)
            assert tr._preprocess_corpus([f]) == [list(t.encode("utf-8")) for t in got]
            if G:
                assert max(gh.digits_in(t.encode("utf-8")) for t in got if t not in sp) <= G
    # chunks are texts of their own: a cut inside a digit run restarts the count
    f.write_bytes(b"1234567890" * 20)
    tr = BBPETrainer(BBPETrainerConfig(digit_group=3, special_tokens=[], chunk_size_bytes=64))
    starts = [a for a, _ in tr._chunk_ranges(f)]
    assert len(starts) == 4 and [t.encode() for t in tr._pretokenize([f])] == gh.regex_split(b"1234567890" * 20, 3, (), starts)


def _reference_encode(tok, text: str, G: int | None):
    """encode restated: the special split, regex.findall with the grouped pattern, the tokenizer's own word merge"""
    pat = regex.compile(gh.grouped_pattern(G or 0))
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
    assert max(gh.digits_in(t) for t in vocab if t.decode("utf-8", "ignore") not in SP) <= 3  # what the grouping is for
    plain = BBPETokenizer(vocab, merges, SP)
    assert plain.digit_group is None
    differs = 0
    for G in (1, 3):
        tok = BBPETokenizer(vocab, merges, SP, digit_group=G)
        assert tok.digit_group == G
        for text in TEXTS:
            ids, pieces = _reference_encode(tok, text, G)
            assert tok.encode(text) == ids and tok.decode(ids) == text
            differs += tok.encode(text) != plain.encode(text)
            # the spans tile the text, and no token crosses a pre-token cut
            data = text.encode("utf-8")
            got_ids, spans = tok.encode_with_offsets(text, unit="byte")
            assert got_ids == ids and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))
            assert not data or (spans[0][0] == 0 and spans[-1][1] == len(data))
            cuts, pos = set(), 0
            for p in pieces:
                cuts.add(pos)
                pos += len(p)
            assert all(not any(s < c < e for c in cuts) for s, e in spans)
            char_ids, char_spans = tok.encode_with_offsets(text, unit="char")
            assert char_ids == ids and (not text or (char_spans[0][0] == 0 and char_spans[-1][1] == len(text)))
            # dropout: p = 0 is encode, p = 1 one id per byte of every pre-token (a special stays one id)
            assert tok.encode_dropout(text, 0.0, seed=5) == ids
            every_byte = [i for p in pieces for i in ([vocab[p]] if p.decode() in SP else [vocab[bytes([b])] for b in p])]
            assert tok.encode_dropout(text, 1.0, seed=5) == every_byte
        rows, lengths = tok.encode_batch_padded(TEXTS[:3])
        assert [r[:n] for r, n in zip(rows, lengths)] == [tok.encode(t) for t in TEXTS[:3]]
    assert differs  # (the grouping changes the ids of these texts: the tests above are not vacuous)
    for bad in (0, 256, True, "3"):
        with pytest.raises(ValueError, match="digit_group"):
            BBPETokenizer(vocab, merges, SP, digit_group=bad)


def test_save_and_reload(trained, tmp_path):
    from yet_another_bpe.tokenizer import BBPETokenizer
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    for G in (None, 3):
        tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=G))
        tr._vocab, tr._merges = dict(vocab), list(merges)
        a, b = tmp_path / f"text_{G}", tmp_path / f"hex_{G}"
        tr.save(a)
        tr.save_lossless(b)
        if G is None:  # exactly the files a model always had
            assert sorted(p.name for p in a.iterdir()) == ["merges.txt", "special_tokens.json", "vocab.json"]
            assert sorted(p.name for p in b.iterdir()) == ["merges.hex", "special_tokens.json", "vocab.hex.json"]
        else:
            assert json.loads((a / "pretokenizer.json").read_text()) == {"digit_group": 3} == json.loads((b / "pretokenizer.json").read_text())
        assert BBPETokenizer.from_file(a).digit_group == G and BBPETokenizer.from_file_lossless(b).digit_group == G
        model = BBPEModel.from_file_lossless(b)
        assert model.digit_group == G and model.vocab == vocab and model.merges == merges
        tok = BBPETokenizer.from_file_lossless(b)
        assert tok.encode(TEXTS[0]) == BBPETokenizer(vocab, merges, SP, digit_group=G).encode(TEXTS[0])
    long_run = "x" + "0123456789" * 3
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_3").encode(long_run) != BBPETokenizer.from_file_lossless(tmp_path / "hex_None").encode(long_run)
    # saving a model without a group over one with a group leaves no stale file behind
    tr = BBPETrainer(BBPETrainerConfig(special_tokens=SP))
    tr._vocab, tr._merges = dict(vocab), list(merges)
    tr.save_lossless(tmp_path / "hex_3")
    assert BBPETokenizer.from_file_lossless(tmp_path / "hex_3").digit_group is None


def test_train_from_refuses_another_grouping(trained, tmp_path):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    vocab, merges = trained
    f = tmp_path / "more.txt"
    f.write_text("12345 more text 678")

    class Bare:  # anything with .vocab, .merges, .special_tokens: no digit_group means None
        def __init__(self):
            self.vocab, self.merges, self.special_tokens = vocab, merges, SP

    for model_g, cfg_g in [(3, None), (None, 3), (3, 1)]:
        with pytest.raises(ValueError, match="digit_group"):
            BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=cfg_g, vocab_size=2000)).train_from(BBPEModel(vocab, merges, SP, model_g), [f])
    with pytest.raises(ValueError, match="digit_group"):
        BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=3, vocab_size=2000)).train_from(Bare(), [f])
    # the same grouping and no budget left: the model comes back unchanged, grouping included (no device call)
    same = BBPETrainer(BBPETrainerConfig(special_tokens=SP, digit_group=3, vocab_size=len(vocab))).train_from(BBPEModel(vocab, merges, SP, 3), [f])
    assert same.digit_group == 3 and same.merges == merges and same.vocab == vocab
