"""GPU (-m gpu): the sharded text drivers (distributed.train_text_sharded / train_device_text_sharded) with the text options on --
errors="replace" / "ignore", lowercase, normalizer="nfc", the cl100k and o200k_base patterns, digit groups, a maximum token
length -- over two and four ranks that share one GPU (custom transport, gloo underneath).  Every rank repairs, lowers,
normalises and pre-tokenises ITS chunks; the merges must be the CPU oracle's on regex's words of the chunks as this interpreter
transforms them (tests/text_dist_helpers.py; tests/test_text_sharded_inputs.py shows that an option applied on one rank only
would give another model).  Also: a rank whose text vanishes, ranks without a chunk, errors that every rank must learn of, and
a share that starts at an unaligned device address."""
from __future__ import annotations

import pytest

from tests import dist_workers, text_dist_helpers as th, text_dist_workers as tw

pytestmark = pytest.mark.gpu


def _pairs(merges):
    return [(bytes.fromhex(a), bytes.fromhex(b)) for a, b in merges]


def _file(tmp_path, data: bytes, name: str = "text.txt"):
    f = tmp_path / name
    f.write_bytes(data)
    return f


def _check_ranks(outs, names, golden_dir):
    for rank, out in enumerate(outs):
        assert list(out) == list(names)
        for name in names:
            exp_vocab, exp_merges = th.expected(name, golden_dir)
            merges, n_vocab = out[name]
            assert _pairs(merges) == exp_merges, (name, rank)
            assert n_vocab == len(exp_vocab), (name, rank)


def test_two_ranks_every_option(golden_dir, tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer

    names = ["full_o200k", "ignore_cl100k_g1"]
    f = _file(tmp_path, th.file_bytes("damaged", golden_dir))
    outs = dist_workers.spawn(tw.gpu_text_options, 2, str(f), names, timeout=300)
    assert len(outs) == 2
    _check_ranks(outs, names, golden_dir)
    # the single-device control: the same file and configuration through BBPETrainer's device route
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    monkeypatch.setenv("YABPE_OPT_verify", "1")
    for name in names:
        exp_vocab, exp_merges = th.expected(name, golden_dir)
        model = BBPETrainer(th.config(name)).train([f])
        assert model.merges == exp_merges and model.vocab == exp_vocab, name


def test_two_ranks_strict_with_limit(golden_dir, tmp_path):
    names = ["strict_gpt2_g3_limit"]
    f = _file(tmp_path, th.file_bytes("clean", golden_dir))
    outs = dist_workers.spawn(tw.gpu_text_options, 2, str(f), names, timeout=300)
    assert len(outs) == 2
    _check_ranks(outs, names, golden_dir)
    for out in outs:
        assert len(out[names[0]][0]) == 300 and all(len(l) + len(r) <= 6 for l, r in _pairs(out[names[0]][0]))


def test_rank_whose_text_vanishes(golden_dir, tmp_path):
    """errors="ignore" drops every byte of rank 1's chunks: it loads nothing in the pooled layout and still joins every
    collective (the spawn's timeout is the guard against a rank that waits for it)."""
    names = ["vanishing"]
    f = _file(tmp_path, th.file_bytes("vanishing", golden_dir))
    outs = dist_workers.spawn(tw.gpu_text_options, 2, str(f), names, timeout=300)
    assert len(outs) == 2
    _check_ranks(outs, names, golden_dir)
    assert all(len(out["vanishing"][0]) == 100 for out in outs)


def test_four_ranks_fewer_chunks_than_ranks(golden_dir, tmp_path):
    names = ["full_o200k_small"]
    data = th.file_bytes("damaged_head", golden_dir)
    assert any(c0 == c1 for c0, c1 in th.shares(th.ranges_of(data), 4))  # a rank without a chunk
    f = _file(tmp_path, data)
    outs = dist_workers.spawn(tw.gpu_text_options, 4, str(f), names, timeout=300)
    assert len(outs) == 4
    _check_ranks(outs, names, golden_dir)
    assert all(len(out[names[0]][0]) == 60 for out in outs)


@pytest.mark.parametrize("name", list(th.ERROR_CONFIGS))
def test_errors_reach_every_rank(name, golden_dir, tmp_path, monkeypatch):
    """What one rank finds in its share, every rank raises -- in the words of the single-device trainer for that file: the file
    position of the first ill-formed byte anywhere (bad_both: rank 0's), the chunk and the position inside it of a run over the
    normaliser's cap behind a repair (long_run) or behind a chunk of the same rank that lower-casing shortened (long_run_lowered)."""
    from yet_another_bpe.trainer import BBPETrainer

    data, spots = th.error_file(name, golden_dir)
    cfg = th.config(name)
    f = _file(tmp_path, data, name + ".txt")
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    with pytest.raises(ValueError) as single:
        BBPETrainer(cfg).train([f])
    message = str(single.value)
    # what the message must say, worked out from the file
    ranges = th.ranges_of(data, cfg.chunk_size_bytes)
    if name.startswith("bad"):
        assert message == f"File {f} contains invalid UTF-8 at position {spots[0]}."
    else:
        a, b = next((a, b) for a, b in ranges if a <= spots[0] < b)
        inside = len(th.transformed(data[a:spots[0]], th.config(name, normalizer=None)))
        if name == "long_run":
            assert f"in the chunk of bytes {a} to {b}, at position {inside} of that chunk after" in message and str(f) in message
        else:
            assert f"File {f} holds a run" in message and f"cap at position {a + inside}:" in message
    kwargs = {k: getattr(cfg, k) for k in ("vocab_size", "min_frequency", "special_tokens", "chunk_size_bytes", "errors", "lowercase", "normalizer")}
    outs = dist_workers.spawn(tw.gpu_text_error, 2, str(f), kwargs, timeout=300)
    assert outs == [message, message]


def test_device_text_unaligned_share(golden_dir, tmp_path):
    """train_device_text_sharded hands rank 1 the text's address plus its share's start, which is no multiple of 16: the four
    passes must read it piece by piece the slow way and still give the oracle's words."""
    data = th.file_bytes("damaged", golden_dir)
    assert th.byte_share(th.ranges_of(data, th.DEVICE_CHUNK), 2, 1)[0] % 16 != 0
    exp_merges = th.expected("full_o200k", golden_dir, th.DEVICE_CHUNK)[1]
    f = _file(tmp_path, data)
    outs = dist_workers.spawn(tw.gpu_device_text_options, 2, str(f), "full_o200k", th.DEVICE_CHUNK, timeout=300)
    assert len(outs) == 2
    for merges, n_words in outs:
        assert _pairs(merges) == exp_merges
        assert n_words > 0  # both ranks held words
