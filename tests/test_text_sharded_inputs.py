"""CPU: the inputs of tests/test_gpu_text_sharded.py tell a right driver from a wrong one -- the oracle's model changes when one
option is applied wrongly to rank 1's chunks only, or when the file is read as one text; the vanishing file really empties
rank 1; the device-text share really starts at an odd address; the error files hold what raises in the share of the rank named."""
from __future__ import annotations

import unicodedata

import pytest

from tests import limit_helpers, text_dist_helpers as th

NAMES = ["full_o200k", "ignore_cl100k_g1", "strict_gpt2_g3_limit"]


@pytest.fixture(scope="module")
def files(golden_dir):
    return {kind: th.file_bytes(kind, golden_dir) for kind in ("damaged", "clean", "vanishing", "damaged_head")}


def test_corpus(files, golden_dir, tmp_path):
    from tests import utf8_helpers
    from yet_another_bpe.trainer import BBPETrainer

    damaged, clean = files["damaged"], files["clean"]
    assert 100_000 <= len(clean) <= 125_000 and len(damaged) == len(clean)
    text = clean.decode("utf-8")
    assert text.lower() != text and unicodedata.normalize("NFC", text) != text
    for piece in ("Σ ", "İstanbul", "Kelvin", "<|e|>", "HTTPServer", "0123456789", "é"):
        assert piece in text, piece
    differing = [i for i, (a, b) in enumerate(zip(damaged, clean)) if a != b]
    assert len(clean) // th.DAMAGE_RATE * 0.9 <= len(differing) <= len(clean) // th.DAMAGE_RATE
    assert all(damaged[i] in utf8_helpers.HIGH for i in differing)
    for s in th.SP:
        assert s == s.lower() and s == unicodedata.normalize("NFC", s)
    # the helper's cuts are the product's cuts in a file of these bytes
    for kind, step in (("damaged", th.CHUNK), ("clean", th.CHUNK), ("damaged", th.DEVICE_CHUNK), ("vanishing", th.CHUNK)):
        f = tmp_path / "f.txt"
        f.write_bytes(files[kind])
        assert BBPETrainer(th.config("full_o200k", chunk_size_bytes=step))._chunk_ranges(f) == th.ranges_of(files[kind], step)


@pytest.mark.parametrize("name", NAMES)
def test_every_configuration_has_300_merges_and_two_busy_ranks(name, files, golden_dir):
    data = files[th.CONFIGS[name][0]]
    ranges = th.ranges_of(data)
    assert 26 <= len(ranges) <= 30
    assert all(c1 - c0 >= 10 for c0, c1 in th.shares(ranges, 2))
    vocab, merges = th.expected(name, golden_dir)
    assert len(merges) == 300 and len(vocab) == 256 + len(th.SP) + 300
    if name == "strict_gpt2_g3_limit":
        assert all(len(l) + len(r) <= 6 for l, r in merges)
        free = th.expected_model(th.reference_words(data, ranges, th.config(name), th.splitter(th.config(name))), th.config(name, max_token_length=None))[1]
        assert free != merges  # the limit binds within the 300


def test_an_option_dropped_on_rank_1_changes_the_model(files, golden_dir):
    cfg = th.config("full_o200k")
    data = files["damaged"]
    ranges = th.ranges_of(data)
    merges = th.expected("full_o200k", golden_dir)[1]
    for drop in ("errors", "lower", "nfc"):
        wrong = th.expected_model(th.reference_words(data, ranges, cfg, th.splitter(cfg), drop=drop), cfg)[1]
        at = limit_helpers.first_difference(merges, wrong)
        print(f"drop={drop}: first difference at merge {at}")
        assert at < 300, drop
    # ... and so do the chunk-local rules: the file read as one text (a final sigma, a mark or a truncated sequence at a cut)
    whole = th.expected_model(th.reference_words(data, [(0, len(data))], cfg, th.splitter(cfg)), cfg)[1]
    at = limit_helpers.first_difference(merges, whole)
    print(f"one text: first difference at merge {at}")
    assert at < 300
    # the second configuration tells its options too
    cfg = th.config("ignore_cl100k_g1")
    merges = th.expected("ignore_cl100k_g1", golden_dir)[1]
    for drop in ("errors", "lower"):
        wrong = th.expected_model(th.reference_words(data, ranges, cfg, th.splitter(cfg), drop=drop), cfg)[1]
        assert limit_helpers.first_difference(merges, wrong) < 300, drop


def test_vanishing_share(files, golden_dir):
    data = files["vanishing"]
    cfg = th.config("vanishing")
    ranges = th.ranges_of(data)
    (a0, a1), (b0, b1) = th.shares(ranges, 2)
    assert a1 == b0 and b1 == len(ranges) and b1 > b0
    for a, b in ranges[b0:b1]:
        assert len(data[a:b].decode("utf-8", "ignore")) == 0
    assert len(th.reference_words(data, ranges[a0:a1], cfg, th.splitter(cfg))) > 1000
    vocab, merges = th.expected("vanishing", golden_dir)
    assert len(merges) == 100


def test_four_ranks_share_three_chunks(files, golden_dir):
    data = files["damaged_head"]
    ranges = th.ranges_of(data)
    assert len(ranges) == 3
    shares = th.shares(ranges, 4)
    assert any(c0 == c1 for c0, c1 in shares) and sum(c1 - c0 for c0, c1 in shares) == 3
    assert len(th.expected("full_o200k_small", golden_dir)[1]) == 60


def test_device_text_share_is_unaligned(files, golden_dir):
    assert th.DEVICE_CHUNK % 16
    ranges = th.ranges_of(files["damaged"], th.DEVICE_CHUNK)
    assert all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))
    a0 = th.byte_share(ranges, 2, 1)[0]
    assert a0 % 16 != 0
    assert all(c1 - c0 >= 10 for c0, c1 in th.shares(ranges, 2))
    assert len(th.expected("full_o200k", golden_dir, th.DEVICE_CHUNK)[1]) == 300


def test_a_run_is_reported_alike_from_any_buffer():
    """The normaliser's error names a byte of the buffer it read -- the whole corpus, or one rank's chunks: the trainer's message
    names the file position (or the chunk and the position in it) and must not repeat the buffer's."""
    from pathlib import Path

    from yet_another_bpe import _native
    from yet_another_bpe.trainer import repaired_segment_error, segment_error

    chunks = [(Path("f.txt"), 100, 200), (Path("f.txt"), 200, 300)]
    words = "the segment that starts at byte {} holds more than 16384 code points to normalise together (a base and its combining marks): over the cap of 16384"
    for make in (segment_error, repaired_segment_error):
        whole = str(make(chunks, [0, 90], _native.SegmentTooLong(95, words.format(95))))      # (the first chunk lost 10 bytes on the way)
        share = str(make(chunks[1:], [0], _native.SegmentTooLong(5, words.format(5))))
        assert whole == share and "16384" in whole and "at byte" not in whole
    assert "at position 205: it holds more than" in str(segment_error(chunks, [0, 90], _native.SegmentTooLong(95, words.format(95))))


@pytest.mark.parametrize("name", list(th.ERROR_CONFIGS))
def test_error_files(name, golden_dir):
    from tests import nfc_helpers

    data, spots = th.error_file(name, golden_dir)
    cfg = th.config(name)
    ranges = th.ranges_of(data, cfg.chunk_size_bytes)
    assert len(spots) == len(th.ERROR_RANK[name])
    for pos, rank in zip(spots, th.ERROR_RANK[name]):
        a, b = th.byte_share(ranges, 2, rank)
        assert a <= pos < b, (pos, rank, a, b)
    if name.startswith("bad"):
        assert [i for i, x in enumerate(data) if x == 0xFF] == spots and spots == sorted(spots)
        with pytest.raises(UnicodeDecodeError) as e:
            data.decode("utf-8")
        assert e.value.start == spots[0]
        data.replace(b"\xff", b"x").decode("utf-8")  # nothing else is wrong with it
    else:
        # the whole run lies in one chunk, behind bytes of the same rank's share that change length on the way to the normaliser
        k = max(i for i, (a, _b) in enumerate(ranges) if a <= spots[0])
        assert spots[0] + 1 + 2 * (nfc_helpers.CAP + 5) <= ranges[k][1]
        a, _b = th.byte_share(ranges, 2, 1)
        front = data[a:spots[0]]
        moved = front.decode("utf-8", cfg.errors if cfg.errors != "strict" else "strict")
        moved = moved.lower() if cfg.lowercase else moved
        assert len(moved.encode("utf-8")) != len(front)
        if name == "long_run":
            assert b"\xff" in data[slice(*th.byte_share(ranges, 2, 0))]
        else:
            assert ranges[k][0] > a  # an earlier chunk of rank 1 shrank: the run's chunk no longer starts where it did
            data.decode("utf-8")
