"""Shared by the multi-rank tests of the text options (tests/test_text_sharded_inputs.py on the CPU, tests/test_gpu_text_sharded.py
and tests/text_dist_workers.py on the device): the files the ranks read, the configurations they run, and the reference -- every
chunk through bytes.decode / str.lower / unicodedata of this interpreter, regex's words of the result, the CPU oracle's merges."""
from __future__ import annotations

import random
import unicodedata
from functools import lru_cache

SP = ["<|e|>", "<a>", "[unk]", "[pad]"]   # lower case and NFC: lowercase and the normaliser accept them
CHUNK = 1 << 12                           # chunk_size_bytes of every configuration
DAMAGE_RATE = 500                         # one byte in this many becomes a class byte >= 0x80
LINE = "Call 0123456789 Or 2024-10-20, Room 1234567 <|e|> HTTPServer ÉCOLE İSTANBUL ΟΔΥΣΣΕΥΣ\n"
DEVICE_CHUNK = 4099                       # the device-text scenario: no multiple of 16, so rank 1's share starts at an odd address

BASE = dict(min_frequency=2, special_tokens=SP, chunk_size_bytes=CHUNK)
CONFIGS = {
    "full_o200k": ("damaged", dict(vocab_size=256 + len(SP) + 300, errors="replace", lowercase=True, normalizer="nfc", pretokenizer="o200k_base")),
    "ignore_cl100k_g1": ("damaged", dict(vocab_size=256 + len(SP) + 300, errors="ignore", lowercase=True, pretokenizer="cl100k", digit_group=1)),
    "strict_gpt2_g3_limit": ("clean", dict(vocab_size=256 + len(SP) + 300, lowercase=True, normalizer="nfc", digit_group=3, max_token_length=6)),
    # the vanishing file: rank 1's chunks decode to nothing
    "vanishing": ("vanishing", dict(vocab_size=256 + len(SP) + 100, errors="ignore", lowercase=True, normalizer="nfc")),
    # the first three chunks' worth of the damaged file over four ranks
    "full_o200k_small": ("damaged_head", dict(vocab_size=256 + len(SP) + 60, errors="replace", lowercase=True, normalizer="nfc", pretokenizer="o200k_base")),
}
BIG_CHUNK = 1 << 16                       # the files with a run over the normaliser's cap (32 KiB of marks) need chunks that hold it
ERROR_CONFIGS = {
    "bad_lower": dict(vocab_size=256 + len(SP) + 50, lowercase=True),
    "bad_both": dict(vocab_size=256 + len(SP) + 50, lowercase=True),
    "long_run": dict(vocab_size=256 + len(SP) + 50, errors="replace", normalizer="nfc", chunk_size_bytes=BIG_CHUNK),
    # strict: the run behind a chunk of the same rank that lower-casing made shorter
    "long_run_lowered": dict(vocab_size=256 + len(SP) + 50, lowercase=True, normalizer="nfc", chunk_size_bytes=BIG_CHUNK),
}
ERROR_RANK = {"bad_lower": (1,), "bad_both": (0, 1), "long_run": (1,), "long_run_lowered": (1,)}   # whose share holds what raises


def config(name: str, **over):
    from yet_another_bpe.trainer import BBPETrainerConfig

    kw = CONFIGS[name][1] if name in CONFIGS else ERROR_CONFIGS[name]
    return BBPETrainerConfig(**{**BASE, **kw, **over})


# ---------------------------------------------------------------- the files
@lru_cache(maxsize=None)
def corpus(golden_dir) -> tuple[bytes, bytes]:
    """-> (damaged, clean): the lower-casing tests' training text (cased, multilingual, decomposed marks, Greek capitals with
    final sigmas, a dotted I and a Kelvin sign), 60 lines of digits, case changes and a special, and the head of the text
    again; `damaged` has a seeded 1 byte in DAMAGE_RATE replaced by a class byte >= 0x80."""
    from tests import case_helpers, utf8_helpers

    text = case_helpers.training_text(golden_dir, 40_000)
    clean = text + (LINE * 60).encode("utf-8") + text[:15_000]
    clean.decode("utf-8")  # (the head is cut at a character boundary, or this raises)
    data = bytearray(clean)
    rng = random.Random(29)
    for _ in range(len(data) // DAMAGE_RATE):
        data[rng.randrange(len(data))] = rng.choice(utf8_helpers.HIGH)
    return bytes(data), clean


def vanishing(golden_dir) -> bytes:
    return corpus(golden_dir)[1][:30_000] + b"\x80" * 30_000


def file_bytes(kind: str, golden_dir) -> bytes:
    """The bytes of CONFIGS[name][0]."""
    damaged, clean = corpus(golden_dir)
    if kind == "vanishing":
        return vanishing(golden_dir)
    return {"damaged": damaged, "clean": clean, "damaged_head": damaged[:3 * CHUNK - 100]}[kind]


def ranges_of(data: bytes, step: int = CHUNK) -> list[tuple[int, int]]:
    """The chunk cuts BBPETrainer._chunk_ranges makes in a file of these bytes (the tests check that against a file)."""
    from yet_another_bpe.trainer import chunk_ranges

    return chunk_ranges(len(data), step, lambda off, n: data[off:off + n])


def shares(ranges, world: int) -> list[tuple[int, int]]:
    """[c0, c1) chunk indices per rank, as the drivers plan them."""
    from yet_another_bpe.distributed import plan_chunk_shards

    return plan_chunk_shards([b - a for a, b in ranges], world)


def byte_share(ranges, world: int, rank: int) -> tuple[int, int]:
    """The file positions [a, b) of the rank's chunks."""
    c0, c1 = shares(ranges, world)[rank]
    assert c1 > c0
    return ranges[c0][0], ranges[c1 - 1][1]


def error_file(name: str, golden_dir) -> tuple[bytes, list[int]]:
    """Files that make the drivers raise -> (bytes, the file positions of the bad bytes or of the run's base letter, in
    order): each lies in the share of the rank ERROR_RANK names, of two (the CPU test checks it)."""
    from tests import nfc_helpers

    run = b"a" + "\u0301".encode("utf-8") * (nfc_helpers.CAP + 5)
    if name in ("bad_lower", "bad_both"):
        data = bytearray(corpus(golden_dir)[1][:40_000].decode("utf-8", "ignore").encode("utf-8"))
        spots = []
        for pos in ((5_003, 30_001) if name == "bad_both" else (30_001,)):
            while data[pos] >= 0x80:  # an ASCII byte: one ill-formed byte in its place, whatever the cuts
                pos += 1
            data[pos] = 0xFF
            spots.append(pos)
        return bytes(data), spots
    if name == "long_run":  # rank 0: a chunk of repairs; rank 1: more repairs (the positions behind them move), then the run
        head = b"fine \xff" * 1000
        front = b"some \xff\xff words \xff" * 20
        data = head + b" " * (BIG_CHUNK - len(head)) + front + run + b" tail " + b"and more text " * 300
        return data, [BIG_CHUNK + len(front)]
    if name == "long_run_lowered":  # rank 0: three chunks; rank 1: a chunk that loses 2 bytes per Kelvin sign, then one with the run
        kelvin = "\u212a".encode("utf-8") * 1000
        data = b"plain text " * (3 * BIG_CHUNK // 11) + b" " * (3 * BIG_CHUNK % 11) + kelvin + b" " * (BIG_CHUNK - len(kelvin)) + run + b" tail"
        return data, [4 * BIG_CHUNK]
    raise ValueError(name)


# ---------------------------------------------------------------- the reference
def splitter(cfg):
    """The regex splitter of cfg's pattern and digit group: (bytes, chunk starts) -> words"""
    from tests import group_helpers, split4_helpers, split5_helpers

    if cfg.pretokenizer == "o200k_base":
        return lambda b, st: split5_helpers.regex_split(b, cfg.digit_group or 3, list(cfg.special_tokens), st)
    if cfg.pretokenizer == "cl100k":
        return lambda b, st: split4_helpers.regex_split(b, cfg.digit_group or 3, list(cfg.special_tokens), st)
    return lambda b, st: group_helpers.regex_split(b, cfg.digit_group or 0, list(cfg.special_tokens), st)


def transformed(chunk: bytes, cfg, drop=None) -> bytes:
    """One chunk as the trainer must read it; drop in {"errors", "lower", "nfc"}: that one step done wrongly."""
    errors = cfg.errors
    if drop == "errors":
        errors = {"replace": "ignore", "ignore": "replace"}[errors]
    s = chunk.decode("utf-8", errors)
    if cfg.lowercase and drop != "lower":
        s = s.lower()
    if cfg.normalizer and drop != "nfc":
        s = unicodedata.normalize("NFC", s)
    return s.encode("utf-8")


def reference_words(data: bytes, ranges, cfg, split, drop=None, world: int = 2) -> list[bytes]:
    """Every chunk transformed on its own, then split(the concatenation, the chunk starts in it).  `drop` applies one step
    wrongly to the chunks of rank 1 of `world`: what a driver would compute that forgot the option there."""
    c0, c1 = shares(ranges, world)[1] if drop else (0, 0)
    parts = [transformed(data[a:b], cfg, drop if c0 <= k < c1 else None) for k, (a, b) in enumerate(ranges)]
    starts = [0]
    for p in parts:
        starts.append(starts[-1] + len(p))
    return split(b"".join(parts), starts[:-1])


def expected_model(words, cfg):
    """-> (vocab, merges): the CPU oracle; under a limit the plain-Python trainer of tests/limit_helpers.py, as tests/test_gpu_limit.py"""
    from oracle import oracle
    from tests import helpers, limit_helpers

    if cfg.max_token_length is None:
        return oracle.merge_loop(words, cfg.vocab_size, cfg.min_frequency, list(cfg.special_tokens))
    uw, fq = helpers.pooled(words)
    return limit_helpers.train(uw, fq, cfg.vocab_size - 256 - len(cfg.special_tokens), cfg.min_frequency, list(cfg.special_tokens), limit=cfg.max_token_length)


_MODELS: dict = {}


def expected(name: str, golden_dir, step: int = CHUNK):
    """(vocab, merges) of CONFIGS[name] on its file, chunked every `step` bytes; computed once per process and shared."""
    if (name, step) not in _MODELS:
        cfg = config(name, chunk_size_bytes=step)
        data = file_bytes(CONFIGS[name][0], golden_dir)
        _MODELS[name, step] = expected_model(reference_words(data, ranges_of(data, step), cfg, splitter(cfg)), cfg)
    return _MODELS[name, step]
