"""Word-length cases for the loader tests (tests/test_load_model.py on the CPU, tests/test_gpu_load_form.py on the GPU):
name -> (lengths of the words, offset of the first word in its byte buffer).  SPAN = 961 packed positions per tile, words of
64 bytes and more are long."""
from __future__ import annotations

import random

import numpy as np

CAP, LMAX = 1024, 64
SPAN = CAP - LMAX + 1


def _random_short(n: int, seed: int) -> list[int]:
    rng = random.Random(seed)
    return [rng.choice([0, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9, 11, 14, 20, 33]) for _ in range(n)]


def cases() -> dict[str, tuple[list[int], int]]:
    many = _random_short(40_000, 3)  # ~300 tiles: more than one workgroup of 64 tiles
    return {
        "ends_on_last_span_slot": ([SPAN - 6, 4, 3, 9], 0),          # 956 slots, then 4 bytes: the SEP lies on slot SPAN-1
        "starts_on_slot_span_minus_1": ([62, SPAN - 65, 63, 2], 0),  # the 63-byte word runs through the whole LMAX tail
        "lengths_0_1_2_63_64": ([0, 1, 2, 63, 64, 2, 0, 1, 64, 63, 2], 0),
        "longer_than_a_span": ([3, 2 * SPAN + 100, 4, 5], 0),        # tile 1 has no word start
        "off_base": (_random_short(700, 5) + [70, 2], 37),
        "zero_words": ([], 0),
        "one_word": ([5], 0),
        "partly_filled_last_tile": (_random_short(300, 7), 0),
        "random_300_tiles": (many, 0),
        "random_300_tiles_off_base_long": (many[:20_000] + [64, 200, 3 * SPAN] + many[20_000:], 1001),
        "only_empty_words": ([0] * 3000, 0),
    }


def build(lens: list[int], off_base: int) -> tuple[np.ndarray, np.ndarray]:
    """-> (bytes u8 with off_base bytes in front that belong to no word, offsets u64 starting at off_base)"""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[0] = off_base
    if lens:
        off[1:] = off_base + np.cumsum(np.asarray(lens, dtype=np.uint64))
    n = int(off[-1])
    flat = ((np.arange(n, dtype=np.uint64) * 131 + 7) % 26 + 97).astype(np.uint8)  # letters: every byte is a base token
    return flat, off
