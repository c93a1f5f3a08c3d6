"""CPU: the contract of BBPETokenizer.decode_rows / decode_rows_with_offsets on hand-written rows, and the character-start rule
of csrc/decode_logic.h (what lets a kernel compute the offsets locally) against bytes.decode on every short byte string."""
from __future__ import annotations

import ctypes
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import decode_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"
EOS, PAD, SEP = 256, 257, 258  # specials of the byte-level tokenizer below; 300 is an id it does not name
E9, ZH = list("é".encode()), list("中".encode())


@pytest.fixture(scope="module")
def tok():
    vocab = {bytes([b]): b for b in range(256)}
    vocab.update({b"<eos>": EOS, b"<pad>": PAD, b"<sep>": SEP})
    return BBPETokenizer(vocab=vocab, merges=[], special_tokens=["<eos>", "<pad>", "<sep>"])


# (row, keyword arguments) -> (text, offsets, n_kept)
CASES = {
    "stop_at_lo": (([65, EOS, 66, 67], dict(starts=[1], stop_ids=[EOS])), ("", [(0, 0)] * 4, 0)),
    "stop_at_last_column": (([65, 66, EOS], dict(stop_ids=[EOS])), ("AB", [(0, 1), (1, 2), (2, 2)], 2)),
    "no_stop": (([65, 66, 67], dict(stop_ids=[EOS])), ("ABC", [(0, 1), (1, 2), (2, 3)], 3)),
    "include_stop_kept": (([65, EOS, 66], dict(stop_ids=[EOS], include_stop=True, skip_special_tokens=False)),
                          ("A<eos>", [(0, 1), (1, 6), (6, 6)], 2)),
    "include_stop_still_a_special": (([65, EOS, 66], dict(stop_ids=[EOS], include_stop=True)), ("A", [(0, 1), (1, 1), (1, 1)], 1)),
    "special_inside_a_character": (([E9[0], SEP, E9[1], 65], {}), ("éA", [(0, 1), (1, 1), (1, 1), (1, 2)], 3)),
    "cut_inside_a_character": (([65, ZH[0], ZH[1], EOS, ZH[2]], dict(stop_ids=[EOS])), ("A�", [(0, 1), (1, 2), (2, 2), (2, 2), (2, 2)], 3)),
    "all_pad": (([PAD] * 3, dict(pad_id=PAD, skip_special_tokens=False)), ("", [(0, 0)] * 3, 0)),
    "right_padding": (([65, 66, 0, 0], dict(ends=[2])), ("AB", [(0, 1), (1, 2), (2, 2), (2, 2)], 2)),
    "left_padding": (([0, 0, 65, 66], dict(starts=[2])), ("AB", [(0, 0), (0, 0), (0, 1), (1, 2)], 2)),
    "unknown_ids": (([65, 300, -5, 1 << 40, 66], {}), ("AB", [(0, 1), (1, 1), (1, 1), (1, 1), (1, 2)], 5)),
    "skip_ids": (([65, 66, 67], dict(skip_ids=[66])), ("AC", [(0, 1), (1, 1), (1, 2)], 2)),
}


@pytest.mark.parametrize("name", CASES)
def test_contract(tok, name):
    (row, kw), (text, offsets, kept) = CASES[name]
    assert tok.decode_rows_with_offsets([row], **kw) == ([text], [offsets], [kept])
    assert tok.decode_rows(np.asarray([row]) if max(row) < 1 << 32 else [row], **kw) == [text]


def test_empty_shapes_and_bad_windows(tok):
    assert tok.decode_rows_with_offsets([]) == ([], [], [])
    assert tok.decode_rows_with_offsets([[], []]) == (["", ""], [[], []], [0, 0])
    assert tok.decode_rows_with_offsets(np.zeros((0, 5), np.uint32)) == ([], [], [])
    for kw in (dict(starts=[3], ends=[2]), dict(ends=[5]), dict(starts=[-1]), dict(starts=[0, 0])):
        with pytest.raises(ValueError):
            tok.decode_rows([[65, 66, 67, 68]], **kw)
    with pytest.raises(ValueError):
        tok.decode_rows([[65, 66], [65]])


def test_nchars_is_the_count_of_character_starts():
    """nchars(b) = len(data[:b].decode("utf-8", "replace")) = the bytes in [0, b) that dec_char_start marks in all of data."""
    so, src = HM / "libdecrows_model.so", HM / "decrows_model.cpp"
    deps = [src, HM.parent.parent / "yet-another-bpe_amd/csrc/decode_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    for n in range(1, 5):
        docs = list(itertools.product(decode_helpers.CLASS_BYTES, repeat=n))
        data = np.asarray(docs, dtype=np.uint8)
        out = np.zeros_like(data)
        lib.char_starts(ctypes.c_void_p(data.ctypes.data), ctypes.c_uint64(len(docs)), ctypes.c_uint64(n), ctypes.c_void_p(out.ctypes.data))
        exp = [[len(bytes(d[:b]).decode("utf-8", "replace")) for b in range(1, n + 1)] for d in docs]
        assert np.array_equal(np.cumsum(out, axis=1), np.asarray(exp)), n
