"""Shared by the layout tests: synthetic ids with document lengths from a list, the length grid, numpy references for both
layouts (np.repeat for `doc`, arange minus the repeated starts for `pos`), and the plain-Python contract run on given ids."""
from __future__ import annotations

import itertools

import numpy as np

from yet_another_bpe.tokenizer import BBPETokenizer

NO_DOC = 0xFFFFFFFF
ROW_LENS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65)
ADDED = ((None, None), (70001, None), (None, 70002), (70001, 70002))  # (bos, eos): n_added 0, 1, 1, 2
PAD = 70000


def grid_lengths(L: int, n_added: int) -> list[int]:
    """The document lengths around every edge of a row of L with n_added framing ids, and one document over many rows."""
    return [max(0, n) for n in (0, 1, L - 1, L, L + 1, L - n_added, L - n_added + 1, 10 * L + 3, 2, 0)]


def special_length_sets() -> dict[str, list[int]]:
    """Document lengths that take the packed write's other paths (a piece is 4,096 slots, its LDS window 2,048 offsets)."""
    rng = np.random.default_rng(5)
    return {
        "one document over two pieces": [5000],
        "a piece of only empty documents": [7] + [0] * 3000 + [9],
        "a window larger than the stage": [3, 1] + rng.integers(0, 4, 2049).tolist() + [4000],  # SCAN_TILE + 1 tiny documents
        "only empty documents": [0, 0, 0],
        "one empty document": [0],
        "many rows": rng.integers(0, 300, 40).tolist(),
    }


def synth(lens) -> tuple[np.ndarray, np.ndarray]:
    """-> (ids = arange(sum(lens)) as u32, the n_docs document starts as u64)"""
    lens = np.asarray(lens, dtype=np.int64)
    starts = np.zeros(max(len(lens), 1), dtype=np.uint64)
    starts[1:] = np.cumsum(lens)[:-1]
    return np.arange(int(lens.sum()), dtype=np.uint32), starts


def pad_cases():
    """(L, bos, eos, truncation left, padding left) over the whole grid"""
    for L, (bos, eos), tl, pl in itertools.product(ROW_LENS, ADDED, (False, True), (False, True)):
        if L >= (bos is not None) + (eos is not None):
            yield L, bos, eos, tl, pl


def pack_cases():
    """(L, bos, eos, drop_last) over the whole grid"""
    for L, (bos, eos), dl in itertools.product(ROW_LENS, ADDED, (False, True)):
        yield L, bos, eos, dl


def np_pad(ids, lens, L, pad, bos, eos, trunc_left, pad_left):
    """-> (rows u32[n, L], kept u32[n]); L None: the longest sequence"""
    ids, lens = np.asarray(ids, dtype=np.uint32), np.asarray(lens, dtype=np.int64)
    b, e = int(bos is not None), int(eos is not None)
    if L is None:
        L = int((lens + b + e).max()) if len(lens) else 0
    start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    kept = np.minimum(lens + b + e, L)
    kc = kept - b - e  # content ids kept
    p = np.arange(L, dtype=np.int64)[None, :] - ((L - kept)[:, None] if pad_left else 0)  # index into the kept sequence
    inside = (p >= 0) & (p < kept[:, None])
    content = inside & (p >= b) & (p < (kept - e)[:, None])
    src = (start + (lens - kc if trunc_left else 0))[:, None] + p - b
    rows = np.full((len(lens), L), pad, dtype=np.uint32)
    rows[content] = ids[src[content]]
    if b:
        rows[inside & (p == 0)] = bos
    if e:
        rows[inside & (p == (kept - 1)[:, None])] = eos
    return rows, kept.astype(np.uint32)


def np_pack(ids, lens, L, pad, bos, eos, drop_last):
    """-> (ids, doc, pos), each u32[n_rows, L]"""
    ids, lens = np.asarray(ids, dtype=np.uint32), np.asarray(lens, dtype=np.int64)
    b, e = int(bos is not None), int(eos is not None)
    seq = lens + b + e
    total = int(seq.sum())
    doc = np.repeat(np.arange(len(lens), dtype=np.int64), seq)
    pos = np.arange(total, dtype=np.int64) - np.repeat(np.concatenate(([0], np.cumsum(seq)))[:-1], seq)
    is_b = (pos == 0) if b else np.zeros(total, dtype=bool)
    is_e = (pos == np.repeat(seq, seq) - 1) if e else np.zeros(total, dtype=bool)
    stream = np.empty(total, dtype=np.uint32)
    stream[~(is_b | is_e)] = ids  # the content slots, in order, are the ids
    stream[is_b] = bos if b else 0
    stream[is_e] = eos if e else 0
    n_rows = total // L if drop_last else -(-total // L)
    out = []
    for flat, filler in ((stream, pad), (doc, NO_DOC), (pos, 0)):
        a = np.full(max(n_rows * L, total), filler, dtype=np.uint32)
        a[:total] = flat
        out.append(a[:n_rows * L].reshape(n_rows, L))
    return tuple(out)


class GivenIds(BBPETokenizer):
    """The plain-Python contract on given ids: every "text" is its list of ids."""

    def encode_batch(self, texts):
        return [list(t) for t in texts]


def contract_docs(ids, lens):
    off = np.concatenate(([0], np.cumsum(lens))).tolist()
    flat = np.asarray(ids).tolist()
    return [flat[off[d]:off[d + 1]] for d in range(len(lens))]


def pad_stats(lens, L, n_added):
    """-> (n_truncated_docs, n_ids_dropped, n_pad_slots) of a padded batch"""
    seq = np.asarray(lens, dtype=np.int64) + n_added
    kept = np.minimum(seq, L)
    return int((seq > kept).sum()), int((seq - kept).sum()), int(len(seq) * L - kept.sum())
