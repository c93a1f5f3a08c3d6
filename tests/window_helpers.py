"""Shared by the window tests (encode_batch_windows / yabpe_layout_windows): the case grid, a numpy reference for the rows, their
records and the spans of their slots, and the plain-Python contract run on given ids (synthetic ids and GivenIds come from
tests/layout_helpers.py)."""
from __future__ import annotations

import itertools

import numpy as np

from tests.layout_helpers import ADDED, PAD, ROW_LENS, GivenIds, contract_docs, synth  # noqa: F401 (re-exported)


def win_cases():
    """(max_length, stride, bos, eos, padding left) over the whole grid: every row length with at least one content slot, the
    strides {0, 1, C // 2, C - 1}"""
    for L, (bos, eos), pl in itertools.product(ROW_LENS, ADDED, (False, True)):
        C = L - (bos is not None) - (eos is not None)
        if C >= 1:
            for stride in sorted({0, 1, C // 2, C - 1} & set(range(C))):
                yield L, stride, bos, eos, pl


def win_lengths(L: int, n_added: int, stride: int) -> list[int]:
    """The document lengths around the first and the second row's end, and one document over many rows."""
    C = L - n_added
    step = C - stride
    return [max(0, n) for n in (0, 1, C - 1, C, C + 1, C + step - 1, C + step, C + step + 1, 2 * C, 10 * L + 3, 2, 0)]


def synth_spans(n: int) -> np.ndarray:
    """spans[i] = (2 i, 2 i + 1): a wrong gather shows"""
    return np.arange(2 * n, dtype=np.uint64).reshape(n, 2)


def n_rows_of(lens, C: int, step: int) -> np.ndarray:
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= C, 1, 1 + -(-(lens - C) // step))


def np_windows(ids, lens, L, stride, pad, bos, eos, pad_left, spans=None):
    """-> (rows u32[R, L], row_doc u32[R], row_start u32[R], lengths u32[R]) and, with spans u64[n, 2], the slots' u64[R, L, 2]"""
    ids, lens = np.asarray(ids, dtype=np.uint32), np.asarray(lens, dtype=np.int64)
    b, e = int(bos is not None), int(eos is not None)
    C = L - b - e
    step = C - stride
    start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    per_doc = n_rows_of(lens, C, step)
    row_doc = np.repeat(np.arange(len(lens), dtype=np.int64), per_doc)
    row_start = (np.arange(int(per_doc.sum()), dtype=np.int64) - np.repeat(np.cumsum(per_doc) - per_doc, per_doc)) * step
    kept = np.minimum(lens[row_doc] - row_start, C) + b + e
    p = np.arange(L, dtype=np.int64)[None, :] - ((L - kept)[:, None] if pad_left else 0)  # index into the kept sequence
    inside = (p >= 0) & (p < kept[:, None])
    content = inside & (p >= b) & (p < (kept - e)[:, None])
    src = (start[row_doc] + row_start)[:, None] + p - b
    rows = np.full((len(row_doc), L), pad, dtype=np.uint32)
    rows[content] = ids[src[content]]
    if b:
        rows[inside & (p == 0)] = bos
    if e:
        rows[inside & (p == (kept - 1)[:, None])] = eos
    out = (rows, row_doc.astype(np.uint32), row_start.astype(np.uint32), kept.astype(np.uint32))
    if spans is None:
        return out
    slot_spans = np.zeros((len(row_doc), L, 2), dtype=np.uint64)
    slot_spans[content] = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)[src[content]]
    return out + (slot_spans,)


def contract_windows(lens, L, stride, pad, bos, eos, pad_left):
    """encode_batch_windows on the synthetic ids of `lens`, as arrays"""
    ids, _ = synth(lens)
    out = GivenIds().encode_batch_windows(contract_docs(ids, lens), L, stride, pad_id=pad, bos_id=bos, eos_id=eos,
                                          padding_side="left" if pad_left else "right")
    return (np.asarray(out[0], dtype=np.uint32).reshape(-1, L),) + tuple(np.asarray(a, dtype=np.uint32) for a in out[1:])


def win_stats(lens, L, n_added, stride):
    """-> (n_rows, n_truncated_docs, n_pad_slots) of a windows batch"""
    C = L - n_added
    lens = np.asarray(lens, dtype=np.int64)
    per_doc = n_rows_of(lens, C, C - stride)
    kept = lens + (per_doc - 1) * stride + per_doc * n_added  # every row but the first repeats `stride` ids
    return int(per_doc.sum()), int((per_doc > 1).sum()), int(per_doc.sum() * L - kept.sum())
