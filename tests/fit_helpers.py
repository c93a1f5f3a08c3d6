"""Shared by the whole-document packing tests: the plain-Python contract BBPETokenizer.encode_batch_fit on given ids as numpy
arrays, the row shapes read back from such a result, a literal one-by-one best-fit decreasing, and the counters of a call."""
from __future__ import annotations

import bisect
from collections import Counter

import numpy as np

from tests import layout_helpers as lh

TOK = lh.GivenIds()


def flags_of(bos, eos) -> int:
    return (1 if bos is not None else 0) | (2 if eos is not None else 0)


def kept_lengths(lens, C: int, n_added: int) -> list[int]:
    """n_d of every document"""
    return [min(n + n_added, C) for n in lens]


def contract(lens, C: int, bos=None, eos=None, pad=lh.PAD, ids=None):
    """-> (ids, doc, pos: u32[n_rows, C], used u32[n_rows]) of encode_batch_fit on synthetic ids (arange unless given)"""
    if ids is None:
        ids, _ = lh.synth(lens)
    out = TOK.encode_batch_fit(lh.contract_docs(ids, lens), C, pad_id=pad, bos_id=bos, eos_id=eos)
    return tuple(np.asarray(a, dtype=np.uint32).reshape(-1, C) for a in out[:3]) + (np.asarray(out[3], dtype=np.uint32),)


def row_shapes(doc: np.ndarray, pos: np.ndarray) -> list[tuple[int, ...]]:
    """the sequence lengths of every row, left to right (a sequence starts where pos is 0 in a filled slot)"""
    shapes = []
    for drow, prow in zip(doc.tolist(), pos.tolist()):
        filled = [c for c, d in enumerate(drow) if d != lh.NO_DOC]
        starts = [c for c in filled if prow[c] == 0] + [len(filled)]
        shapes.append(tuple(b - a for a, b in zip(starts[:-1], starts[1:])))
    return shapes


def literal_rooms(kept, C: int) -> Counter:
    """Best-fit decreasing one sequence at a time (decreasing length; the row with the smallest room that fits; else a new row)
    -> the multiset of the rooms left"""
    rooms: list[int] = []  # ascending
    for k in sorted((k for k in kept if k), reverse=True):
        i = bisect.bisect_left(rooms, k)
        left = (rooms.pop(i) if i < len(rooms) else C) - k
        bisect.insort(rooms, left)
    return Counter(rooms)


def stats(lens, C: int, n_added: int, n_rows: int):
    """-> (n_truncated_docs, n_ids_dropped, n_pad_slots) of a call"""
    seq = np.asarray(lens, dtype=np.int64) + n_added
    kept = np.minimum(seq, C)
    return int((seq > kept).sum()), int((seq - kept).sum()), int(n_rows * C - kept.sum())
