"""Shared by the pair tests (encode_batch_pairs / yabpe_layout_pairs): the case grid, the pair lengths at every edge of the
rules, a numpy reference for the rows, their types, their per-row records and the spans of their slots, and the plain-Python
contract run on given ids (synthetic ids and GivenIds come from tests/layout_helpers.py).  Documents 2p and 2p + 1 of a list of
document lengths are the two sides of pair p."""
from __future__ import annotations

import itertools

import numpy as np

from tests.layout_helpers import PAD, GivenIds, contract_docs, synth  # noqa: F401 (re-exported)
from tests.window_helpers import n_rows_of, synth_spans  # noqa: F401 (re-exported)

BOS, EOS, SEP = 70001, 70002, 70003
MODES = ("longest_first", "only_first", "only_second", "windows")
ROW_LENS = (5, 7, 8, 64)


class GivenPairIds(GivenIds):
    """The plain-Python contract on given ids: every "text" of either side is its list of ids."""

    @staticmethod
    def _pair_texts(firsts, seconds):
        if len(firsts) != len(seconds):
            raise ValueError("firsts and seconds must be equally long")
        return list(firsts), list(seconds)


def n_added_of(bos, eos, sep, n_sep) -> int:
    return (bos is not None) + (eos is not None) + (n_sep if sep is not None else 0)


def pair_cases():
    """(max_length, mode, stride, bos, eos, sep, n_sep, padding left) over the whole grid: row lengths 5, 7, 8 and 64 (and 1 with
    nothing added), no / one / two separators, BOS and EOS each on and off, both sides, all four modes; windows mode with the
    strides {0, 1, C // 2, C - 1}"""
    shapes = [(1, None, None, None, 0)] + [(L, bos, eos, SEP if n_sep else None, n_sep) for L, bos, eos, n_sep in
                                           itertools.product(ROW_LENS, (None, BOS), (None, EOS), (0, 1, 2))]
    for (L, bos, eos, sep, n_sep), pl, mode in itertools.product(shapes, (False, True), MODES):
        C = L - n_added_of(bos, eos, sep, n_sep)
        if C < 1:
            continue
        for stride in (sorted({0, 1, C // 2, C - 1} & set(range(C))) if mode == "windows" else (0,)):
            yield L, mode, stride, bos, eos, sep, n_sep, pl


def pair_lengths(C: int, mode: str, stride: int) -> list[int]:
    """Document lengths, two a pair, at every edge of the rules for C content slots: la + lb around C, ties with odd and even
    sums, empty sides, a side that alone exceeds C; in windows mode also la around C - stride - 1 with lb at and one past the
    slots the second side has, an empty second and a second over many rows."""
    h = C // 2
    pairs = [(h, C - h - 1), (h, C - h), (h + 1, C - h), (C - h, h), (0, C - 1), (C + 1, 0), (1, C),  # sums C - 1, C, C + 1
             (h, h), (h + 1, h + 1), (C, C), (C + 1, C + 1),                                           # ties
             (0, 0), (0, 3), (3, 0), (0, C + 4), (C + 4, 0),                                            # empty sides
             (C + 3, 2), (2, C + 3), (C + 2, C + 5), (C + 5, C + 2), (3 * C + 1, 1), (1, 3 * C + 1)]   # a side alone exceeds C
    if mode == "windows":
        most = C - stride - 1  # the ids the first side keeps at most
        for la in sorted({max(0, most - 1), most, most + 1}):
            Cb = C - min(la, most)
            pairs += [(la, Cb), (la, Cb + 1), (la, 0), (la, Cb - 1), (la, 10 * C + 3), (la, 2 * Cb - stride), (la, 2 * Cb - stride + 1)]
    return [max(0, n) for pair in pairs for n in pair]


def np_keep(la, lb, C: int, mode: str):
    """what the two sides keep in a truncation mode, as arrays"""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    over = la + lb > C
    if mode == "longest_first":  # a side is cut to its half of the row, or to what the other leaves free if that is more
        h2 = C // 2
        ka, kb = np.minimum(la, np.maximum(C - h2, C - lb)), np.minimum(lb, np.maximum(h2, C - la))
    elif mode == "only_first":
        ka, kb = np.maximum(0, la - (la + lb - C)), np.minimum(lb, C)
    else:
        ka, kb = np.minimum(la, C), np.maximum(0, lb - (la + lb - C))
    return np.where(over, ka, la), np.where(over, kb, lb)


def np_pairs(ids, lens, L, mode, stride, pad, bos, eos, sep, n_sep, pad_left, spans=None):
    """-> (rows u32[R, L], types u8[R, L], row_pair, row_start, first_len, second_len: u32[R]) and, with spans u64[n, 2], the
    slots' u64[R, L, 2]"""
    ids, lens = np.asarray(ids, dtype=np.uint32), np.asarray(lens, dtype=np.int64)
    b, e = int(bos is not None), int(eos is not None)
    n_sep = n_sep if sep is not None else 0
    C = L - b - e - n_sep
    start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    la, lb, start_a, start_b = lens[0::2], lens[1::2], start[0::2], start[1::2]
    n_pairs = len(la)
    if mode == "windows":
        ka = np.minimum(la, C - stride - 1)
        Cb = C - ka
        step = Cb - stride
        per_pair = np.where(lb <= Cb, 1, 1 + -(-(lb - Cb) // step))
        row_pair = np.repeat(np.arange(n_pairs, dtype=np.int64), per_pair)
        row_start = (np.arange(int(per_pair.sum()), dtype=np.int64) - np.repeat(np.cumsum(per_pair) - per_pair, per_pair)) * step[row_pair]
        ka = ka[row_pair]
        kb = np.minimum(lb[row_pair] - row_start, Cb[row_pair])
    else:
        ka, kb = np_keep(la, lb, C, mode)
        row_pair, row_start = np.arange(n_pairs, dtype=np.int64), np.zeros(n_pairs, dtype=np.int64)
    kept = b + ka + n_sep + kb + e
    p = np.arange(L, dtype=np.int64)[None, :] - ((L - kept)[:, None] if pad_left else 0)  # index into the kept sequence
    inside = (p >= 0) & (p < kept[:, None])
    qa = p - b                          # index into the first side's kept ids
    qb = qa - ka[:, None] - n_sep       # index into the second side's
    is_a = inside & (qa >= 0) & (qa < ka[:, None])
    is_sep = inside & (qa >= ka[:, None]) & (qb < 0)
    is_b = inside & (qb >= 0) & (qb < kb[:, None])
    is_eos = inside & (p == (kept - 1)[:, None]) if e else np.zeros_like(inside)
    src_a = start_a[row_pair][:, None] + qa
    src_b = (start_b[row_pair] + row_start)[:, None] + qb
    rows = np.full((len(row_pair), L), pad, dtype=np.uint32)
    rows[is_a] = ids[src_a[is_a]]
    rows[is_b] = ids[src_b[is_b]]
    if n_sep:
        rows[is_sep] = sep
    if b:
        rows[inside & (p == 0)] = bos
    if e:
        rows[is_eos] = eos
    out = (rows, (is_b | is_eos).astype(np.uint8)) + tuple(a.astype(np.uint32) for a in (row_pair, row_start, ka, kb))
    if spans is None:
        return out
    spans = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    slot_spans = np.zeros((len(row_pair), L, 2), dtype=np.uint64)
    slot_spans[is_a] = spans[src_a[is_a]]
    slot_spans[is_b] = spans[src_b[is_b]]
    return out + (slot_spans,)


def as_arrays(out, L):
    """the lists encode_batch_pairs returns, as the arrays of np_pairs"""
    res = (np.asarray(out[0], dtype=np.uint32).reshape(-1, L), np.asarray(out[1], dtype=np.uint8).reshape(-1, L)) + tuple(
        np.asarray(a, dtype=np.uint32) for a in out[2:6])
    return res if len(out) == 6 else res + (np.asarray(out[6], dtype=np.uint64).reshape(-1, L, 2),)


def contract_pairs(lens, L, mode, stride, pad, bos, eos, sep, n_sep, pad_left):
    """encode_batch_pairs on the synthetic ids of `lens`, as arrays"""
    docs = contract_docs(synth(lens)[0], lens)
    out = GivenPairIds().encode_batch_pairs(docs[0::2], docs[1::2], L, truncation=mode, stride=stride, sep_id=sep, n_sep=n_sep, pad_id=pad,
                                            bos_id=bos, eos_id=eos, padding_side="left" if pad_left else "right")
    return as_arrays(out, L)


def pair_stats(lens, ref, L, n_added, mode):
    """-> (n_rows, n_truncated_docs, n_ids_dropped, n_pad_slots) of the call whose reference results are `ref`"""
    lens = np.asarray(lens, dtype=np.int64)
    la, lb = lens[0::2], lens[1::2]
    _rows, _types, row_pair, _row_start, first_len, second_len = (a.astype(np.int64) for a in ref[:6])
    n_rows = len(row_pair)
    n_pad = n_rows * L - int((first_len + second_len + n_added).sum())
    if mode == "windows":
        per_pair = np.bincount(row_pair, minlength=len(la))
        first_kept = np.zeros(len(la), dtype=np.int64)
        first_kept[row_pair] = first_len
        return n_rows, int(((per_pair > 1) | (first_kept < la)).sum()), 0, n_pad
    lost = la + lb - first_len - second_len
    return n_rows, int((lost > 0).sum()), int(lost.sum()), n_pad
