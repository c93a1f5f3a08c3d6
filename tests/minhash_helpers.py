"""Shapes the MinHash tests share (test_minhash_model.py on the CPU, test_gpu_minhash.py on the GPU): document lengths at
the edges of a piece (MH_TILE = 1,024 shingle positions) for an n-gram width, ids from a small alphabet that holds 0 and
2^32 - 1, and the plain-Python contract's result for a case, computed once per process."""
from __future__ import annotations

import functools

import numpy as np

from yet_another_bpe.tokenizer import BBPETokenizer

TILE = 1024
NGRAMS, PERMS = (1, 5, 32), (1, 64, 100, 128, 512)
BANDS = ((128, 1), (128, 32), (128, 128), (100, 100), (1, 1))  # (num_perm, bands)
ALPHABET = np.asarray([0, 0xFFFFFFFF] + list(range(1, 40)), np.uint32)


def edge_lengths(n: int) -> list[int]:
    return [0, 1, n - 1, n, n + 1, TILE + n - 2, TILE + n - 1, TILE + n, 3 * TILE + 7]


def batch_lengths(n: int) -> list[int]:
    """About 300 documents: empties first, last and adjacent; every edge length between short one-piece documents."""
    short = np.random.default_rng(n).integers(0, 3 * n + 2, 290).tolist()
    lens = [0, 0] + short[:100]
    for k, e in enumerate(edge_lengths(n)):
        lens += [e] + short[100 + 20 * k:120 + 20 * k]
    return lens + short[280:] + [0, 0]


@functools.lru_cache(maxsize=None)
def documents(lens: tuple) -> tuple:
    rng = np.random.default_rng(len(lens))
    return tuple(ALPHABET[rng.integers(0, len(ALPHABET), n)] for n in lens)


def flat(docs) -> tuple[np.ndarray, np.ndarray]:
    """-> (ids u32[n], doc_off u64[n_docs + 1])"""
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    return np.concatenate(docs + (np.zeros(0, np.uint32),)).astype(np.uint32), off


@functools.lru_cache(maxsize=None)
def contract(lens: tuple, num_perm: int, ngram: int, bands, seed: int = 7):
    """minhash_tokens over documents(lens) as arrays -> (sig u32[n_docs, num_perm], n_shingles, keys u64[n_docs, bands] or None)"""
    sig, cnt, keys = BBPETokenizer().minhash_tokens(documents(lens), num_perm=num_perm, ngram=ngram, bands=bands, seed=seed)
    return np.asarray(sig, np.uint32).reshape(len(lens), num_perm), np.asarray(cnt, np.uint64), None if keys is None else np.asarray(keys, np.uint64)
