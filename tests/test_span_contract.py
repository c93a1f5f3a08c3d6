"""CPU: the statistical contract of BBPETokenizer.corrupt_spans, plain Python on 200,000 synthetic ids with fixed seeds at
(p, mean_span_length, max_span_length) = (0.15, 3, 10) and (0.5, 3, 10): the noise density, the mean drawn length, every run
below the sentinel cap in the target in order, and the document back from inputs and targets.

The density bound is derived, not measured: unit v is noise iff an opener in [v - Lmax + 1, v] reaches it, so the noise
indicators of units further than Lmax - 1 apart read disjoint draws and are independent.  With X the noise count of n units,
Var X = sum_v sum_w Cov(I_v, I_w) <= n * (2 Lmax - 1) * p (1 - p): each v has at most 2 Lmax - 1 partners w with a non-zero
covariance, each at most Var I = p (1 - p).  The test allows five such standard deviations around n p and nothing more.  (The
rule's own bias against p -- the first Lmax - 1 units of a document look back over fewer openers, here 90 units in all; the
bisection and the integer thresholds -- is some tens of units, against a bound of 3,481 and 4,873.)"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import pytest

from yet_another_bpe.synth import rnd_int
from yet_another_bpe.tokenizer import BBPETokenizer

N, N_DOCS, SENT_BASE = 200_000, 10, 1_000_000
SETTINGS = [(0.15, 3.0, 10, 31), (0.5, 3.0, 10, 32)]  # (p, mean, Lmax, seed)


@lru_cache(maxsize=None)
def drawn(index: int):
    """-> (documents, inputs, targets) with a sentinel for every run, computed once per setting"""
    p, mean, lmax, seed = SETTINGS[index]
    ids = np.random.default_rng(seed).integers(0, 50_000, N).tolist()
    docs = [ids[d * (N // N_DOCS):(d + 1) * (N // N_DOCS)] for d in range(N_DOCS)]
    sent = list(range(SENT_BASE, SENT_BASE + N // N_DOCS + 1))
    inputs, targets = BBPETokenizer().corrupt_spans(docs, sentinels=sent, p=p, mean_span_length=mean, max_span_length=lmax, seed=seed)
    return docs, inputs, targets


@pytest.mark.parametrize("index", range(len(SETTINGS)))
def test_noise_density(index):
    p, _mean, lmax, _seed = SETTINGS[index]
    docs, inputs, _targets = drawn(index)
    noise = sum(len(d) for d in docs) - sum(x < SENT_BASE for row in inputs for x in row)
    bound = 5 * math.sqrt(N * p * (1 - p) * (2 * lmax - 1))
    print(f"p {p}: {noise} noise ids of {N} ({noise / N:.4f}), allowed {N * p:.0f} +- {bound:.0f}")
    assert abs(noise - N * p) <= bound


@pytest.mark.parametrize("index", range(len(SETTINGS)))
def test_mean_drawn_length(index):
    p, mean, lmax, seed = SETTINGS[index]
    To, C = BBPETokenizer.span_thresholds(p, mean, lmax)
    S = [1.0] + [c / 2**32 for c in C]  # P(len > k); E len = sum_k P(len > k)
    lengths = []
    for d in range(N_DOCS):
        kd = rnd_int(seed, 0x63, d)
        for u in range(N // N_DOCS):
            r = rnd_int(kd, 0x6f, u)
            if (r >> 32) < To:
                lengths.append(1 + sum((r & 0xFFFFFFFF) < c for c in C))
    got, want = sum(lengths) / len(lengths), sum(S)
    print(f"p {p}: {len(lengths)} openers, mean drawn length {got:.4f}, sum S_k {want:.4f}, opening rate {len(lengths) / N:.5f} for {To / 2**32:.5f}")
    assert abs(got - want) <= 0.02 * want
    assert max(lengths) <= lmax and min(lengths) == 1
    assert want < mean  # the clamp at Lmax: mean_span_length is the mean before it


@pytest.mark.parametrize("index", range(len(SETTINGS)))
def test_runs_in_order_and_the_document_back(index):
    docs, inputs, targets = drawn(index)
    n_runs, run_len = 0, 0
    for doc, row, tgt in zip(docs, inputs, targets):
        # the target: sentinels SENT_BASE, SENT_BASE + 1, ... in order, each with at least one id, then the final one alone
        marks = [k for k, x in enumerate(tgt) if x >= SENT_BASE]
        assert [tgt[k] for k in marks] == list(range(SENT_BASE, SENT_BASE + len(marks))) and marks[0] == 0 and marks[-1] == len(tgt) - 1
        assert all(b - a > 1 for a, b in zip(marks, marks[1:]))
        runs = {tgt[a]: tgt[a + 1:b] for a, b in zip(marks, marks[1:])}
        # the input: the same sentinels in the same order, never two in a row (adjacent spans merge)
        assert [x for x in row if x >= SENT_BASE] == list(runs)
        assert not any(a >= SENT_BASE and b >= SENT_BASE for a, b in zip(row, row[1:]))
        back = []
        for x in row:
            back.extend(runs[x] if x >= SENT_BASE else [x])
        assert back == doc
        n_runs += len(runs)
        run_len += sum(len(r) for r in runs.values())
    p, mean, _lmax, _seed = SETTINGS[index]
    print(f"p {p}: {n_runs} runs, mean merged run {run_len / n_runs:.3f} (mean_span_length {mean})")
    assert run_len / n_runs > sum([1.0] + [c / 2**32 for c in BBPETokenizer.span_thresholds(*SETTINGS[index][:3])[1]])  # merged runs are longer


def test_the_cut_and_the_cap_reconstruct_too():
    docs, _inputs, _targets = drawn(0)
    docs = [d[:3000] for d in docs[:4]]
    sent = list(range(SENT_BASE, SENT_BASE + 20))  # (1,000 tokens at p = 0.15 hold about 46 runs)
    tok = BBPETokenizer()
    for final, cut in ((True, None), (False, 1000), (True, 2999)):
        inputs, targets = tok.corrupt_spans(docs, sentinels=sent, p=0.15, seed=31, final_sentinel=final, max_tokens=cut)
        K = len(sent) - final
        for doc, row, tgt in zip(docs, inputs, targets):
            marks = [k for k, x in enumerate(tgt) if x >= SENT_BASE] + ([] if final else [len(tgt)])
            runs = {tgt[a]: tgt[a + 1:b] for a, b in zip(marks, marks[1:])}
            assert len(runs) == K and list(runs) == sent[:K]  # more runs than sentinels: the cap holds
            assert not final or tgt[-1] == sent[K]
            back = []
            for x in row:
                back.extend(runs[x] if x >= SENT_BASE else [x])
            assert back == doc[:cut]
