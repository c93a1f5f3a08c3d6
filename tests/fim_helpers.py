"""Shared by the fill-in-the-middle tests, CPU and GPU: the case lists that the CPU model (tests/hostmodel/fim_model.cpp),
yabpe_fim and yabpe_fim_cuts run against the plain-Python BBPETokenizer.fim_tokens / fim_cuts.  Token cases run on the
synthetic ids of tests/mask_helpers.py (ids below 1000, so an id of PRE or more in a result is a sentinel); a case carries the
rates 0, 0.5 and 1, whose thresholds are exactly 0, 2^31 and 2^32.  tests/test_fim_inputs.py pins that, with the seeds chosen
here, the cases reach every branch of the rule."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests import mask_helpers as mh
from yet_another_bpe.tokenizer import BBPETokenizer

PRE, SUF, MID, EOT = 9001, 9002, 9003, 9004
GRANULE = 64  # ENC_GRANULE: bytes per entry of the lead-byte table
RATES = (0.0, 0.5, 1.0)

# document lengths in ids: (name, lengths, doc_off given) -- a write block is 256 output slots
LENGTH_SETS = [
    ("lengths around a block", [0, 1, 2, 3, 255, 256, 257, 1000], True),
    ("300 documents of 0 or 1 ids", [(i * 7 % 5 != 0) * 1 for i in range(300)], True),
    ("runs of 40 empty documents", [0] * 40 + [5, 300] + [0] * 40 + [7] + [0] * 40, True),
    ("one document without doc_off", [77], False),
]


def threshold(rate: float) -> int:
    return min(1 << 32, int(rate * 4294967296.0))


def max_lengths(eot: bool):
    X = 3 + eot
    return (None, X + 1, X + 2, 8, 300, 5000)


def _case(name, lens, with_off, fim_rate, spm_rate, eot, loss, max_length, seed, first_doc, batch_seed=1):
    return {"name": name, "lens": list(lens), "with_off": with_off, "fim_rate": fim_rate, "spm_rate": spm_rate, "eot": EOT if eot else None, "loss": loss,
            "max_length": max_length, "seed": seed, "first_doc": first_doc, "batch_seed": batch_seed}


@lru_cache(maxsize=None)
def cases() -> tuple[dict, ...]:
    """Every (fim_rate, spm_rate) with every max_length on the first length set, eot, the loss and first_doc rotating so that
    each value meets each max_length; on the other sets one pass over the max_lengths with the rates rotating."""
    out = []
    first_docs = (0, 7, 1 << 40)
    k = 0
    name, lens, with_off = LENGTH_SETS[0]
    for fr in RATES:
        for sr in RATES:
            for m in range(6):
                eot, loss = bool((k + m) & 1), ("all", "middle")[(k // 2 + m // 2) & 1]
                ml = max_lengths(eot)[m]
                out.append(_case(f"{name}; fim {fr} spm {sr} eot {eot} loss {loss} max_length {ml} case {k}", lens, with_off, fr, sr, eot, loss, ml, 100 + k,
                                 first_docs[k % 3]))
                k += 1
    for name, lens, with_off in LENGTH_SETS[1:]:
        for m in range(6):
            for eot in (False, True):
                fr, sr = RATES[(k + 1) % 3] if m else 0.5, RATES[(k // 3) % 3]
                loss, ml = ("all", "middle")[(k // 2) & 1], max_lengths(eot)[m]
                out.append(_case(f"{name}; fim {fr} spm {sr} eot {eot} loss {loss} max_length {ml} case {k}", lens, with_off, fr, sr, eot, loss, ml, 100 + k,
                                 first_docs[k % 3]))
                k += 1
    return tuple(out)


CASE_IDS = [c["name"] for c in cases()]


def kwargs(c) -> dict:
    """the case as fim_tokens / fim_array take it"""
    return {"pre": PRE, "suf": SUF, "mid": MID, "eot": c["eot"], "fim_rate": c["fim_rate"], "spm_rate": c["spm_rate"], "seed": c["seed"],
            "first_doc": c["first_doc"], "max_length": c["max_length"], "loss": c["loss"]}


def native_kwargs(c) -> dict:
    """the case as _native.Context.fim takes it"""
    return {"seed": c["seed"], "first_doc": c["first_doc"], "fim": threshold(c["fim_rate"]), "spm": threshold(c["spm_rate"]), "pre_id": PRE, "suf_id": SUF,
            "mid_id": MID, "eot_id": c["eot"], "max_len": c["max_length"] or 0, "loss_middle": c["loss"] == "middle"}


@lru_cache(maxsize=None)
def batch(index: int) -> list[list[int]]:
    c = cases()[index]
    return mh.synth_batch(c["lens"], seed=c["batch_seed"])[0]


def counts_of(lens_in, seqs, info) -> dict:
    """what yabpe_fim_stats counts, from a plain-Python result (lens_in: the ids every document came in with)"""
    dropped = [n - (p + m + s) for n, (_mode, p, m, s) in zip(lens_in, info)]
    return {"n_docs": len(info), "n_psm": sum(i[0] == 1 for i in info), "n_spm": sum(i[0] == 2 for i in info),
            "n_truncated_docs": sum(x > 0 for x in dropped), "n_ids_dropped": sum(dropped), "n_out": sum(len(s) for s in seqs)}


@lru_cache(maxsize=None)
def expected(index: int):
    """-> (sequences, labels, info, counts) of token case `index` from the plain Python, computed once"""
    c = cases()[index]
    seqs, labels, info = BBPETokenizer().fim_tokens(batch(index), **kwargs(c))
    return seqs, labels, info, counts_of(c["lens"], seqs, info)


@lru_cache(maxsize=None)
def draws(index: int) -> list[tuple[int, int, int]]:
    """(mode, a, b) of every document of token case `index`"""
    c = cases()[index]
    return [BBPETokenizer._fim_draw(c["seed"], c["first_doc"] + d, n, threshold(c["fim_rate"]), threshold(c["spm_rate"])) for d, n in enumerate(c["lens"])]


@lru_cache(maxsize=None)
def pieces(index: int):
    """Token case `index` as the pieces route sees it: every document split at two places that the rule did NOT draw (its
    draws under another seed), the modes the rule's own -> (piece lengths, 3 per document; cuts u64[n, 3]; expected
    (sequences, labels, info, counts))."""
    c = cases()[index]
    tok = BBPETokenizer()
    pre, suf, mid, eot, _Tf, _Ts, _seed, _fd, max_len, loss_middle = tok._fim_args(PRE, SUF, MID, c["eot"], c["fim_rate"], c["spm_rate"], 0, 0,
                                                                                    c["max_length"], c["loss"])
    lens3, cuts, seqs, labels, info = [], [], [], [], []
    for d, (ids, (mode, _a, _b)) in enumerate(zip(batch(index), draws(index))):
        _m, a, b = BBPETokenizer._fim_draw(c["seed"] + 77, d, len(ids), 1 << 32, 0)
        lens3 += [a, b - a, len(ids) - b]
        cuts.append((mode, 1000 + d, 2000 + d))  # (a and b in characters: never read)
        seq, lab, inf = tok._fim_sequence(mode, ids[:a], ids[a:b], ids[b:], pre, suf, mid, eot, max_len, loss_middle)
        seqs.append(seq)
        labels.append(lab)
        info.append(inf)
    return lens3, np.asarray(cuts, np.uint64).reshape(-1, 3), (seqs, labels, info, counts_of(c["lens"], seqs, info))


def flat_arrays(index: int):
    """-> (ids u32, document starts u64 or None) of token case `index`, as the C ABI takes them"""
    c = cases()[index]
    return mh.flat(batch(index), np.uint32), mh.starts(c["lens"]) if c["with_off"] else None


def ragged(flat, off) -> list[list[int]]:
    flat, off = np.asarray(flat).tolist(), np.asarray(off).tolist()
    return [flat[off[d]:off[d + 1]] for d in range(len(off) - 1)]


# ---------------------------------------------------------------- texts for the character-level cuts
def _bytes_long(n: int, wide: str) -> str:
    """a text of exactly n UTF-8 bytes: `wide` characters and ASCII letters mixed"""
    out, size, k = [], 0, 0
    w = len(wide.encode("utf-8"))
    while size < n:
        if k % 3 == 1 and size + w <= n:
            out.append(wide)
            size += w
        else:
            out.append("abcdefghij"[k % 10])
            size += 1
        k += 1
    return "".join(out)


CUT_TEXTS = [
    "plain ASCII text, nothing else in it",
    "aé€\U0001F600 mixed: naïve €5 \U0001F680 café 한국어 done",
    "\U0001F600" * 20,
    "",
    _bytes_long(63, "é"), _bytes_long(64, "€"), _bytes_long(65, "\U0001F600"),
    _bytes_long(127, "é"), _bytes_long(128, "€"), _bytes_long(129, "\U0001F600"),
    "a" * 62 + "\U0001F600" + "b" * 10,  # the 4-byte character takes bytes 62 .. 65 of its document
    "",
    "é",
    "x",
    "€" * 43,
    "",
]
# the same documents as neighbours in one buffer, then once more behind a 2-byte character (every granule seam moves), with a
# 4-byte character over the seam at byte 256 of the buffer
_PAD = "é"
CUT_BATCHES = [[t] for t in CUT_TEXTS] + [CUT_TEXTS, [_PAD] + CUT_TEXTS + ["y" * 3], ["a" * 254 + "\U0001F600" + "b" * 40, "", "tail"]]
CUT_SEEDS = (0, 1, 2, 3)  # every batch runs under each, fim_rate 1 (and once under 0.5)


@lru_cache(maxsize=None)
def encode_docs() -> tuple[str, ...]:
    """texts for the encode route: empty documents, specials alone, specials inside text, digit runs, a document of more than
    a block of ids, non-ASCII text, and 40 short documents with a special in each"""
    words = mh.corpus_words()
    base = ["", "[MASK]", "<|endoftext|>[PAD]", "Hello [MASK] world <|endoftext|> done [PAD] and more text here", "In 1234567 we paid 89012.50 for 007",
            " ".join(words[(5 * i) % len(words)] for i in range(400)), "naïve café — 한국어 \U0001F600 text", ""]
    return tuple(base + [f"{words[i]} it's {i * 7}. [MASK] {words[i + 1]}" for i in range(40)])


def special_hits(tok, text: str, a: int, b: int) -> tuple[bool, bool]:
    """-> (a cut lies strictly inside an occurrence of a special token, an occurrence lies wholly inside one piece) for the
    cuts (a, b) of normalize(text)"""
    t = tok.normalize(text)
    under = inside = False
    for s in tok.special_tokens:
        k = t.find(s)
        while k >= 0:
            e = k + len(s)
            under = under or k < a < e or k < b < e
            inside = inside or not (k < a < e or k < b < e)
            k = t.find(s, k + 1)
    return under, inside


def encode_seed(tok, docs, **kw) -> int:
    """the first seed under which, at character level, one document has a cut inside a special token's occurrence, another a
    special inside a piece, and a third is left alone"""
    for seed in range(2000):
        cuts = tok.fim_cuts(docs, seed=seed, **kw)
        hits = [special_hits(tok, t, a, b) for t, (mode, a, b) in zip(docs, cuts) if mode]
        if any(h[0] for h in hits) and any(h[1] for h in hits) and any(c[0] == 0 for c in cuts) and {c[0] for c in cuts} == {0, 1, 2}:
            return seed
    raise AssertionError("no seed in 0 .. 1999 gives the situation")


def piece_starts(texts, cuts) -> np.ndarray:
    """the byte starts (document, middle, suffix) in the buffer of the documents back to back -> u64[n, 3]"""
    out, base = [], 0
    for t, (_mode, a, b) in zip(texts, cuts):
        out.append((base, base + len(t[:a].encode("utf-8")), base + len(t[:b].encode("utf-8"))))
        base += len(t.encode("utf-8"))
    return np.asarray(out, np.uint64).reshape(-1, 3)


def cut_runs():
    """-> (batch index, seed, fim_rate) of every run of the cut tests"""
    return [(k, seed, 1.0) for k in range(len(CUT_BATCHES)) for seed in CUT_SEEDS] + [(k, 9, 0.5) for k in range(len(CUT_BATCHES))]
