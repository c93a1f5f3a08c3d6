"""CPU: the cases of tests/fim_helpers.py reach every branch of the fill-in-the-middle rule with the seeds chosen there --
checked on the plain Python's own draws, so a change of the rule or of a seed cannot leave the GPU tests testing nothing."""
from __future__ import annotations

from tests import fim_helpers as fh
from tests import mask_helpers as mh


def token_docs():
    """(case, document length, (mode, a, b), info after the cut) of every document of every token case"""
    for index, c in enumerate(fh.cases()):
        for n, draw, info in zip(c["lens"], fh.draws(index), fh.expected(index)[2]):
            yield c, n, draw, info


def test_cut_branches_at_token_level():
    seen = set()
    for _c, n, (mode, a, b), _info in token_docs():
        if mode and n >= 3:
            seen |= {("a == b", a == b), ("a == 0", a == 0 and b < n), ("b == n", b == n and a > 0), ("both", a == 0 and b == n), ("inner", 0 < a < b < n)}
    assert all((name, True) in seen for name in ("a == b", "a == 0", "b == n", "both", "inner")), sorted(seen)


def test_every_mode_and_modes_side_by_side():
    modes = set()
    mixed = False
    for index in range(len(fh.cases())):
        ms = [d[0] for d in fh.draws(index)]
        modes |= set(ms)
        mixed = mixed or any(x == 0 and y != 0 or x != 0 and y == 0 for x, y in zip(ms, ms[1:]))
    assert modes == {0, 1, 2} and mixed


def test_truncation_stages():
    stages = set()
    for c, n, (mode, a, b), (_mode, p, m, s) in token_docs():
        if not mode or not c["max_length"]:
            continue
        p0, m0, s0 = a, b - a, n - b
        if p + m + s == n:
            stages.add("fits")
        elif s > 0 and s < s0 and p == p0 and m == m0:
            stages.add("stops in the suffix")
        elif s == 0 and s0 > 0 and 0 < p < p0 and m == m0:
            stages.add("the whole suffix and part of the prefix")
        elif s == 0 and p == 0 and 0 < m < m0 and p0 > 0 and s0 > 0:
            stages.add("reaches the middle")
        assert p + m + s == min(n, c["max_length"] - 3 - (c["eot"] is not None))
    assert stages == {"fits", "stops in the suffix", "the whole suffix and part of the prefix", "reaches the middle"}
    left_alone_cut = [1 for c, n, (mode, _a, _b), info in token_docs() if not mode and c["max_length"] and n > c["max_length"] and info[1] == c["max_length"]]
    assert left_alone_cut


def test_every_option_value_appears():
    cs = fh.cases()
    assert {c["fim_rate"] for c in cs} == {c["spm_rate"] for c in cs} == set(fh.RATES)
    assert {(c["fim_rate"], c["spm_rate"]) for c in cs} == {(f, s) for f in fh.RATES for s in fh.RATES}
    assert {c["first_doc"] for c in cs} == {0, 7, 1 << 40} and {c["loss"] for c in cs} == {"all", "middle"}
    for eot in (None, fh.EOT):
        assert {c["max_length"] for c in cs if c["eot"] == eot} == set(fh.max_lengths(eot is not None))
        assert {c["loss"] for c in cs if c["eot"] == eot} == {"all", "middle"}
    for name, _lens, _off in fh.LENGTH_SETS:
        assert {c["max_length"] for c in cs if c["name"].startswith(name)} >= {None, 8, 300, 5000}


def test_cut_branches_at_character_level():
    tok = mh.tokenizer()
    seen = set()
    for k, seed, rate in fh.cut_runs():
        texts = fh.CUT_BATCHES[k]
        cuts = tok.fim_cuts(texts, fim_rate=rate, spm_rate=0.5, seed=seed, first_doc=3)
        starts = fh.piece_starts(texts, cuts).tolist()
        for t, (mode, a, b), (s0, s1, s2) in zip(texts, cuts, starts):
            n, end = len(t), s0 + len(t.encode("utf-8"))
            seen.add(("mode", mode))
            if not mode or n < 3:
                continue
            seen |= {("a == b", a == b), ("a == 0", a == 0), ("b == n", b == n), ("both", a == 0 and b == n)}
            for pos, at in ((s1, a), (s2, b)):
                if s0 < pos < end and pos % fh.GRANULE == 0:
                    seen.add("a cut on a granule boundary")
                if at < n and len(t[at].encode("utf-8")) > 1 and pos // fh.GRANULE != (pos + len(t[at].encode("utf-8")) - 1) // fh.GRANULE:
                    seen.add("a cut in front of a character that straddles a granule")
                if at < n and len(t[:at].encode("utf-8")) != at:
                    seen.add("a cut behind multi-byte characters")
    want = {("mode", 0), ("mode", 1), ("mode", 2), ("a == b", True), ("a == 0", True), ("b == n", True), ("both", True), "a cut on a granule boundary",
            "a cut behind multi-byte characters"}
    assert want <= seen, sorted(map(str, want - seen))
    # a character that straddles a granule seam exists in the buffers whether or not a cut lands in front of it
    blob = "".join(fh.CUT_BATCHES[-1]).encode("utf-8")
    assert blob[254:258] == "\U0001F600".encode("utf-8")
    assert fh.CUT_TEXTS[10].encode("utf-8")[62:66] == "\U0001F600".encode("utf-8")
    assert [len(t.encode("utf-8")) for t in fh.CUT_TEXTS[4:10]] == [63, 64, 65, 127, 128, 129]
