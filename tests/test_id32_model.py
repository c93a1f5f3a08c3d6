"""CPU: the width-parameterised per-position rules of yet-another-bpe_amd/csrc/tile_logic.h at u32 width
(tests/hostmodel/id32_model.cpp) against a literal Python rewrite (resume_helpers.replace_pair) and a literal recount, on
words that hold the ids around the old bound and the last u32 id; the pair key's round trip; and the u16 instantiation
against tests/hostmodel/tile_model.cpp on the same words."""
from __future__ import annotations

import ctypes
import random
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from tests import helpers, resume_helpers
from tests.test_hostmodel import model_lib  # noqa: F401  (the tile model's fixture)

HM = Path(__file__).resolve().parent / "hostmodel"
LAST = (1 << 24) - 3
SPECIAL_IDS = [0xFFFD, 0xFFFE, 0xFFFF, 0x10000, LAST]


@pytest.fixture(scope="module")
def lib():
    so, src = HM / "libid32_model.so", HM / "id32_model.cpp"
    hdr = HM.parent.parent / "yet-another-bpe_amd/csrc/tile_logic.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    L = ctypes.CDLL(str(so))
    L.id32_model_apply.restype = ctypes.c_int
    return L


def apply(lib, width, ids, a, b, c, w):
    n = len(ids)
    src = np.array(ids, dtype=np.uint32)
    out = np.zeros(n + 1, dtype=np.uint32)
    dl, dr = np.zeros(5 * n + 5, dtype=np.uint32), np.zeros(5 * n + 5, dtype=np.uint32)
    dv = np.zeros(5 * n + 5, dtype=np.int64)
    on, nd = ctypes.c_int(0), ctypes.c_int(0)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.id32_model_apply(width, vp(src), n, ctypes.c_uint32(a), ctypes.c_uint32(b), ctypes.c_uint32(c), ctypes.c_longlong(w), vp(out),
                              ctypes.byref(on), vp(dl), vp(dr), vp(dv), ctypes.byref(nd))
    assert rc == 0
    return out[:on.value].tolist(), {(int(dl[i]), int(dr[i])): int(dv[i]) for i in range(nd.value)}


def literal(ids, a, b, c, w):
    """The literal rewrite and the literal recount: ids as 4-byte strings, so that replace_pair's left + right names c."""
    enc = lambda t: int(t).to_bytes(4, "big")  # noqa: E731
    word = resume_helpers.replace_pair(tuple(enc(t) for t in ids), enc(a), enc(b))
    new = [c if len(t) == 8 else int.from_bytes(t, "big") for t in word]
    before, after = Counter(zip(ids, ids[1:])), Counter(zip(new, new[1:]))
    delta = {k: (after[k] - before[k]) * w for k in set(before) | set(after) if after[k] != before[k]}
    return new, delta


def test_u32_rules_against_the_literal_rewrite(lib):
    rng = random.Random(5)
    words = [[0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF], [0xFFFE] * 6, [LAST] * 7, [0x10000] * 2, [0xFFFD],
             [0xFFFE, 0xFFFF, 0xFFFE, 0xFFFF], [0xFFFF, 0x10000, 0xFFFF, 0x10000, 0xFFFF], [LAST, 0xFFFD, LAST, 0xFFFD, LAST, 0xFFFD],
             [7, 0xFFFF, 0xFFFF, 0xFFFF, 8, 0xFFFF, 0xFFFF], [0x10000, LAST, LAST, LAST, LAST, 0x10000]]
    for _ in range(300):
        al = rng.choice([SPECIAL_IDS, SPECIAL_IDS[:2], SPECIAL_IDS[2:4], [LAST, 5]])
        words.append([rng.choice(al) for _ in range(rng.randint(1, 40))])
    n_sites = 0
    for ids in words:
        for a in set(ids):
            for b in set(ids):
                c, w = rng.choice([LAST - 1, 0x10001, 300]), rng.choice([1, 3, (1 << 32) - 1])
                new, delta = literal(ids, a, b, c, w)
                got_new, got_delta = apply(lib, 32, ids, a, b, c, w)
                assert got_new == new and got_delta == delta, (ids, a, b, c)
                n_sites += len(ids) - len(new)
    assert n_sites > 2000


def test_pair_key_round_trip_and_sentinels(lib):
    lim = (ctypes.c_uint32 * 3)()
    lib.id32_model_limits(32, lim)
    assert list(lim) == [0xFFFFFFFF, 0xFFFFFFFE, (1 << 24) - 2]
    key, l2, r2, emp = ctypes.c_ulonglong(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
    seen = set()
    for left in [0, 1, 255, 0xFFFD, 0xFFFE, 0xFFFF, 0x10000, LAST - 1, LAST]:
        for right in [0, 1, 255, 0xFFFD, 0xFFFE, 0xFFFF, 0x10000, LAST - 1, LAST]:
            lib.id32_model_key(32, left, right, ctypes.byref(key), ctypes.byref(l2), ctypes.byref(r2), ctypes.byref(emp))
            assert (l2.value, r2.value) == (left, right) and not emp.value and key.value < 1 << 48
            seen.add(key.value)
    assert len(seen) == 81
    # the u16 instantiation means what the macros mean
    mac = (ctypes.c_uint32 * 4)()
    lib.id32_model_macros(mac)
    lib.id32_model_limits(16, lim)
    assert list(lim) == list(mac)[:3] == [0xFFFF, 0xFFFE, 0xFFFE]
    lib.id32_model_key(16, 0x1234, 0xABCD, ctypes.byref(key), ctypes.byref(l2), ctypes.byref(r2), ctypes.byref(emp))
    assert key.value == mac[3] and (l2.value, r2.value) == (0x1234, 0xABCD)
    lib.id32_model_key(16, 0xFFFD, 0xFFFD, ctypes.byref(key), ctypes.byref(l2), ctypes.byref(r2), ctypes.byref(emp))
    assert not emp.value


@pytest.mark.parametrize("width", [16, 32])
def test_both_widths_give_what_the_tile_model_gives(lib, model_lib, width):  # noqa: F811
    """The tile model (u16, tile_logic.h through its old names) trains on pooled words; replaying its merges word by word
    through the width-parameterised rules keeps a pair table whose count of every selected pair is the tile model's."""
    rng = random.Random(9)
    words = [bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 25))) for _ in range(150)] + [b"aaaaaaa", b"abababab", b"aa"]
    uw, fq = helpers.pooled(words)
    toks = helpers.base_tokens([])
    nm = 120
    flat, off = helpers.flatten(uw)
    tb = np.frombuffer(b"".join(toks), dtype=np.uint8).copy()
    to = np.zeros(len(toks) + 1, dtype=np.uint32)
    to[1:] = np.cumsum([len(t) for t in toks])
    L, R, M = (np.zeros(nm + 1, np.uint32) for _ in range(3))
    C = np.zeros(nm + 1, np.uint64)
    vp = ctypes.c_void_p
    n = model_lib.tile_model_train(vp(flat.ctypes.data), vp(off.ctypes.data), vp(fq.ctypes.data), ctypes.c_uint64(len(uw)), vp(tb.ctypes.data),
                                   vp(to.ctypes.data), ctypes.c_uint32(len(toks)), ctypes.c_uint32(nm), ctypes.c_uint64(1), 64, 32, 1,
                                   vp(L.ctypes.data), vp(R.ctypes.data), vp(M.ctypes.data), vp(C.ctypes.data))
    assert n > 50
    segs = [list(w) for w in uw]
    table: Counter = Counter()
    for ids, f in zip(segs, fq.tolist()):
        for pair in zip(ids, ids[1:]):
            table[pair] += f
    for i in range(n):
        a, b, c = int(L[i]), int(R[i]), int(M[i])
        assert table[(a, b)] == int(C[i]), i
        for k, (ids, f) in enumerate(zip(segs, fq.tolist())):
            new, delta = apply(lib, width, ids, a, b, c, f)
            segs[k] = new
            for pair, d in delta.items():
                table[pair] += d
        assert table[(a, b)] == 0
    recount: Counter = Counter()
    for ids, f in zip(segs, fq.tolist()):
        for pair in zip(ids, ids[1:]):
            recount[pair] += f
    assert {k: v for k, v in table.items() if v} == dict(recount)
