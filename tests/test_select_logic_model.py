"""CPU: the rules of the candidate list and of the selection's window (yet-another-bpe_amd/csrc/select_logic.h) run by
tests/hostmodel/select_model.cpp.  The listing rule before the "listed" bitmap (a count that crosses the threshold again is
listed again) against the rule with it (one bit per slot, a crossing lists only if the bit was clear), over random tables
and random sequences of adds:
  - the SET of listed slots is the same, the new list holds no slot twice, and every slot with count >= T is on it;
  - the bitmap names exactly the listed slots (the rebuild writes every word, stale ones included);
  - the window (as a set), its size, the floor, the number of narrowing steps and the fallback decision are the same;
  - a list permuted at random gives the same window.
Among the cases: more than WIN distinct pairs at the top (no window) and within 16 of it (the window is narrowed)."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

HM = Path(__file__).resolve().parent / "hostmodel"
U64, U32, I64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
WIN, KMAX = 128, 16


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libselect_model.so", HM / "select_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "select_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.sel_win_attempts.restype = U32
    lib.sel_list_replay.restype = U32
    lib.sel_list_replay.argtypes = [U32, U64, ctypes.c_void_p, U32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, U32, ctypes.c_void_p]
    lib.sel_window.restype = None
    lib.sel_window.argtypes = [U32, ctypes.c_void_p, ctypes.c_void_p, U32, U32, U64, U32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def replay(model, counts, T, ev_slot, ev_delta, rule):
    """-> (list of slots, counts afterwards, bitmap words)"""
    cnt = np.array(counts, dtype=np.int64)
    es, ed = np.array(ev_slot, dtype=np.uint32), np.array(ev_delta, dtype=np.int64)
    cap = len(cnt) + len(es) + 1
    out = np.zeros(cap, dtype=np.uint32)
    bits = np.zeros((len(cnt) + 63) // 64, dtype=np.uint64)
    n = model.sel_list_replay(len(cnt), T, cnt.ctypes.data, len(es), es.ctypes.data if len(es) else None, ed.ctypes.data if len(ed) else None, rule,
                              out.ctypes.data, cap, bits.ctypes.data)
    assert n <= cap
    return out[:n].tolist(), cnt, bits


def window(model, lst, counts, kmax, wshift, T, rule):
    """-> (L, n_win, narrowed, fallback, attempts, frozenset of window slots)"""
    la = np.array(lst, dtype=np.uint32)
    cnt = np.array(counts, dtype=np.int64)
    out = np.zeros(5, dtype=np.uint64)
    wnd = np.zeros(WIN, dtype=np.uint32)
    model.sel_window(len(la), la.ctypes.data if len(la) else None, cnt.ctypes.data, kmax, wshift, T, WIN, rule, out.ctypes.data, wnd.ctypes.data)
    L, n, narrowed, fallback, attempts = (int(v) for v in out)
    return L, n, narrowed, fallback, attempts, frozenset(wnd[:n].tolist())


def random_table(rng: random.Random, kind: str):
    """-> (counts by slot, T, ceiling of the adds or None): `kind` shapes the top of the table."""
    n_slots = rng.choice([1, 63, 64, 65, 200, 1000, 3000])
    top = rng.choice([1, 5, 40, 1000, 10 ** 6, 1 << 33])
    if kind == "spread":
        counts = [rng.randrange(0, top + 1) for _ in range(n_slots)]
    elif kind == "plateau":  # more than WIN slots tie at the top
        n_slots = max(n_slots, 400)
        counts = [top if rng.random() < 0.6 else rng.randrange(0, top + 1) for _ in range(n_slots)]
    else:  # "near": a small top level, more than WIN slots within 16 of it
        n_slots = max(n_slots, 400)
        top = max(top, 40)
        counts = [top - rng.randrange(1, 17) if rng.random() < 0.7 else rng.randrange(0, top) for _ in range(n_slots)]
        for s in rng.sample(range(n_slots), rng.randrange(1, 20)):
            counts[s] = top
    T = max(1, int(top * rng.choice([0.0, 0.3, 0.8, 0.95, 1.0])))
    return counts, T, (None if kind == "spread" else top)


def random_events(rng: random.Random, counts, T, ceiling=None):
    """Adds that move slots across T in both directions, some of them more than once; a few transiently negative counts.
    With a ceiling no add takes a count above it, so the top level the table was given stays the top."""
    n = len(counts)
    cur = list(counts)
    hot = [rng.randrange(n) for _ in range(max(1, min(n, 12)))]
    ev_slot, ev_delta = [], []
    for _ in range(rng.randrange(0, 400)):
        s = rng.choice(hot) if rng.random() < 0.7 else rng.randrange(n)
        d = rng.choice([1, -1, T, -T, T // 2 + 1, -(T // 2 + 1), rng.randrange(-3 * T - 3, 3 * T + 4)])
        if ceiling is not None and cur[s] + d > ceiling:
            d = ceiling - cur[s]
        if d:
            cur[s] += d
            ev_slot.append(s)
            ev_delta.append(d)
    return ev_slot, ev_delta


KINDS = ["spread", "plateau", "near"]


@pytest.mark.parametrize("kind", KINDS)
def test_same_slots_listed_and_none_twice(model, kind):
    rng = random.Random({"spread": 1, "plateau": 2, "near": 3}[kind])
    recross = 0
    for _ in range(150):
        counts, T, ceiling = random_table(rng, kind)
        ev_slot, ev_delta = random_events(rng, counts, T, ceiling)
        old_list, old_cnt, _ = replay(model, counts, T, ev_slot, ev_delta, 0)
        new_list, new_cnt, bits = replay(model, counts, T, ev_slot, ev_delta, 1)
        assert np.array_equal(old_cnt, new_cnt)
        assert set(old_list) == set(new_list)
        assert len(new_list) == len(set(new_list))                      # no slot twice
        recross += len(old_list) - len(set(old_list))
        assert {s for s, c in enumerate(new_cnt.tolist()) if c > 0 and c >= T} <= set(new_list)  # every slot >= T is listed
        listed = {w * 64 + b for w, word in enumerate(bits.tolist()) for b in range(64) if (word >> b) & 1}
        assert listed == set(new_list)                                  # the bitmap names exactly the list
    assert recross > 100, recross  # (the inputs do cross again: the old rule listed slots twice)


@pytest.mark.parametrize("kind", KINDS)
def test_same_window_from_both_lists_and_any_order(model, kind):
    rng = random.Random({"spread": 11, "plateau": 12, "near": 13}[kind])
    seen = {"narrowed": 0, "fallback": 0, "repeats": 0, "fits": 0}
    for _ in range(150):
        counts, T, ceiling = random_table(rng, kind)
        ev_slot, ev_delta = random_events(rng, counts, T, ceiling)
        old_list, cnt, _ = replay(model, counts, T, ev_slot, ev_delta, 0)
        new_list, _, _ = replay(model, counts, T, ev_slot, ev_delta, 1)
        seen["repeats"] += len(old_list) != len(new_list)
        for kmax in (1, 2, KMAX):
            wshift = rng.randrange(1, 21)
            a = window(model, old_list, cnt, kmax, wshift, T, 0)
            b = window(model, new_list, cnt, kmax, wshift, T, 1)
            assert a == b, (kind, kmax, wshift, T, a[:5], b[:5])
            perm = new_list[:]
            rng.shuffle(perm)
            assert window(model, perm, cnt, kmax, wshift, T, 1) == b    # nothing depends on the order of the list
            L, n, narrowed, fallback, attempts, wnd = b
            assert n == len(wnd) <= WIN and attempts <= model.sel_win_attempts()
            cl = cnt.tolist()
            if n:  # the window is every listed slot with count >= L, whole count levels
                assert wnd == {s for s in new_list if cl[s] > 0 and cl[s] >= L}
            seen["narrowed"] += narrowed > 0 and n > 0
            seen["fallback"] += fallback
            seen["fits"] += n > 0 and narrowed == 0
    assert seen["repeats"] > 20, seen
    if kind == "plateau":
        assert seen["fallback"] > 50, seen   # more than WIN distinct pairs tie at the top: no window
    if kind == "near":
        assert seen["narrowed"] > 50, seen   # more than WIN within 16 of the top, fewer at the top: narrowed until it fits
    if kind == "spread":
        assert seen["fits"] > 50, seen


def test_named_windows(model):
    """Hand-made tops: exactly WIN and WIN + 1 at the top; WIN + 1 within 16 of a top of one; a list that holds only repeats."""
    T, big = 10, 1000
    for n_top, want_fallback in ((WIN, 0), (WIN + 1, 1)):
        counts = [big] * n_top + [1] * 50
        lst = list(range(len(counts)))
        for rule in (0, 1):
            L, n, narrowed, fallback, _, wnd = window(model, lst, counts, KMAX, 1, T, rule)
            assert fallback == want_fallback and n == (0 if want_fallback else WIN), (n_top, rule, n, fallback)
    counts = [big] + [big - 1 - (i % 16) for i in range(WIN + 40)]
    lst = list(range(len(counts)))
    a, b = window(model, lst + lst, counts, KMAX, 20, T, 0), window(model, lst, counts, KMAX, 20, T, 1)
    assert a == b and b[2] > 0 and 0 < b[1] <= WIN and not b[3], b[:5]
    # below T the maximum is not proven by the list (the stop rules ask for a rescan); the floor then follows cmax alone
    a, b = window(model, [3, 3, 3], [0, 0, 0, 7], KMAX, 1, T, 0), window(model, [3], [0, 0, 0, 7], KMAX, 1, T, 1)
    assert a == b and b[1] == 1 and b[5] == {3}
    # nothing positive on the list: no window and no fallback
    assert window(model, [0, 1], [0, -5], KMAX, 1, T, 1)[:4] == (0, 0, 0, 0)
