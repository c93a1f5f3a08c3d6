"""CPU: the training driver's decisions (yet-another-bpe_amd/csrc/train_rules.h) run by tests/hostmodel/train_rules_model.cpp.
Every rule is restated here in Python from the expressions the driver used before they were gathered in that header (unsigned
32- and 64-bit arithmetic written out with masks), and compared on seeded random inputs and on the edges; the production
points that DESIGN.md quotes are pinned; the launch shape's invariants hold whatever the inputs."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import pytest

HM = Path(__file__).resolve().parent / "hostmodel"
U64, U32, I64, INT = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
BLOCK, AGG_N, KMAX, MAX_LISTS, MAX_APPLY_BLOCKS, WPB, YB_MAX_TOKENS = 256, 1024, 16, 2048, 8192, 4, 0xFFFE


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libtrain_rules_model.so", HM / "train_rules_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "train_rules.h", csrc / "steal_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    sig = {
        "rules_opt_unset": (I64, []),
        "rules_scan_kt_max": (U32, [U32]),
        "rules_max_lists": (U32, []),
        "rules_count_grid": (U32, [U32, U32, U32, I64]),
        "rules_sparse_geom": (None, [U32, U32, U64, INT, U32, I64, I64, I64, I64, I64, ctypes.POINTER(U32)]),
        "rules_want_sparse": (INT, [U32, INT, INT, U64, U64, I64]),
        "rules_sparse_now": (INT, [I64, INT]),
        "rules_cand_rebuild": (INT, [INT, U32, U32, I64, U64, U64, U64, U32, I64]),
        "rules_sig_rebuild": (INT, [INT, U32, U32, I64, U64, U64, I64]),
        "rules_xeff_next": (U32, [ctypes.POINTER(U32), U32, I64, I64, I64, I64]),
        "rules_xeff_after_full": (U32, [U32, U32]),
        "rules_round_launches": (U32, [INT, INT, U32]),
        "rules_round_kmax": (U32, [INT, I64]),
        "rules_round_records": (U32, [U32, U32, U32, U32]),
        "rules_rec_first": (U32, [U32]),
        "rules_tok_upper": (U32, [U32, U32, U32]),
        "rules_partials": (U32, [U64]),
        "rules_table_grow": (INT, [U64, U64, I64]),
        "rules_table_grow_target": (U64, [U64, I64, U64]),
        "rules_retile": (INT, [U32, U64, U64, I64, INT]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


# ------------------------------------------------------------------------------------------------ the sparse launch's shape
def py_piece_tiles(rest, blocks, chunk):
    p = (rest + max(blocks, 1) - 1) // max(blocks, 1)
    p = (p + 63) // 64 * 64
    return min(max(p, 256), chunk)


def py_geom(n_tiles, n_cu, best, weighted, kmax_now, full_wpb, wide, skip_blocks, steal, agg_small):
    """skip_blocks None: the option is not set."""
    wpb = full_wpb
    if wpb <= 0:
        wpb = 16 if (best <= (wide * n_cu) & M64 and ((n_tiles + 2047) & M32) // 2048 <= n_cu) else 8
    nw = 16 if wpb >= 16 else 8
    nt = nw * 64
    target = max(1, n_cu * (16 // nw) if skip_blocks is None else skip_blocks) & M32
    ktm = 2 if nw >= 16 else 4
    chunk = min(nt * ktm, max(64, ((((n_tiles + target - 1) & M32) // target + 63) // 64 * 64) & M32))
    kt = (chunk + nt - 1) // nt
    n_chunks = ((n_tiles + chunk - 1) & M32) // chunk
    scan_grid = max(1, min(n_chunks, target, MAX_LISTS))
    rest = n_tiles - min(n_tiles, scan_grid * chunk)
    pieces = 1 if (rest and nw == 8 and steal) else 0
    piece = 0 if not rest else py_piece_tiles(rest, scan_grid, chunk) if pieces else chunk
    n_pieces = (rest + piece - 1) // piece if pieces else 0
    agg_mask = AGG_N - 1
    if agg_small and not weighted and (best * 4) & M64 < 48 * max(1, n_cu * 3):
        agg_mask = (AGG_N if kmax_now > 2 else AGG_N // 2 if nw >= 16 else AGG_N // 4) - 1
    return (nw, chunk, kt, scan_grid, rest, pieces, piece, n_pieces, agg_mask)


def c_geom(model, n_tiles, n_cu, best, weighted, kmax_now, full_wpb, wide, skip_blocks, steal, agg_small):
    out = (U32 * 9)()
    model.rules_sparse_geom(n_tiles, n_cu, best, int(weighted), kmax_now, full_wpb, wide, model.rules_opt_unset() if skip_blocks is None else skip_blocks,
                            steal, agg_small, out)
    return tuple(out)


def geom_cases():
    rng = random.Random(20)
    cases = []
    for n_cu in (1, 256):
        for full_wpb in (0, 8, 16):
            nw_set = (8, 16) if full_wpb == 0 else (full_wpb,)
            for skip_blocks in (None, 1, 2, 3, 512, 5000):
                edges = {0, 1, 63, 64, 65}
                for nw in nw_set:
                    target = n_cu * (16 // nw) if skip_blocks is None else skip_blocks
                    full = nw * 64 * (2 if nw == 16 else 4) * min(target, MAX_LISTS)  # one round of full chunks: rest = 0 up to here
                    edges |= {full - 1, full, full + 1, full + 100, full + 255, full + 256, 2 * full + 7, 3 * full}
                for n_tiles in sorted(e for e in edges if 0 <= e < 1 << 31):
                    for best in (0, 20 * n_cu - 1, 20 * n_cu, 20 * n_cu + 1, 10 ** 9):  # either side of wide_sites_per_cu * n_cu
                        cases.append((n_tiles, n_cu, best, rng.random() < 0.5, rng.choice((1, 2, 3, 16)), full_wpb, 20, skip_blocks, rng.choice((0, 1)), rng.choice((0, 1))))
    for _ in range(4000):
        n_cu = rng.choice((1, 256, rng.randrange(1, 400)))
        wide = rng.choice((20, 0, rng.randrange(0, 1000)))
        best = rng.choice((rng.randrange(0, 1 << rng.randrange(1, 40)), max(0, wide * n_cu + rng.randrange(-2, 3)), rng.randrange(0, 40 * n_cu * 3)))
        cases.append((rng.randrange(0, 1 << rng.randrange(1, 32)), n_cu, best, rng.random() < 0.5, rng.randrange(1, 17), rng.choice((0, 0, 8, 16, -1, 4, 32)),
                      wide, rng.choice((None, None, rng.randrange(1, 5000), rng.randrange(-2, 3))), rng.choice((0, 1, 1)), rng.choice((0, 1, 1))))
    return cases


def test_sparse_geometry_equals_the_restated_rule_and_keeps_its_invariants(model):
    seen = {"rest0": 0, "rest_small": 0, "rest_big": 0, "nw16": 0, "pieces": 0, "agg": 0}
    for case in geom_cases():
        got = c_geom(model, *case)
        assert got == py_geom(*case), case
        nw, chunk, kt, scan_grid, rest, pieces, piece, n_pieces, agg_mask = got
        n_tiles = case[0]
        assert nw in (8, 16) and scan_grid >= 1 and 1 <= kt <= model.rules_scan_kt_max(nw) and chunk % 64 == 0 and chunk >= 64, (case, got)
        assert chunk <= nw * 64 * kt and scan_grid <= MAX_LISTS, (case, got)
        assert rest == max(0, n_tiles - scan_grid * chunk) and agg_mask in (255, 511, 1023), (case, got)
        if pieces:
            assert nw == 8 and scan_grid * chunk + n_pieces * piece >= n_tiles and piece % 64 == 0 and (n_pieces - 1) * piece < rest, (case, got)
        else:
            assert n_pieces == 0 and piece == (chunk if rest else 0), (case, got)
        seen["rest0"] += rest == 0
        seen["rest_small"] += 0 < rest < 256
        seen["rest_big"] += rest > chunk * scan_grid
        seen["nw16"] += nw == 16
        seen["pieces"] += pieces
        seen["agg"] += agg_mask != 1023
    assert all(v > 20 for v in seen.values()), seen  # every region the issue names is in the cases


def test_sparse_geometry_production_points(model):
    # n_cu = 256, options at their defaults, 8-wave workgroups: 512 workgroups of 2,048 tiles (kt 4); the flat 1 GiB stream
    # before its first retile (630 chunks) leaves 118 chunks behind the first round, cut into 472 pieces of 512 tiles
    assert c_geom(model, 630 * 2048, 256, 10 ** 6, False, 16, 0, 20, None, 1, 1) == (8, 2048, 4, 512, 118 * 2048, 1, 512, 472, 1023)
    # ... and with chunk_steal = 0 the same tiles go out as whole chunks by workgroup index
    assert c_geom(model, 630 * 2048, 256, 10 ** 6, False, 16, 0, 20, None, 0, 1) == (8, 2048, 4, 512, 118 * 2048, 0, 2048, 0, 1023)
    # a late merge (at most 20 sites per CU) on a stream that one round of 16-wave workgroups covers: 256 of them, kt <= 2,
    # and the small aggregator of a flat job (a full one once the batch limit is above 2)
    assert c_geom(model, 256 * 2048, 256, 5120, False, 2, 0, 20, None, 1, 1) == (16, 2048, 2, 256, 0, 0, 0, 0, 511)
    assert c_geom(model, 256 * 2048, 256, 5120, False, 16, 0, 20, None, 1, 1)[8] == 1023
    assert c_geom(model, 256 * 2048, 256, 5121, False, 2, 0, 20, None, 1, 1)[:4] == (8, 1024, 2, 512)
    assert c_geom(model, 256 * 2048 + 1, 256, 5120, False, 2, 0, 20, None, 1, 1)[0] == 8  # (more than one round of them: 8 waves)
    assert c_geom(model, 100_000, 256, 100, False, 2, 8, 20, None, 1, 1)[8] == 255 and c_geom(model, 100_000, 256, 100, True, 2, 8, 20, None, 1, 1)[8] == 1023


def test_streaming_grid(model):
    unset = model.rules_opt_unset()
    rng = random.Random(3)
    cases = [(n, cu, occ, ab) for n in (0, 1, 3, 4, 5, 4095, 4096, 4097, 1 << 20, M32 - 2) for cu in (1, 256) for occ in (1, 4, 8) for ab in (None, 0, 1, 7, 100000)]
    cases += [(rng.randrange(0, 1 << rng.randrange(1, 32)), rng.randrange(1, 400), rng.randrange(1, 9), rng.choice((None, rng.randrange(0, 20000)))) for _ in range(2000)]
    for n_tiles, n_cu, occ, ab in cases:
        want = ((n_tiles + WPB - 1) & M32) // WPB
        cap = (n_cu * occ if ab is None else ab) & M32
        assert model.rules_count_grid(n_tiles, n_cu, occ, unset if ab is None else ab) == max(1, min(want, cap, MAX_APPLY_BLOCKS)), (n_tiles, n_cu, occ, ab)
    assert model.rules_count_grid(630 * 2048, 256, 4, unset) == 1024  # four workgroups per CU


# ------------------------------------------------------------------------------------------------ form, upkeep
def test_form_switch(model):
    rng = random.Random(4)
    for _ in range(3000):
        n_tiles = rng.choice((0, 1, rng.randrange(0, 1 << 31)))
        merged, weighted = rng.random() < 0.8, rng.random() < 0.5
        sites = rng.choice((0, rng.randrange(0, 1 << 33)))
        best = rng.choice((rng.randrange(0, 1 << 40), n_tiles + rng.randrange(-2, 3) if n_tiles > 2 else 0))
        pct = rng.choice((100, 0, 1, 50, 400))
        cnt = sites if (weighted and sites) else best
        want = bool(n_tiles and merged and (cnt * 100) & M64 < n_tiles * pct)
        assert model.rules_want_sparse(n_tiles, merged, weighted, sites, best, pct) == want
    # split_pct 100: sparse once the last merge had fewer sites than there are tiles
    assert model.rules_want_sparse(1000, 1, 0, 0, 999, 100) == 1 and model.rules_want_sparse(1000, 1, 0, 0, 1000, 100) == 0
    assert model.rules_want_sparse(1000, 1, 1, 10, 10 ** 6, 100) == 1  # (pooled words: the resident sites count)
    assert model.rules_want_sparse(1000, 0, 0, 0, 0, 100) == 0  # (nothing merged yet: the best count is not known)
    for split, glob, want in [(-1, 0, 0), (-1, 1, 1), (0, 1, 0), (0, 0, 0), (1, 0, 1), (1, 1, 1), (2, 1, 0)]:
        assert model.rules_sparse_now(split, glob) == want


def test_candidate_list_upkeep(model):
    rng = random.Random(5)
    for _ in range(4000):
        use = rng.random() < 0.8
        i, built = rng.randrange(0, 100000), rng.randrange(0, 100000)
        if rng.random() < 0.6:
            built = max(0, i - rng.randrange(0, 600))
        every = rng.choice((512, 1, 0, -3, 100))
        T = rng.randrange(0, 1 << 30)
        best = T + rng.randrange(-5, 2000) if rng.random() < 0.7 else rng.randrange(0, 1 << 31)
        best = max(best, 0)
        prev = best + rng.choice((0, 0, rng.randrange(0, 500))) if rng.random() < 0.8 else rng.randrange(0, 1 << 31)
        n_all, target = rng.randrange(0, 3000), rng.choice((768, 0, 2000, 960))
        drop = prev - best if prev > best else 0
        near_T = best < (T + 2 * drop + 1) & M64
        long_list = n_all > max(4 * BLOCK - 64, target & M32)
        want = (not use) or ((i - built) & M32) >= (max(1, every) & M32) or i < built or near_T or long_list
        assert model.rules_cand_rebuild(use, i, built, every, best, T, prev, n_all, target) == want, (use, i, built, every, best, T, prev, n_all, target)
    # the list is kept while the maximum is clear of T by more than two rounds' drop, the list short and young
    assert model.rules_cand_rebuild(1, 600, 100, 512, 1000, 700, 1100, 500, 768) == 0
    assert model.rules_cand_rebuild(1, 612, 100, 512, 1000, 700, 1100, 500, 768) == 1  # 512 merges old
    assert model.rules_cand_rebuild(1, 600, 100, 512, 1000, 800, 1100, 500, 768) == 1  # 1000 < 800 + 2 * 100 + 1
    assert model.rules_cand_rebuild(1, 600, 100, 512, 1000, 700, 1100, 961, 768) == 1 and model.rules_cand_rebuild(1, 600, 100, 512, 1000, 700, 1100, 960, 768) == 0


def test_signature_upkeep(model):
    rng = random.Random(6)
    for _ in range(3000):
        valid = rng.random() < 0.8
        i, built = rng.randrange(0, 100000), rng.randrange(0, 100000)
        every = rng.choice((16384, 1, 0, 100))
        at_build = rng.randrange(0, 1 << 34)
        now = rng.choice((at_build, max(0, at_build - at_build * rng.randrange(0, 40) // 100 + rng.randrange(-2, 3)), rng.randrange(0, 1 << 34)))
        pct = rng.choice((20, 0, 5, 100))
        since = at_build - now if at_build > now else 0
        want = (not valid) or ((i - built) & M32) >= max(1, every) or i < built or since * 100 > at_build * pct
        assert model.rules_sig_rebuild(valid, i, built, every, at_build, now, pct) == want
    assert model.rules_sig_rebuild(1, 100, 0, 16384, 1000, 800, 20) == 0 and model.rules_sig_rebuild(1, 100, 0, 16384, 1000, 799, 20) == 1  # a fifth merged away


# ------------------------------------------------------------------------------------------------ exchange, rounds, housekeeping
def py_xeff(xseen, xcap, headroom, margin, granule, floor):
    recent = max(xseen)
    gran = max(1, granule)
    raw = recent * max(1, headroom) // 100 + max(0, margin)
    want = (raw + gran - 1) // gran * gran
    return min(xcap, max(want, min(max(1, floor), xcap)))


def test_exchange_sizing(model):
    rng = random.Random(7)
    cases = [([0, 0, 0, 0], xcap, 200, 1024, 1024, 2048) for xcap in (1, 100, 2047, 2048, 2049, 65536)]  # nothing seen; xcap below and above delta_floor
    for _ in range(3000):
        top = 1 << rng.randrange(1, 24)
        cases.append(([rng.choice((0, rng.randrange(0, top))) for _ in range(4)], rng.choice((rng.randrange(1, 4096), rng.randrange(1, 1 << 22))),
                      rng.choice((200, 100, 0, 150, 400)), rng.choice((1024, 0, -5, 100)), rng.choice((1024, 1, 0, 64)), rng.choice((2048, 0, 1, 100000))))
    for xseen, xcap, headroom, margin, granule, floor in cases:
        got = model.rules_xeff_next((U32 * 4)(*xseen), xcap, headroom, margin, granule, floor)
        assert got == py_xeff(xseen, xcap, headroom, margin, granule, floor), (xseen, xcap, headroom, margin, granule, floor)
        assert 1 <= got <= xcap
    # defaults: twice the largest of the last four rounds plus 1,024, in granules of 1,024, never below 2,048 records
    assert model.rules_xeff_next((U32 * 4)(0, 0, 0, 0), 65536, 200, 1024, 1024, 2048) == 2048
    assert model.rules_xeff_next((U32 * 4)(10, 3000, 20, 0), 65536, 200, 1024, 1024, 2048) == 7168
    assert model.rules_xeff_next((U32 * 4)(10, 300000, 20, 0), 65536, 200, 1024, 1024, 2048) == 65536
    for _ in range(500):
        xcap = rng.randrange(1, 1 << 31)
        xeff = rng.randrange(1, xcap + 1)
        assert model.rules_xeff_after_full(xeff, xcap) == min(xcap, 4 * xeff)
    assert model.rules_xeff_after_full(2048, 65536) == 8192 and model.rules_xeff_after_full(1 << 30, M32) == M32  # (no 32-bit wrap)


def test_round_sizing(model):
    rng = random.Random(8)
    for first in (0, 1):
        for sparse in (0, 1):
            for check in (1, 7, 8, 9, 32, 1000):
                assert model.rules_round_launches(first, sparse, check) == (min(check, 8) if first and not sparse else check)
    for bm in (-1, 0, 1, 2, 15, 16, 17, 1000):
        assert model.rules_round_kmax(1, bm) == max(1, min(KMAX, bm)) and model.rules_round_kmax(0, bm) == 1
    for _ in range(2000):
        nm, i, nl, k = rng.randrange(0, M32), rng.randrange(0, M32), rng.randrange(1, 5000), rng.randrange(1, 17)
        assert model.rules_round_records(nm, i, nl, k) == min(nm, i + (nl + 2) * k)
        assert model.rules_rec_first(nm) == min(nm, YB_MAX_TOKENS + 4096)
        t0, la = rng.randrange(0, 70000), rng.randrange(0, 5000)
        assert model.rules_tok_upper(t0, la, k) == t0 + (la + 1) * k + 1
        cap = 1 << rng.randrange(0, 34)
        assert model.rules_partials(cap) == min(1024, max(1, cap // (BLOCK * 8)))
    assert model.rules_round_records(50000, 0, 8, 1) == 10 and model.rules_round_records(50000, 1000, 32, 16) == 1000 + 34 * 16
    assert model.rules_rec_first(1 << 20) == 0xFFFE + 4096 and model.rules_partials(1 << 16) == 32


def test_table_and_stream_housekeeping(model):
    rng = random.Random(9)
    for _ in range(3000):
        cap = 1 << rng.randrange(10, 32)
        pct = rng.choice((30, 0, 50, 100))
        entries = rng.choice((rng.randrange(0, cap + 1), cap * pct // 100 + rng.randrange(-1, 2)))
        entries = max(entries, 0)
        assert model.rules_table_grow(entries, cap, pct) == (entries * 100 > cap * pct)
        gx, floor = rng.choice((8, 4, 2, 1, 0, -7)), rng.choice((1 << 16, 1024))
        assert model.rules_table_grow_target(entries, gx, floor) == max(entries * max(2, gx), floor)
        n_tiles = rng.randrange(0, 1 << 24)
        min_tiles = rng.choice((4096, 2, 0, 1 << 20))
        rpct, span = rng.choice((60, 0, 100, 33)), rng.choice((961, 449, 1))
        live = rng.choice((rng.randrange(0, n_tiles * span + 1), int(rpct / 100.0 * n_tiles * span) + rng.randrange(-1, 2)))
        live = max(live, 0)
        want = n_tiles >= min_tiles and float(live) < (float(rpct) / 100.0) * float(n_tiles) * span
        assert model.rules_retile(n_tiles, min_tiles, live, rpct, span) == want
    # 30 % load grows the table eightfold over its entries (a load of 12.5 %), never to fewer than 2^16 slots
    assert model.rules_table_grow(300, 1000, 30) == 0 and model.rules_table_grow(301, 1000, 30) == 1
    assert model.rules_table_grow_target(1 << 20, 8, 1 << 16) == 1 << 23 and model.rules_table_grow_target(100, 8, 1 << 16) == 1 << 16
    assert model.rules_table_grow_target(1000, 4, 1024) == 4000  # (the u32 loop's target)
    assert model.rules_retile(4096, 4096, 4096 * 961 * 6 // 10 - 1, 60, 961) == 1 and model.rules_retile(4095, 4096, 0, 60, 961) == 0
