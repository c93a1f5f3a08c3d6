"""GPU: the start tables that yabpe_pretokenize ("chunk") and the three text passes yabpe_normalize, yabpe_utf8_repair and
yabpe_lowercase ("part") refuse -- one check for all four (csrc/yabpe.hip: offset_table).  Every call here is refused on the
host before anything is launched; a refused call frees nothing and resets nothing, so the results and the stats of the pass's
call before it are still there, and the call after it works."""
from __future__ import annotations

import numpy as np
import pytest

from yet_another_bpe import _native

pytestmark = pytest.mark.gpu

E_INVALID = -1
TEXT = b"Abc dEf!"
OTHER = b"ZYXWVUTS"  # what a pass that runs in between writes: into a block of the same size, were one free
ASCEND, FIRST = "{} offsets must ascend inside the text", "the first {} must start at 0"
TABLES = [([1, 2], FIRST), ([0, 5, 3], ASCEND), ([0, 9], ASCEND)]
# pass -> (its word in the messages, the text it gives for TEXT, a pass to run in between)
PASSES = {"pretokenize": ("chunk", TEXT, "utf8_repair"), "normalize": ("part", TEXT, "utf8_repair"), "utf8_repair": ("part", TEXT, "normalize"),
          "lowercase": ("part", TEXT.lower(), "normalize")}


@pytest.fixture(scope="module")
def ctx():
    with _native.Context(0) as c:
        yield c


def call(ctx, name, text, starts=None):
    """-> (device text, device offsets, number of offsets - 1)"""
    if name == "pretokenize":
        return ctx.pretokenize(text, chunk_starts=starts)
    dt, do, _nb = getattr(ctx, name)(text, part_starts=starts)
    return dt, do, len(starts) if starts is not None else 1


def read(ctx, dt, do, n):
    return ctx.d2h(dt, len(TEXT)).tobytes(), ctx.d2h(do, 8 * (n + 1), np.uint64).tolist()


@pytest.mark.parametrize("name", list(PASSES))
def test_refused_start_tables(ctx, name):
    what, out, between = PASSES[name]
    before = call(ctx, name, TEXT, [0, 4])
    expect = read(ctx, *before)
    assert expect[0] == out and (expect[1] == [0, 4, 8] if name != "pretokenize" else expect[1][0] == 0 and expect[1][-1] == 8)
    stats = getattr(ctx, name + "_stats")() if name != "pretokenize" else None
    for starts, message in TABLES:
        with pytest.raises(_native.YabpeError) as e:
            call(ctx, name, TEXT, starts)
        assert e.value.code == E_INVALID and str(e.value) == f"yabpe error {E_INVALID}: {message.format(what)}", starts
    assert stats is None or getattr(ctx, name + "_stats")() == stats  # (not reset either)
    call(ctx, between, OTHER)
    assert read(ctx, *before) == expect  # the refused calls freed nothing
    after = call(ctx, name, TEXT, [0, 2, 5])
    got = read(ctx, *after)
    assert got[0] == out and (got[1] == [0, 2, 5, 8] if name != "pretokenize" else got[1][-1] == 8)


def test_the_pass_checks_its_own_argument_first(ctx):
    for starts, _message in TABLES:
        with pytest.raises(_native.YabpeError) as e:
            ctx.normalize(TEXT, part_starts=starts, form=2)
        assert e.value.code == E_INVALID and str(e.value) == f"yabpe error {E_INVALID}: normalisation form 2: only YABPE_NORM_NFC (1) is there"
        with pytest.raises(_native.YabpeError) as e:
            ctx.utf8_repair(TEXT, part_starts=starts, mode=3)
        assert e.value.code == E_INVALID and str(e.value) == f"yabpe error {E_INVALID}: utf8 mode 3: YABPE_UTF8_REPLACE (1) or YABPE_UTF8_IGNORE (2)"
