"""GPU: every device buffer of the host drivers is traced and released.  A fresh child process runs pretokenize, load_words
with pooling, a resumed load, encode, encode_spans and decode -- good inputs and malformed ones -- under YABPE_TRACE_ALLOC=1
at the smallest sizes that reach the two-level prefix sum (SCAN_TILE + 1 = 2,049 items); the parent walks the trace: every
allocation is freed before its address comes back or the process ends, and the buffers of the pre-tokeniser, of the pooling
of equal words and of the scan are among the traced ones."""
from __future__ import annotations

import json
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import pretok
from tests import helpers

pytestmark = pytest.mark.gpu

SP = "<|endoftext|>"
TEXT = b"ab " * 2731 + SP.encode() + b" ab" * 2731  # 16 KiB: 9 count / scatter workgroups, some 5,460 pre-tokens
BAD_AT = 9001
BROKEN = TEXT[:BAD_AT] + b"\xff" + TEXT[BAD_AT + 1:]
WORDS = [b"w%d" % (i % 700) for i in range(2100)]  # 2,100 words, 700 distinct
SCAN_TILE = 2048


def mark(name):
    print(f"[mark] {name}", file=sys.stderr, flush=True)


def child():
    """Runs in the child process; the results the parent checks leave as one JSON line on stdout."""
    from yet_another_bpe import _native
    from yet_another_bpe.trainer import BBPETrainer

    res = {}
    base = helpers.base_tokens([SP])
    flat, off = helpers.flatten(WORDS)
    vocab = {bytes([i]): i for i in range(256)}
    vocab[b"ab"] = 256
    vocab[SP.encode()] = 257
    ctx = _native.Context()
    mark("pretokenize")
    _dt, _do, res["n_pre"] = ctx.pretokenize(TEXT, special_tokens=[SP])
    mark("pretokenize_broken")
    try:
        ctx.pretokenize(BROKEN, special_tokens=[SP])
    except Exception as e:  # noqa: BLE001 (the parent checks the type)
        res["pretok_err"] = [type(e).__name__, getattr(e, "position", None)]
    mark("load_words")
    ctx.set_vocab(base)
    ctx.load_words(flat, off, dedup=True)
    left, right, merged, _count = ctx.train(10, 1)
    _v, merges = BBPETrainer._decode_merges(base, left, right, merged)
    res["n_merges"] = len(merges)
    mark("load_words_resumed")
    toks, triples = _native.merge_triples(base, merges)
    with _native.Context() as ctx2:
        ctx2.set_vocab(toks)
        ctx2.load_words_resumed(flat, off, None, triples, dedup=True)
        res["resumed_unique"] = ctx2.resume_stats()["n_unique"]
    mark("encode")
    ctx.encode_set_model(vocab, [(b"a", b"b")], [SP], 0)
    ids, _doc = ctx.encode_to_host(TEXT)
    res["n_ids"] = int(ids.size)
    mark("encode_spans")
    ids2, _doc, spans = ctx.encode_spans_to_host(TEXT, chars=True)
    res["spans_ok"] = bool(np.array_equal(ids, ids2) and len(spans) == len(ids))
    mark("encode_broken")
    try:
        ctx.encode(BROKEN)
    except Exception as e:  # noqa: BLE001
        res["encode_err"] = [type(e).__name__, getattr(e, "position", None)]
    mark("decode")
    ctx.decode_set_model(vocab)
    ids = ids.copy()
    ids[100] = 255  # the byte 0xFF: the text needs a U+FFFD
    text, _toff = ctx.decode_to_host(ids)
    res["n_replacements"] = ctx.decode_stats()["n_replacements"]
    res["decoded_ok"] = text.tobytes().decode("utf-8").count("�") == 1
    mark("close")
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


ALLOC = re.compile(r"^\[yabpe alloc r(-?\d+)\] (0x[0-9a-f]+) \.\. 0x[0-9a-f]+  (\d+) B")
FREE = re.compile(r"^\[yabpe free\] (0x[0-9a-f]+)")


def test_every_traced_buffer_is_released():
    import os

    repo = helpers.GOLDEN.parent.parent
    code = (
        "import sys\n"
        f"sys.path[:0] = [{str(repo)!r}, {str(repo / 'yet-another-bpe_amd')!r}]\n"
        "from tests.test_gpu_scratch_balance import child\n"
        "child()\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, YABPE_TRACE_ALLOC="1"))
    assert out.returncode == 0, out.stderr[-2000:]  # (a)
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    # (b) the malformed byte is reported as the other GPU tests expect it: Utf8Error at UnicodeDecodeError.start
    with pytest.raises(UnicodeDecodeError) as e:
        BROKEN.decode("utf-8")
    assert e.value.start == BAD_AT
    assert res["pretok_err"] == ["Utf8Error", BAD_AT] and res["encode_err"] == ["Utf8Error", BAD_AT]
    n_pre = res["n_pre"]
    assert n_pre == len(pretok.pretokenize(TEXT, [SP])) and n_pre > SCAN_TILE and len(WORDS) > SCAN_TILE and len(TEXT) > SCAN_TILE
    assert res["n_merges"] == 10 and res["resumed_unique"] == 700
    assert res["n_ids"] > SCAN_TILE and res["spans_ok"] and res["n_replacements"] == 1 and res["decoded_ok"]
    # (c) walk the trace in order
    live, section, sizes = {}, "start", {}
    for ln in out.stderr.splitlines():
        if ln.startswith("[mark] "):
            section = ln[len("[mark] "):]
        elif (m := ALLOC.match(ln)):
            assert m.group(2) not in live, f"{m.group(2)} handed out again in {section}; still held since {live[m.group(2)]}"
            live[m.group(2)] = section
            sizes.setdefault(section, []).append(int(m.group(3)))
        elif (m := FREE.match(ln)):
            live.pop(m.group(1), None)  # (buffers of plain hipMalloc are freed here too: not in the trace)
    assert not live, f"never freed: {live}"
    # (d) the drivers' own buffers are in the trace
    n, pt, ld = len(TEXT), sizes["pretokenize"], sizes["load_words"]
    assert len(pt) + len(ld) >= 17, (len(pt), len(ld))
    nb = (n + SCAN_TILE - 1) // SCAN_TILE  # count / scatter workgroups (PT_PER_BLOCK is 2,048 bytes too)
    for want in (n, n + 8, nb * 8, (nb + 1) * 8, (n_pre + 1) * 8):  # meta, flags, block counts, their scan, the offsets
        assert want in pt, (want, pt)
    nw = len(WORDS)
    assert ld.count(nw * 8) >= 2 and ld.count((nw + 1) * 8) >= 2 and ld.count(nw * 4) >= 3, ld  # hash, count; the scans; rep, flag, ulen
    scan_blocks = (nw + 1 + SCAN_TILE - 1) // SCAN_TILE
    assert scan_blocks == 2 and ld.count(scan_blocks * 8) >= 4, ld  # two two-level scans, block sums and their scan each
    assert sizes["encode"].count(((n_pre + 1 + SCAN_TILE - 1) // SCAN_TILE) * 8) >= 4, sizes["encode"]
