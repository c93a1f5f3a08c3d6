"""GPU: yabpe_chat bit for bit against the plain-Python BBPETokenizer.chat_tokens, and encode_array_chat against
encode_batch_chat, over the flags and the smallest inputs at which the kernels can go wrong: an output that crosses CHAT_TILE
boundaries inside a footer, a content and a header; one tile covered by more than CHAT_STAGE one-id, empty and dropped turns;
conversations of 0, 1 and 2 turns side by side; batches without any turn; the max_length cases of the CPU file; inputs as
host arrays and as the encoder's device results; and every refused argument, each leaving the previous results valid."""
from __future__ import annotations

import numpy as np
import pytest

from tests import chat_helpers as ch
from yet_another_bpe import _native
from yet_another_bpe.tokenizer import ChatTemplate

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
BARE = ChatTemplate({"user": ("", ""), "assistant": ("", "")})  # no header, no footer: a turn is its content
FULL = ChatTemplate({r: (f"<|im_start|>{r}\n", "<|im_end|>\n") for r in ("system", "user", "assistant")}, prefix="<|im_end|>[PAD]")


@pytest.fixture(scope="module")
def tok():
    return ch.tokenizer()


def shapes(tok) -> dict:
    """name -> (template, content lengths, roles, turns per conversation)"""
    T = _native.CHAT_TILE
    h = {r: len(tok.encode(f"<|im_start|>{r}\n")) for r in ("user", "assistant")}
    c0 = T - 1 - h["user"]                 # the footer of turn 0 covers slots T - 1 and T
    c1 = 3 * T - 1 - (T + 1) - h["assistant"] - 2  # the content of turn 1 crosses 2 T, its body ends at 3 T - 1: turn 2's header crosses 3 T
    many = [0 if t % 3 == 1 or t in (255, 256, 257, 511, 512) else 1 for t in range(3 * _native.CHAT_STAGE)]
    return {
        "tile-straddle": (tok.CHATML, [c0, c1, 5], ["user", "assistant", "user"], [3]),
        "stage-rounds": (BARE, many + [3, 2], ["user", "assistant"] * (len(many) // 2 + 1), [len(many), 2]),
        "sizes-0-1-2": (FULL, [4, 0, 7, 2, 1], ["user", "system", "assistant", "assistant", "user"], [0, 1, 2, 0, 0, 2, 0]),
        "no-turns": (FULL, [], [], [0, 0, 0]),
        "no-turns-no-ids": (tok.CHATML, [], [], [0, 0]),
    }


FLAGS = {
    "default": {},
    "all-gen": {"loss": "all", "add_generation_prompt": True},
    "last-right": {"loss": "last", "truncation": "right", "max_length": 40},
    "drop-120": {"max_length": 120, "train_roles": ("assistant", "user")},
    "drop-unpinned-gen": {"max_length": 25, "pin_first": False, "add_generation_prompt": True},
}


def run(tok, template, lens, roles, sizes, kw, seed=1):
    rng = np.random.default_rng(seed)
    contents = [rng.integers(0, 1000, n).tolist() for n in lens]
    exp = tok.chat_tokens(contents, roles, sizes, template=template, **kw)
    got = tok.chat_array(*ch.flat(contents, sizes), roles, template=template, **kw)
    assert ch.as_lists(got) == tuple(exp)
    return exp


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("shape", ["tile-straddle", "stage-rounds", "sizes-0-1-2", "no-turns", "no-turns-no-ids"])
def test_matches_plain_python(tok, shape, flags):
    template, lens, roles, sizes = shapes(tok)[shape]
    seqs, labels, info = run(tok, template, lens, roles, sizes, FLAGS[flags])
    st = tok._device().chat_stats()
    assert (st["n_convs"], st["n_turns"], st["n_out"]) == (len(sizes), len(lens), sum(len(s) for s in seqs))
    assert st["n_turns_dropped"] == sum(i[1] - i[0] for i in info) and st["n_labelled"] == sum(i[3] for i in info)
    assert st["n_convs_unlabelled"] == sum(i[3] == 0 for i in info)
    if shape == "tile-straddle" and flags == "default":  # the shape is what it claims to be
        assert len(seqs[0]) > 3 * _native.CHAT_TILE and labels[0][_native.CHAT_TILE - 1:_native.CHAT_TILE + 1] == [-100, -100]
    if shape == "stage-rounds" and flags == "drop-120":
        assert info[0][1] - info[0][0] > 2 * _native.CHAT_STAGE  # more dropped turns in a row than a stage holds


@pytest.mark.parametrize("name", list(ch.cut_cases()))
def test_the_cut_cases_of_the_cpu_file(tok, name):
    kw, _turns, kept, qk = ch.cut_cases()[name]
    got = tok.chat_array(*ch.flat(ch.CONTENTS * 2, [5, 5]), ch.ROLES * 2, **kw)
    assert ch.as_lists(got) == tuple(tok.chat_tokens(ch.CONTENTS * 2, ch.ROLES * 2, [5, 5], **kw))
    assert [tuple(r[:3]) for r in got[3].tolist()] == [qk + (kept,)] * 2


CONVS = [[("system", "You are terse."), ("user", "Hello there, General Kenobi!"), ("assistant", "Hello."), ("user", "12345 naïve<|im_end|>"),
          ("assistant", "")], [], [{"role": "assistant", "content": "It's the end."}], [("user", "")]]


@pytest.mark.parametrize("kw", [{}, {"max_length": 24, "bos_id": 1, "eos_id": 2, "padding_side": "left"},
                                {"max_length": 12, "truncation": "right", "add_generation_prompt": True, "loss": "all"}, {"template": FULL}])
def test_rows_from_text_match_plain_python(tok, kw):
    rows, labels, lengths, info = tok.encode_array_chat(CONVS, **kw)  # (yabpe_chat reads the encoder's device results)
    exp = tok.encode_batch_chat(CONVS, **kw)
    assert (rows.tolist(), labels.tolist(), lengths.tolist(), [tuple(r) for r in info.tolist()]) == exp
    assert tok.encode_array_chat([[], []])[0].shape == (2, 0) and tok.encode_array_chat([])[0].shape == (0, 0)


def test_device_inputs_and_results_that_outlive_later_calls(tok):
    ids, off, coff = ch.flat(ch.CONTENTS, [5])
    roles = np.asarray([0, 1, 2, 1, 2], np.uint8)
    ctx = tok._device()
    A = tok._chat_native_args(tok._chat_args(tok.CHATML, ("assistant",), "roles", None, "right", True, None, False))
    first = ctx.chat_to_host(ids, None, off[:-1], None, coff[:-1], None, roles, **A)
    blob = np.concatenate((ids, np.zeros(len(ids) % 2, np.uint32), off[:-1].view(np.uint32), coff[:-1].view(np.uint32)))
    d_ids = ctx.mask(blob, None, None, None, None, select=0)[0]  # (a mask that selects nothing copies the blob to the device)
    d_off = d_ids + 4 * (len(ids) + len(ids) % 2)
    di, dl, do, dn, n_out, nc = ctx.chat(d_ids, len(ids), d_off, 5, d_off + 8 * 5, 1, roles, **A)
    read = lambda: (ctx.d2h(di, 4 * n_out, np.uint32), ctx.d2h(dl, 4 * n_out, np.uint32).view(np.int32), ctx.d2h(do, 16, np.uint64),  # noqa: E731
                    ctx.d2h(dn, 16, np.uint32).reshape(1, 4))
    assert all(np.array_equal(a, b) for a, b in zip(first, read()))
    tok.encode_array_padded(["some text", "more"], 8)
    tok.fim_array(ids, [0, len(ids)], pre=1, suf=2, mid=3)
    assert all(np.array_equal(a, b) for a, b in zip(first, read()))  # later calls leave the results valid
    ctx.chat_free()
    ctx.chat_free()


def test_refused_arguments(tok):
    ids, off, coff = ch.flat(ch.CONTENTS, [5])
    roles = np.asarray([0, 1, 2, 1, 2], np.uint8)
    ctx = tok._device()
    ok = {"heads": [[5, 6], [7], [8, 9]], "feet": [[1], [1], [1, 2]], "prefix": [3], "train_mask": 4, "gen_role": 2}
    di, dl, do, dn, n_out, _ = ctx.chat(ids, None, off[:-1], None, coff[:-1], None, roles, **ok)
    good = ctx.d2h(di, 4 * n_out, np.uint32)
    stats = ctx.chat_stats()
    args = (ids, off[:-1], coff[:-1], roles)
    bad_roles, late, two = np.asarray([0, 1, 3, 1, 2], np.uint8), off[:-1].copy(), np.asarray([0, 6], np.uint64)
    late[2] = 99
    cases = [({"flags": 0x20}, args), ({"loss_all": True, "loss_last": True}, args), ({"gen_role": 3}, args), ({"max_len": 3}, args),
             ({"n_roles": 0}, args), ({"n_roles": 17}, args), ({}, (ids, off[:-1], coff[:-1], bad_roles)), ({}, (ids, late, coff[:-1], roles)),
             ({}, (ids, off[:-1], two, roles)), ({}, (ids, off[:-1], np.asarray([1], np.uint64), roles)), ({}, (ids, off[:-1], [], roles))]
    for bad, (a, b, c, d) in cases:
        with pytest.raises(_native.YabpeError) as e:
            ctx.chat(a, None, b, None, c, None, d, **{**ok, **bad})
        assert e.value.code == E_INVALID, bad
        assert ctx.chat_stats() == stats and np.array_equal(ctx.d2h(di, 4 * n_out, np.uint32), good)  # nothing was freed
    wide = {**ok, "heads": [[5] * 1000, [7] * 1000, [8]], "feet": [[1], [1], [1] * 45]}  # 2,049 template ids with the prefix
    for bad, n_ids in ((wide, None), ({}, (1 << 36) + 1)):
        with pytest.raises(_native.YabpeError) as e:
            ctx.chat(ids if n_ids is None else ids.ctypes.data, n_ids, off[:-1], None, coff[:-1], None, roles, **{**ok, **bad})
        assert e.value.code == E_CAPACITY and ctx.chat_stats() == stats
    assert np.array_equal(ctx.d2h(di, 4 * n_out, np.uint32), good)
    for bad in ({"roles": ["user"] * 4}, {"roles": [0, 1, 2, 1, 9]}, {"conv_off": [0, 4]}, {"doc_off": off[:-1]}, {"loss": "x"}):
        a = {"ids": ids, "doc_off": off, "conv_off": coff, "roles": ch.ROLES, **bad}
        with pytest.raises(ValueError):
            tok.chat_array(a.pop("ids"), a.pop("doc_off"), a.pop("conv_off"), a.pop("roles"), **a)
