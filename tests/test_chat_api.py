"""CPU: the plain-Python conversation rule (BBPETokenizer.chat_tokens / encode_batch_chat) on hand-written conversations, with
the expected sequences and labels written out piece by piece: template rendering, labels on the content and footer of the
trainable turns only, loss "all" and "last", the generation prompt, no turns, an empty content, the right cut inside a header,
a content and a footer, drop_oldest with and without the pinned first turn, and every ValueError."""
from __future__ import annotations

import pytest

from tests import chat_helpers as ch
from yet_another_bpe.tokenizer import BBPETokenizer, ChatTemplate

I = BBPETokenizer.IGNORE_LABEL


@pytest.fixture(scope="module")
def tok():
    return ch.tokenizer()


@pytest.fixture(scope="module")
def pieces(tok):
    S, E = tok.encode("<|im_start|>")[0], tok.encode("<|im_end|>")[0]
    H = {r: [S] + tok.encode(f"{r}\n") for r in ("system", "user", "assistant", "tool")}  # a special in a header is a special
    F = [E] + tok.encode("\n")
    assert len(F) == 2 and S != E and all(len(h) >= 3 for h in H.values())
    return H, F


def one(tok, **kw):
    seqs, labels, info = tok.chat_tokens(ch.CONTENTS, ch.ROLES, [5], **kw)
    return seqs[0], labels[0], info[0]


def test_rendering_and_labels(tok, pieces):
    H, F = pieces
    seq, lab, info = one(tok)
    assert seq == (H["system"] + [11, 12, 13] + F + H["user"] + [21, 22] + F + H["assistant"] + [31, 32, 33] + F + H["user"] + [41] + F
                   + H["assistant"] + F)
    n_before = len(H["system"]) + 3 + 2 + len(H["user"]) + 2 + 2 + len(H["assistant"])
    assert lab == [I] * n_before + [31, 32, 33] + F + [I] * (len(H["user"]) + 1 + 2 + len(H["assistant"])) + F
    assert info == (1, 1, len(seq), 3 + 2 + 2)  # (the system turn is pinned; nothing is cut)
    assert one(tok, loss="all")[1] == seq
    assert one(tok, loss="last")[1] == [I] * (len(seq) - 2) + F
    assert one(tok, loss="last", train_roles=("user",))[1] == [I] * len(seq)  # the last turn is not a user's
    lab_user = one(tok, train_roles=["user", "system"])[1]
    assert lab_user[:len(H["system"]) + 5] == [I] * len(H["system"]) + [11, 12, 13] + F and lab_user[-2:] == [I, I]
    gen = one(tok, add_generation_prompt=True)
    assert gen[0] == seq + H["assistant"] and gen[1] == lab + [I] * len(H["assistant"]) and gen[2] == (1, 1, len(gen[0]), 7)


def test_no_turns_and_a_prefix(tok, pieces):
    H, F = pieces
    llama = ChatTemplate({r: (f"<|im_start|>{r}\n", "<|im_end|>\n") for r in ("user", "bot")}, prefix="<|im_end|>", generation_role="bot")
    bos = tok.encode("<|im_end|>")
    h_bot = tok.encode("<|im_start|>bot\n")
    seqs, labels, info = tok.chat_tokens([[7]], ["bot"], [0, 1, 0], template=llama, train_roles=("bot",), add_generation_prompt=True)
    assert seqs == [bos + h_bot, bos + h_bot + [7] + F + h_bot, bos + h_bot]
    assert labels == [[I] * len(seqs[0]), [I] * len(bos + h_bot) + [7] + F + [I] * len(h_bot), [I] * len(seqs[0])]
    assert info == [(0, 0, len(seqs[0]), 0), (0, 0, len(seqs[1]), 3), (0, 0, len(seqs[2]), 0)]
    assert tok.chat_tokens([], [], [0]) == ([[]], [[]], [(0, 0, 0, 0)])
    cut = tok.chat_tokens([[7]], ["bot"], [1], template=llama, train_roles=("bot",), add_generation_prompt=True, max_length=len(bos + h_bot) + 1)
    assert cut[0] == [bos + h_bot[:1] + h_bot]  # X and G survive, one id is left for the bodies


@pytest.mark.parametrize("name", list(ch.cut_cases()))
def test_the_cut(tok, name):
    kw, turns, kept, qk = ch.cut_cases()[name]
    seq, lab, info = one(tok, **kw)
    full_seq, full_lab, _ = one(tok)
    at = [sum(len(b) for b in ch.bodies()[:t]) for t in range(6)]
    exp_seq = [x for t in turns for x in full_seq[at[t]:at[t + 1]]][:kept]
    exp_lab = [x for t in turns for x in full_lab[at[t]:at[t + 1]]][:kept]
    assert seq == exp_seq and lab == exp_lab and len(seq) == kept <= kw["max_length"]
    assert info == qk + (kept, sum(x != I for x in exp_lab))


def test_rows(tok, pieces):
    H, F = pieces
    convs = [[("user", "Hello there"), ("assistant", "General")], [], [{"role": "assistant", "content": ""}]]
    rows, labels, lengths, info = tok.encode_batch_chat(convs, bos_id=1, pad_id=0)
    first = H["user"] + tok.encode("Hello there") + F + H["assistant"] + tok.encode("General") + F
    L = len(first) + 1
    assert rows == [[1] + first, [1] + [0] * (L - 1), [1] + H["assistant"] + F + [0] * (L - 1 - len(H["assistant"]) - 2)]
    n_gen = len(tok.encode("General"))
    assert labels[0] == [I] * (L - n_gen - 2) + tok.encode("General") + F and labels[1] == [I] * L
    assert lengths == [L, 1, 1 + len(H["assistant"]) + 2] and [i[3] for i in info] == [n_gen + 2, 0, 2]
    rows8, labels8, lengths8, info8 = tok.encode_batch_chat(convs, 8, bos_id=1, pad_id=0, truncation="right", padding_side="left")
    assert rows8[0] == ([1] + first)[:8] and rows8[1] == [0] * 7 + [1] and lengths8 == [8, 1, min(8, lengths[2])] and info8[0][2] == 7


@pytest.mark.parametrize("bad", [
    {"loss": "middle"}, {"truncation": "left"}, {"train_roles": ("bot",)}, {"pin_roles": "nobody"}, {"max_length": 0}, {"max_length": "9"},
    {"template": "chatml"}, {"template": ChatTemplate({})}, {"template": ChatTemplate({str(r): ("a", "b") for r in range(17)})},
    {"template": ChatTemplate({"user": ("x " * 3000, "")})}, {"template": ChatTemplate({"user": ("a", "b")})},
    {"template": ChatTemplate({"user": ("a", "b"), "assistant": ("hello", "")}, generation_role="bot"), "add_generation_prompt": True},
    {"add_generation_prompt": True, "max_length": 3}])
def test_refused_arguments(tok, bad):
    with pytest.raises(ValueError):
        tok.chat_tokens(ch.CONTENTS, ch.ROLES, [5], **bad)


def test_refused_turns(tok):
    with pytest.raises(ValueError, match="'wizard'"):
        tok.encode_batch_chat([[("wizard", "hi")]])
    with pytest.raises(ValueError, match="'wizard'"):
        tok.chat_tokens([[1]], ["wizard"], [1])
    for sizes in ([4], [6], [5, -1, 1]):
        with pytest.raises(ValueError):
            tok.chat_tokens(ch.CONTENTS, ch.ROLES, sizes)
    with pytest.raises(ValueError):
        tok.encode_batch_chat([[("user", b"bytes")]])
    with pytest.raises(ValueError):
        tok.encode_batch_chat([[("user", "hi")]], 3, bos_id=1, eos_id=2, add_generation_prompt=True)  # nothing is left for the bodies
