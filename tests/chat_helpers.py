"""What the conversation tests share: the tokenizer (the corpus.en model with the ChatML specials), one hand-written
conversation as ids, and the max_length cases that the CPU file spells out and the GPU file runs again."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests import mask_helpers as mh

ROLES = ["system", "user", "assistant", "user", "assistant"]
CONTENTS = [[11, 12, 13], [21, 22], [31, 32, 33], [41], []]  # the last turn: an empty content


@lru_cache(maxsize=None)
def tokenizer():
    return mh.tokenizer(specials=("<|im_start|>", "<|im_end|>", "[PAD]"))


@lru_cache(maxsize=None)
def bodies() -> tuple:
    """body_t = H + content + F of the hand-written conversation, from the pieces encoded one by one"""
    tok = tokenizer()
    return tuple(tuple(tok.encode(f"<|im_start|>{r}\n") + c + tok.encode("<|im_end|>\n")) for r, c in zip(ROLES, CONTENTS))


def cut_cases() -> dict:
    """name -> (keyword arguments, the turns that stay, the ids the bodies keep in all, (q, k))"""
    b = [len(x) for x in bodies()]
    head, total = b[0] - 3 - 2, sum(b)  # (the system header; its content has 3 ids, the footer 2)
    right, drop = {"truncation": "right"}, {"truncation": "drop_oldest"}
    return {
        "right-in-header": ({**right, "max_length": head - 1}, [0], head - 1, (0, 0)),
        "right-in-content": ({**right, "max_length": head + 2}, [0], head + 2, (0, 0)),
        "right-in-footer": ({**right, "max_length": head + 4}, [0], head + 4, (0, 0)),
        "right-second-turn": ({**right, "max_length": b[0] + 1}, [0, 1], b[0] + 1, (0, 0)),
        "drop-all-fit": ({**drop, "max_length": total}, [0, 1, 2, 3, 4], total, (1, 1)),
        "drop-middle-k": ({**drop, "max_length": b[0] + b[3] + b[4] + 1}, [0, 3, 4], b[0] + b[3] + b[4], (1, 3)),
        "drop-nothing-fits": ({**drop, "max_length": b[0] + b[4] - 1}, [0, 4], b[0] + b[4] - 1, (1, 4)),
        "drop-unpinned": ({**drop, "pin_first": False, "max_length": b[3] + b[4]}, [3, 4], b[3] + b[4], (0, 3)),
        "drop-pin-other-role": ({**drop, "pin_roles": ("user",), "max_length": b[4]}, [4], b[4], (0, 4)),
        "drop-last-cut": ({**drop, "pin_first": False, "max_length": 2}, [4], 2, (0, 4)),
    }


def flat(contents, sizes):
    """-> (ids u32, doc_off u64[n_turns + 1], conv_off u64[n_convs + 1]) as chat_array takes them"""
    off = np.concatenate(([0], np.cumsum([len(c) for c in contents], dtype=np.int64))).astype(np.uint64)
    return mh.flat(contents, np.uint32), off, np.concatenate(([0], np.cumsum(sizes, dtype=np.int64))).astype(np.uint64)


def as_lists(got):
    ids, labels, off, info = got
    assert (ids.dtype, labels.dtype, off.dtype, info.dtype) == (np.uint32, np.int32, np.uint64, np.uint32)
    assert off[0] == 0 and off[-1] == len(ids) == len(labels) and info.shape == (len(off) - 1, 4)
    o = off.tolist()
    rag = lambda a: [a[o[d]:o[d + 1]].tolist() for d in range(len(o) - 1)]  # noqa: E731
    return rag(ids), rag(labels), [tuple(r) for r in info.tolist()]
