"""GPU: BBPETokenizer.encode_array_with_words (yabpe_encode_words) against the plain-Python encode_batch_with_words, and its
ids and document offsets against encode_array's: empty documents, a document of specials only, the special without an id, a
90-byte pre-token (the sequential path), a document of about 700 pre-tokens (more than a block), 300 short documents (many
documents in a block); under digit_group = 3, "cl100k", "o200k_base" and lowercase + "nfc"; a bytes buffer with
errors="replace"."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu


def compare(tok, docs):
    exp = tok.encode_batch_with_words(docs)
    ids, off, words, special = tok.encode_array_with_words(docs)
    assert (ids.dtype, off.dtype, words.dtype, special.dtype) == (np.uint32, np.uint64, np.uint32, np.bool_)
    assert len(off) == len(docs) + 1 and len(ids) == len(words) == len(special) == off[-1]
    assert off.tolist() == np.concatenate(([0], np.cumsum([len(e[0]) for e in exp]))).tolist()
    o = off.tolist()
    for d, (e_ids, e_words, e_special) in enumerate(exp):
        a, b = o[d], o[d + 1]
        assert ids[a:b].tolist() == e_ids, d
        assert words[a:b].tolist() == e_words, d
        assert special[a:b].tolist() == e_special, d
    plain_ids, plain_off = tok.encode_array(docs)
    assert np.array_equal(plain_ids, ids) and np.array_equal(plain_off, off)
    return exp


def test_matches_plain_python():
    tok = mh.tokenizer()
    docs = mh.word_docs()
    exp = compare(tok, docs)
    assert exp[0] == ([], [], []) and all(exp[2][2])  # an empty document; a document of specials only
    assert exp[4] == ([], [], []) and exp[3][1] != list(range(len(exp[3][1])))  # the special without an id alone, and its gaps
    assert max(exp[6][1]) >= 690  # more pre-tokens than a block has threads
    assert tok.encode_batch_device_with_words(docs) == [tuple(e) for e in exp]
    # the long path: all ids of the 90-byte pre-token have index 0
    assert exp[5][1][:2] == [0, 0] and exp[5][1].count(0) > 1


@pytest.mark.parametrize("options, specials, mask", mh.GPU_OPTIONS, ids=[str(sorted(o)) for o, _s, _m in mh.GPU_OPTIONS])
def test_under_the_tokenizer_options(options, specials, mask):
    tok = mh.tokenizer(specials, **options)
    docs = mh.word_docs(mask) + [t for _o, _s, t in mh.OPTION_TEXTS if "[MASK]" not in t or mask == "[MASK]"]
    compare(tok, docs)


def test_no_texts_only_empty_texts_and_a_bytes_buffer():
    tok = mh.tokenizer()
    ids, off, words, special = tok.encode_array_with_words([])
    assert (len(ids), off.tolist(), len(words), len(special)) == (0, [0], 0, 0) and special.dtype == np.bool_
    ids, off, words, special = tok.encode_array_with_words(["", ""])
    assert (len(ids), off.tolist(), len(words), len(special)) == (0, [0, 0, 0], 0, 0)
    data = "café [MASK] ".encode("utf-8")[:-1] + b"\xff\xf0\x9f tail" + mh.NO_ID.encode() + b" end\xc3"
    exp = tok.encode_with_words(data.decode("utf-8", "replace"))
    ids, off, words, special = tok.encode_array_with_words(data, errors="replace")
    assert (ids.tolist(), words.tolist(), special.tolist()) == exp and off.tolist() == [0, len(exp[0])]
    from yet_another_bpe import _native

    with pytest.raises(_native.Utf8Error):
        tok.encode_array_with_words(data)


def test_a_later_plain_encode_gives_the_same_ids():
    """the words call leaves nothing behind that changes yabpe_encode, and the other way round"""
    tok = mh.tokenizer()
    docs = mh.word_docs()[:12]
    a = tok.encode_array(docs)
    w = tok.encode_array_with_words(docs)
    b = tok.encode_array(docs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], w[0])
