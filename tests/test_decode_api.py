"""CPU: the device decoder's entry points fail loudly without a GPU (no CPU fallback), the plain decode / decode_batch keep
working next to them, and list ids that no device vocab can hold are dropped on the host before upload."""
from __future__ import annotations

import numpy as np
import pytest

from yet_another_bpe import _native
from yet_another_bpe import tokenizer as tokmod
from yet_another_bpe.tokenizer import BBPETokenizer


def _tok() -> BBPETokenizer:
    vocab = {bytes([i]): i for i in range(256)}
    vocab[b"ab"] = 256
    vocab[b"<s>"] = 257
    return BBPETokenizer(vocab=vocab, merges=[(b"a", b"b")], special_tokens=["<s>"])


def test_device_methods_need_a_gpu():
    if _native.lib().yabpe_device_count() > 0:
        pytest.skip("a GPU is present; the no-device error path is checked on CPU-only hosts")
    tok = _tok()
    for call in (lambda: tok.decode_array(np.asarray([256, 257], np.uint32)), lambda: tok.decode_array([256], [0, 1]),
                 lambda: tok.decode_batch_device([[256], [257]])):
        with pytest.raises(_native.YabpeError) as e:
            call()
        assert e.value.code == -2
    assert tok.decode([256, 257, 999]) == "ab<s>"
    assert tok.decode_batch([[256], [], [0xC3]]) == ["ab", "", "�"]
    assert tok.encode("ab<s>") == [256, 257]


def test_decode_symbols_are_bound():
    for name in ("yabpe_decode_set_model", "yabpe_decode", "yabpe_decode_free", "yabpe_decode_stats"):
        assert name in _native.SYMBOLS
        assert getattr(_native.lib(), name).argtypes is not None


def test_out_of_range_list_ids_are_dropped():
    ids = [5, -1, 1 << 32, (1 << 32) - 1, 1 << 70, 0, -(1 << 80), 7]
    assert tokmod._u32_ids(ids).tolist() == [5, (1 << 32) - 1, 0, 7]
    assert tokmod._u32_mask(ids).tolist() == [True, False, False, True, False, True, False, True]
    assert tokmod._u32_ids(np.asarray([3, -2, 1 << 40], np.int64)).tolist() == [3]
    assert tokmod._u32_ids([]).tolist() == []
    # the plain decode skips them too: the ids are not in any vocab
    tok = _tok()
    assert tok.decode(ids) == tok.decode([5, 0, 7])


def test_model_arrays_keep_dict_order():
    a = _native.decode_model_arrays({b"a": 3, b"": 1, b"bc": 3})
    assert a["vb"].tobytes() == b"abc" and a["vo"].tolist() == [0, 1, 1, 3] and a["vi"].tolist() == [3, 1, 3]
    with pytest.raises(_native.YabpeError):
        _native.decode_model_arrays({b"a": 1 << 32})


def test_doc_off_is_checked_before_the_device():
    tok = _tok()
    for off in ([0], [1, 2], [0, 1], [0, 2, 1, 2]):
        with pytest.raises(ValueError):
            tok.decode_array([1, 2], off)
    assert tok.decode_batch_device([]) == []
