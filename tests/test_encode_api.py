"""CPU: the device encoder's entry points fail loudly without a GPU (no CPU fallback), and the plain tokenizer methods
keep working next to them."""
from __future__ import annotations

import pytest

from yet_another_bpe import _native
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
    for call in (lambda: tok.encode_array(["ab<s>"]), lambda: tok.encode_array(b"ab"), lambda: tok.encode_batch_device(["ab"])):
        with pytest.raises(_native.YabpeError) as e:
            call()
        assert e.value.code == -2
    assert tok.encode("ab ab<s>") == [256, 32, 256, 257]
    assert tok.encode_batch(["ab", ""]) == [[256], []]
    assert tok.decode([256, 257]) == "ab<s>"
    assert "misses=" in tok.cache_info()


def test_model_arrays_layout():
    a = _native.encode_model_arrays({b"a": 0, b"bc": 1}, [(b"b", b"c"), (b"", b"a")], ["<s>", "x"])
    assert a["vb"].tobytes() == b"abc" and a["vo"].tolist() == [0, 1, 3] and a["vi"].tolist() == [0, 1]
    assert a["mb"].tobytes() == b"bca" and a["mo"].tolist() == [0, 1, 2, 2, 3]
    assert a["sb"].tobytes() == b"<s>x" and a["so"].tolist() == [0, 3, 4]
