"""GPU: yabpe_fim_cuts against the plain-Python BBPETokenizer.fim_cuts and the byte starts computed in Python, on the texts
of tests/fim_helpers.py -- ASCII and 2-, 3- and 4-byte characters, documents of 63 to 129 bytes, a 4-byte character over a
64-byte granule seam, empty documents; each as a single document and as neighbours in one buffer -- with the text on the host
and in device memory, and a bytes buffer as one document."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fim_helpers as fh
from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


@pytest.mark.parametrize("batch", range(len(fh.CUT_BATCHES)))
def test_cuts_and_byte_starts(tok, batch):
    texts = fh.CUT_BATCHES[batch]
    ctx = tok._device()
    data, starts = tok._device_input(texts)
    for k, seed, rate in fh.cut_runs():
        if k != batch:
            continue
        exp = tok.fim_cuts(texts, fim_rate=rate, spm_rate=0.5, seed=seed, first_doc=3)
        po, cu = ctx.fim_cuts_to_host(data, None, starts, seed=seed, first_doc=3, fim=fh.threshold(rate), spm=1 << 31)
        assert (po.dtype, cu.dtype) == (np.uint64, np.uint64)
        assert [tuple(r) for r in cu.tolist()] == exp, seed
        assert np.array_equal(po, fh.piece_starts(texts, exp)), seed
        assert ctx.fim_stats()["n_docs"] == len(texts)
        got_cuts, got_po = tok.fim_cuts_array(texts, fim_rate=rate, spm_rate=0.5, seed=seed, first_doc=3)  # the Python twin
        assert np.array_equal(got_cuts, cu) and np.array_equal(got_po, po)


def test_device_text_and_a_bytes_buffer(tok):
    texts = fh.CUT_BATCHES[len(fh.CUT_TEXTS)]  # every text as neighbours
    ctx = tok._device()
    data, starts = tok._device_input(texts)
    host = ctx.fim_cuts_to_host(data, None, starts, seed=4, fim=1 << 32, spm=1 << 31)
    buf = np.frombuffer(data, np.uint8)
    pad = np.zeros(-len(buf) % 4, np.uint8)
    d_text = ctx.mask(np.concatenate((buf, pad)).view(np.uint32), None, None, None, None, select=0)[0]  # the text in device memory
    for shift in (0, 1):  # aligned, and one byte in: the call aligns its own copy
        dev = ctx.fim_cuts_to_host(d_text + shift, len(data) - shift, [0], seed=4, fim=1 << 32, spm=1 << 31)
        one = ctx.fim_cuts_to_host(data[shift:], None, None, seed=4, fim=1 << 32, spm=1 << 31)  # a bytes buffer as one document
        assert all(np.array_equal(a, b) for a, b in zip(dev, one))
        whole = data[shift:].decode("utf-8")
        exp = tok.fim_cuts([whole], fim_rate=1, seed=4)
        assert [tuple(r) for r in one[1].tolist()] == exp and np.array_equal(one[0], fh.piece_starts([whole], exp))
    dev = ctx.fim_cuts_to_host(d_text, len(data), starts, seed=4, fim=1 << 32, spm=1 << 31)
    assert all(np.array_equal(a, b) for a, b in zip(dev, host))
    assert np.array_equal(ctx.d2h(d_text, len(data)), buf)  # the text is left alone
    got_cuts, got_po = tok.fim_cuts_array(data, fim_rate=1, seed=4)  # bytes: one document
    assert got_cuts.shape == (1, 3) and got_po[0, 0] == 0 and got_po[0, 2] <= len(data)


def test_a_model_that_changes_the_text(tok):
    low = mh.tokenizer(mh.SPECIALS_LOWER, lowercase=True, normalizer="nfc")
    import unicodedata

    texts = [unicodedata.normalize("NFD", "NAÏVE Café İstanbul") * 3, "", "ÉÉ plain", "İİİİ"]
    exp = low.fim_cuts(texts, fim_rate=1, seed=6)
    got_cuts, got_po = low.fim_cuts_array(texts, fim_rate=1, seed=6)
    assert [tuple(r) for r in got_cuts.tolist()] == exp
    assert np.array_equal(got_po, fh.piece_starts([low.normalize(t) for t in texts], exp))
    assert any(len(low.normalize(t)) != len(t) for t in texts)
