"""CPU: the contract of BBPETokenizer.encode_with_offsets / encode_batch_with_offsets in plain Python -- the ids are
encode's, byte spans name the bytes every token was merged from (tokens the vocab lacks and specials included, a special
without an id leaves a gap), char spans follow from them by the lead rule."""
from __future__ import annotations

import pytest

from tests import encode_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

IDENT = {bytes([i]): i for i in range(256)}


def lead(data: bytes, p: int) -> int:
    return sum(1 for b in data[:p] if b & 0xC0 != 0x80)


def dropped_specials_removed(tok: BBPETokenizer, text: str) -> bytes:
    """The document's bytes without the occurrences of specials that have no id (the tokenizer's own split)."""
    if tok._special_pattern is None:
        return text.encode("utf-8")
    parts = [p for p in tok._special_pattern.split(text) if p]
    return b"".join(p.encode("utf-8") for p in parts if not (p in tok._special_set and p.encode("utf-8") not in tok._vocab))


def test_g9_setups_both_units(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    assert len(setups) >= 5
    for _idx, name, tok in setups:
        unk = tok._vocab.get(b"[UNK]", 0)
        batch_b = tok.encode_batch_with_offsets(g9["texts"], "byte")
        batch_c = tok.encode_batch_with_offsets(g9["texts"])
        for text, (ids_b, sp_b), (ids_c, sp_c) in zip(g9["texts"], batch_b, batch_c):
            data = text.encode("utf-8")
            assert ids_b == ids_c == tok.encode(text), (name, text)
            assert (ids_b, sp_b) == tok.encode_with_offsets(text, "byte") and (ids_c, sp_c) == tok.encode_with_offsets(text, "char")
            assert len(sp_b) == len(sp_c) == len(ids_b)
            for sp in (sp_b, sp_c):
                assert all(s < e for s, e in sp), (name, text)
                assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(sp, sp[1:])), (name, text)
            assert all(a[1] <= b[0] for a, b in zip(sp_b, sp_b[1:])), (name, text)  # bytes never overlap
            assert b"".join(data[s:e] for s, e in sp_b) == dropped_specials_removed(tok, text), (name, text)
            for i, (s, e) in zip(ids_b, sp_b):
                if data[s:e] in tok._vocab:
                    assert tok._vocab_inv[i] == data[s:e], (name, text, s, e)
                else:
                    assert i == unk
            assert sp_c == [(lead(data, s + 1) - 1, lead(data, e)) for s, e in sp_b], (name, text)
            for (s, e), (sc, ec) in zip(sp_b, sp_c):
                assert data[s:e] in text[sc:ec].encode("utf-8")


def test_hand_pinned_cases():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    assert tok.encode_with_offsets("aé", "byte") == ([0x61, 0xC3, 0xA9], [(0, 1), (1, 2), (2, 3)])
    assert tok.encode_with_offsets("aé", "char") == ([0x61, 0xC3, 0xA9], [(0, 1), (1, 2), (1, 2)])
    assert tok.encode_with_offsets("aé") == tok.encode_with_offsets("aé", "char")  # the default unit
    assert tok.encode_with_offsets("😀") == ([0xF0, 0x9F, 0x98, 0x80], [(0, 1)] * 4)
    assert tok.encode_with_offsets("😀", "byte")[1] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert tok.encode_with_offsets("") == ([], []) and tok.encode_batch_with_offsets([]) == []
    merged = BBPETokenizer(vocab={**IDENT, b"\xc3\xa9": 300}, merges=[(b"\xc3", b"\xa9")])
    assert merged.encode_with_offsets("aé") == ([0x61, 300], [(0, 1), (1, 2)])
    assert merged.encode_with_offsets("aé", "byte") == ([0x61, 300], [(0, 1), (1, 3)])


def test_specials_and_unknown_tokens():
    tok = BBPETokenizer(vocab={**IDENT, b"<s>": 400}, merges=[], special_tokens=["<s>", "<t>"])
    # "<s>" has an id and spans its occurrence; "<t>" has none: no id, and its bytes are a gap
    assert tok.encode_with_offsets("é<s>b<t>c", "byte") == ([0xC3, 0xA9, 400, 0x62, 0x63], [(0, 1), (1, 2), (2, 5), (5, 6), (9, 10)])
    assert tok.encode_with_offsets("é<s>b<t>c", "char") == ([0xC3, 0xA9, 400, 0x62, 0x63], [(0, 1), (0, 1), (1, 4), (4, 5), (8, 9)])
    assert tok.encode_with_offsets("<t>") == ([], [])
    unk = BBPETokenizer(vocab={**IDENT, b"[UNK]": 999}, merges=[(b"a", b"b")])  # "ab" is merged, but no vocab entry names it
    assert unk.encode_with_offsets("ab", "byte") == ([999], [(0, 2)]) == unk.encode_with_offsets("ab", "char")
    assert BBPETokenizer(vocab=dict(IDENT), merges=[(b"a", b"b")]).encode_with_offsets("ab c", "byte") == ([0, 0x20, 0x63], [(0, 2), (2, 3), (3, 4)])


def test_unit_is_checked_and_plain_encode_is_untouched():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[(b"a", b"b")])
    for call in (lambda: tok.encode_with_offsets("ab", unit="x"), lambda: tok.encode_batch_with_offsets(["ab"], unit="bytes"),
                 lambda: tok.encode_batch_with_offsets([], unit="x")):
        with pytest.raises(ValueError):
            call()
    before = tok.cache_info()
    tok.encode_with_offsets("zz zz")
    assert tok.cache_info() != before  # the ids come through the word cache, as encode's do ...
    assert tok.encode("ab ab") == [0, 0x20, 0] and tok._encode_word("ab") == [0]
    tok.clear_cache()
    assert tok.cache_info().startswith("hits=0, misses=0, size=0/")
