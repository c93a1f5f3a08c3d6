"""Byte-level BPE tokenizer: consumer of the trainer's (vocab, merges).

Plain Python, same public API as the reference `src/yet_another_bpe/tokenizer.py:35-398`
(encode, decode, encode_batch, decode_batch, from_file, vocab_size, special_tokens, get_vocab,
clear_cache, cache_info, _encode_word).  encode / encode_batch / decode / decode_batch stay plain Python;
encode_array / encode_batch_device compute the same ids on the GPU (yabpe_encode, include/yabpe.h), and
decode_array / decode_batch_device the same text (yabpe_decode).  encode_with_offsets / encode_batch_with_offsets also say
which bytes or characters of the text every id covers; encode_array_with_offsets / encode_batch_device_with_offsets compute
the same on the GPU (yabpe_encode_spans).  encode_batch_padded / encode_batch_packed lay a batch out in the two fixed shapes a
model consumes; encode_array_padded / encode_array_packed compute the same on the GPU (yabpe_layout_pad / yabpe_layout_pack).
encode_dropout / encode_batch_dropout segment with BPE-dropout, reproducibly from (seed, document, position);
encode_array_dropout / encode_batch_device_dropout compute the same ids on the GPU (yabpe_encode_dropout), and the fixed-shape
forms take dropout= and seed=.  encode_with_words also says which piece of its document every id was made from, mask_tokens
draws a seeded masked-language-model mask over such ids, encode_batch_masked lays both out as padded rows;
encode_array_with_words / mask_array / encode_array_masked compute the same on the GPU (yabpe_encode_words, yabpe_mask).
"""
from __future__ import annotations

import json
import numbers
import operator
from collections.abc import Sequence
from functools import lru_cache
from pathlib import Path

import numpy as np
import regex

from .synth import rnd_int
from .trainer import (CL100K_DIGIT_GROUP, NORMALIZERS, PRETOKENIZER_NAMES, BBPETrainerConfig, check_digit_group, check_errors,
                      check_lowercase, check_lowercase_specials, check_normalized_specials, check_normalizer, check_pretokenizer, device_options,
                      device_text_front, lowercase_text, normalize_text, read_lowercase, read_normalizer, read_pretokenizer, split_pattern)

_WORD_CACHE = 8192


class BBPETokenizer:
    """Applies learned merges, lowest rank first (leftmost on ties), to GPT-2 pre-tokens; with digit_group = G (1 .. 255; not
    in the reference) to the pre-tokens of the pattern whose \\p{N}+ is \\p{N}{1,G} -- the pre-tokenisation of a model trained
    with BBPETrainerConfig(digit_group=G); with pretokenizer = "cl100k" to those of the GPT-4 / Llama-3 pattern, with
    "o200k_base" to those of the GPT-4o pattern (digit_group None: 3 for both).  Every method, plain Python or on the GPU, follows it.
    With normalizer = "nfc" every method that takes text replaces each document by unicodedata.normalize("NFC", document) first
    (on the GPU: yabpe_normalize in front of the encode call), so encode(x) == encode(normalize(x)); the specials are matched in
    the normalised text (a special that is not NFC itself: ValueError), and the spans of the *_with_offsets methods, in bytes
    and in characters, refer to the normalised document, which normalize() / normalize_array() return.  Decoding is untouched.
    With lowercase = True every method that takes text replaces each document by document.lower() first -- before the
    normaliser, so with "nfc" as well a document becomes NFC(document.lower()) (on the GPU: yabpe_lowercase in front of
    yabpe_normalize and the encode call).  Lower-then-NFC is idempotent, so encode(x) == encode(normalize(x)) still holds; the
    specials are matched in the lowered text (a special that is not lower case itself: ValueError), the spans refer to the
    lowered, then normalised document, which normalize() / normalize_array() return, and decoding is untouched."""

    def __init__(self, vocab: dict[bytes, int] | None = None, merges: list[tuple[bytes, bytes]] | None = None,
                 special_tokens: list[str] | None = None, digit_group: int | None = None, pretokenizer: str = "gpt2",
                 normalizer: str | None = None, lowercase: bool = False) -> None:
        self._vocab: dict[bytes, int] = vocab or {}
        self._vocab_inv: dict[int, bytes] = {i: t for t, i in self._vocab.items()}
        self._merges: list[tuple[bytes, bytes]] = merges or []
        self._special_tokens: list[str] = special_tokens or []
        self._special_set = frozenset(self._special_tokens)
        self._rank: dict[tuple[bytes, bytes], int] = {pair: i for i, pair in enumerate(self._merges)}
        self._pretokenizer: str = PRETOKENIZER_NAMES[check_pretokenizer(pretokenizer)]
        self._digit_group: int | None = check_digit_group(digit_group) or (CL100K_DIGIT_GROUP if self._pretokenizer != "gpt2" else None)
        self._pattern = regex.compile(split_pattern(self._digit_group, self._pretokenizer))
        self._normalizer: str | None = NORMALIZERS[check_normalizer(normalizer)]
        check_normalized_specials(self._special_tokens, self._normalizer)
        self._lowercase: bool = check_lowercase(lowercase)
        check_lowercase_specials(self._special_tokens, self._lowercase)
        # specials are split out first, longest first (reference tokenizer.py:100-102)
        self._special_pattern = None
        if self._special_tokens:
            ordered = sorted(self._special_tokens, key=len, reverse=True)
            self._special_pattern = regex.compile("(" + "|".join(regex.escape(t) for t in ordered) + ")")
        self._word_ids = lru_cache(maxsize=_WORD_CACHE)(self._word_ids_uncached)
        self._word_lens = lru_cache(maxsize=_WORD_CACHE)(self._word_lens_uncached)  # (a cache of its own: cache_info is _word_ids')
        self._device_ctx = None  # created on the first device call (encode_array / decode_array and their batch forms)
        self._device_models: set[str] = set()  # models uploaded to it: "encode", "decode" (each on its first use)

    # ------------------------------------------------------------------ persistence (tokenizer.py:106-150)
    @classmethod
    def from_file(cls, model_dir: str | Path) -> "BBPETokenizer":
        d = Path(model_dir)
        with open(d / "vocab.json", encoding="utf-8") as f:
            vocab = {k.encode("latin-1"): v for k, v in json.load(f).items()}
        merges: list[tuple[bytes, bytes]] = []
        with open(d / "merges.txt", encoding="utf-8") as f:
            for line in f:
                line = line.rstrip("\n")
                if not line:
                    continue
                left, sep, right = line.partition(" ")  # first space splits (tokenizer.py:137)
                if sep:
                    merges.append((left.encode("latin-1"), right.encode("latin-1")))
        specials: list[str] = []
        sp = d / "special_tokens.json"
        if sp.exists():
            with open(sp, encoding="utf-8") as f:
                specials = list(json.load(f))
        name, group = read_pretokenizer(d)
        return cls(vocab=vocab, merges=merges, special_tokens=specials, digit_group=group, pretokenizer=name, normalizer=read_normalizer(d),
                   lowercase=read_lowercase(d))

    @classmethod
    def from_file_lossless(cls, model_dir: str | Path) -> "BBPETokenizer":
        """Loads what BBPETrainer.save_lossless wrote (hex files): every token and merge exactly as trained."""
        d = Path(model_dir)
        with open(d / "vocab.hex.json", encoding="ascii") as f:
            vocab = {bytes.fromhex(k): v for k, v in json.load(f).items()}
        merges: list[tuple[bytes, bytes]] = []
        with open(d / "merges.hex", encoding="ascii") as f:
            for line in f:
                left, _, right = line.strip().partition(" ")
                if left or right:
                    merges.append((bytes.fromhex(left), bytes.fromhex(right)))
        specials: list[str] = []
        if (d / "special_tokens.json").exists():
            with open(d / "special_tokens.json", encoding="utf-8") as f:
                specials = list(json.load(f))
        name, group = read_pretokenizer(d)
        return cls(vocab=vocab, merges=merges, special_tokens=specials, digit_group=group, pretokenizer=name, normalizer=read_normalizer(d),
                   lowercase=read_lowercase(d))

    # ------------------------------------------------------------------ encode
    def _word_parts(self, data: bytes) -> list[bytes]:
        parts = [bytes([b]) for b in data]
        rank = self._rank
        while len(parts) > 1:
            best_rank, best_i = None, -1
            for i in range(len(parts) - 1):
                r = rank.get((parts[i], parts[i + 1]))
                if r is not None and (best_rank is None or r < best_rank):
                    best_rank, best_i = r, i
            if best_rank is None:
                break
            parts[best_i:best_i + 2] = [parts[best_i] + parts[best_i + 1]]
        return parts

    def _word_ids_uncached(self, word: str) -> tuple[int, ...]:
        data = word.encode("utf-8")
        if not data:
            return ()
        unk = self._vocab.get(b"[UNK]", 0)
        return tuple(self._vocab.get(p, unk) for p in self._word_parts(data))

    def _word_lens_uncached(self, word: str) -> tuple[int, ...]:
        """The byte length of every part of the word: one per id of _word_ids(word), in the vocab or not."""
        return tuple(len(p) for p in self._word_parts(word.encode("utf-8")))

    def _encode_word(self, word: str) -> list[int]:
        return list(self._word_ids(word))

    def _encode_plain(self, text: str, out: list[int]) -> None:
        for pre in self._pattern.findall(text):
            out.extend(self._word_ids(pre))

    def normalize(self, text: str) -> str:
        """The document the ids and spans of `text` refer to: `text` lowered when the model lowers, then as the model's
        normaliser leaves it (neither: as it is)."""
        return normalize_text(lowercase_text(text, self._lowercase), self._normalizer)

    def encode(self, text: str) -> list[int]:
        return self._encode_normalized(self.normalize(text))

    def _encode_normalized(self, text: str) -> list[int]:
        """the ids of a text that normalize() has already seen (or a piece cut out of one): specials, pattern, merges"""
        if not text:
            return []
        ids: list[int] = []
        if self._special_pattern is None:
            self._encode_plain(text, ids)
            return ids
        for part in self._special_pattern.split(text):
            if not part:
                continue
            if part in self._special_set:
                tid = self._vocab.get(part.encode("utf-8"))
                if tid is not None:
                    ids.append(tid)
            else:
                self._encode_plain(part, ids)
        return ids

    def encode_batch(self, texts: Sequence[str]) -> list[list[int]]:
        return [self.encode(t) for t in texts]

    # ------------------------------------------------------------------ encode with BPE-dropout
    @staticmethod
    def _dropout_threshold(p) -> int:
        """T = min(2^32, int(p * 2^32)): a draw (32 bits) below T drops its candidate.  p: a real number in [0, 1]."""
        if not isinstance(p, numbers.Real) or not 0.0 <= float(p) <= 1.0:  # (NaN compares false)
            raise ValueError(f"p must be a real number in [0, 1], not {p!r}")
        return min(1 << 32, int(float(p) * 4294967296.0))

    @staticmethod
    def _u64(value, name: str) -> int:
        try:
            value = operator.index(value)
        except TypeError:
            raise ValueError(f"{name} must be an integer in [0, 2^64), not {value!r}") from None
        if not 0 <= value < 1 << 64:
            raise ValueError(f"{name} must be an integer in [0, 2^64), not {value!r}")
        return value

    def _word_parts_dropout(self, data: bytes, kw: int, T: int) -> list[bytes]:
        """_word_parts where, at step t (merges performed so far), the candidate whose left part starts at byte q is dropped
        iff rnd(kw, t, q) >> 32 < T; the surviving candidate of lowest rank merges, leftmost on ties; none: finished."""
        parts = [bytes([b]) for b in data]
        starts = list(range(len(data)))
        rank = self._rank
        t = 0
        while len(parts) > 1:
            best_rank, best_i = None, -1
            for i in range(len(parts) - 1):
                r = rank.get((parts[i], parts[i + 1]))
                if r is None or (rnd_int(kw, t, starts[i]) >> 32) < T:
                    continue
                if best_rank is None or r < best_rank:
                    best_rank, best_i = r, i
            if best_rank is None:
                break
            parts[best_i:best_i + 2] = [parts[best_i] + parts[best_i + 1]]
            del starts[best_i + 1]
            t += 1
        return parts

    def encode_dropout(self, text: str, p: float, seed: int = 0, *, doc: int = 0) -> list[int]:
        """encode(text) with BPE-dropout (Provilkov et al., 2020): at every merge step of every pre-token each candidate pair
        is skipped with probability p.  The result depends on (model, text, p, seed, doc) alone: with rnd of synth.py, the
        document key is Kd = rnd(seed, 0x64, doc), the key of the pre-token at byte s of text.encode("utf-8") is Kw =
        rnd(Kd, 0x77, s), and _word_parts_dropout draws from Kw.  The special split, the pre-tokens, [UNK] and the specials
        are encode's; specials draw nothing.  p = 0 gives encode(text), p = 1 one id per byte of every pre-token.
        Nothing is cached: every occurrence of a word draws on its own."""
        T = self._dropout_threshold(p)
        seed, doc = self._u64(seed, "seed"), self._u64(doc, "doc")
        text = self.normalize(text)
        if not text:
            return []
        kd = rnd_int(seed, 0x64, doc)
        unk = self._vocab.get(b"[UNK]", 0)
        ids: list[int] = []
        pos = 0  # byte offset into text.encode("utf-8"), as in _byte_spans
        parts = [text] if self._special_pattern is None else self._special_pattern.split(text)
        for part in parts:
            if not part:
                continue
            if part in self._special_set:
                data = part.encode("utf-8")
                tid = self._vocab.get(data)
                if tid is not None:
                    ids.append(tid)
                pos += len(data)
                continue
            for pre in self._pattern.findall(part):
                data = pre.encode("utf-8")
                ids.extend(self._vocab.get(x, unk) for x in self._word_parts_dropout(data, rnd_int(kd, 0x77, pos), T))
                pos += len(data)
        return ids

    def encode_batch_dropout(self, texts: Sequence[str], p: float, seed: int = 0) -> list[list[int]]:
        """Document d draws as encode_dropout(texts[d], p, seed, doc=d): equal documents of one batch differ."""
        return [self.encode_dropout(t, p, seed, doc=d) for d, t in enumerate(texts)]

    def _encode_batch_for_layout(self, texts: Sequence[str], dropout, seed) -> list[list[int]]:
        """the content ids of the fixed-shape forms: encode_batch's, or encode_batch_dropout's when a draw can drop"""
        T, seed = self._dropout_threshold(dropout), self._u64(seed, "seed")
        return self.encode_batch_dropout(texts, dropout, seed) if T else self.encode_batch(texts)

    # ------------------------------------------------------------------ encode with offsets
    def _byte_spans(self, text: str) -> tuple[list[int], list[tuple[int, int]]]:
        ids: list[int] = []
        spans: list[tuple[int, int]] = []
        pos = 0  # byte offset into text.encode("utf-8"); the parts of the special split and the pre-tokens tile the text

        def plain(part: str) -> None:
            nonlocal pos
            for pre in self._pattern.findall(part):
                ids.extend(self._word_ids(pre))
                for n in self._word_lens(pre):
                    spans.append((pos, pos + n))
                    pos += n

        if self._special_pattern is None:
            plain(text)
            return ids, spans
        for part in self._special_pattern.split(text):
            if not part:
                continue
            if part in self._special_set:
                data = part.encode("utf-8")
                tid = self._vocab.get(data)
                if tid is not None:
                    ids.append(tid)
                    spans.append((pos, pos + len(data)))
                pos += len(data)  # (without an id: no span, a gap)
            else:
                plain(part)
        return ids, spans

    def encode_with_offsets(self, text: str, unit: str = "char") -> tuple[list[int], list[tuple[int, int]]]:
        """-> (encode(text), one (start, end) per id).  unit "byte": offsets into text.encode("utf-8"), the bytes the token was
        merged from (also when the vocab lacks it and the id is [UNK]'s); a special with an id spans its occurrence, one without
        an id leaves a gap; everything else tiles the text in ascending order.  unit "char": code-point offsets into text, the
        smallest run of whole characters that covers the token's bytes -- with lead(p) = the non-continuation bytes below p,
        (lead(start + 1) - 1, lead(end))."""
        if unit not in ("char", "byte"):
            raise ValueError(f"unit must be 'char' or 'byte', not {unit!r}")
        text = self.normalize(text)
        if not text:
            return [], []
        ids, spans = self._byte_spans(text)
        if unit == "char" and spans:
            data = np.frombuffer(text.encode("utf-8"), dtype=np.uint8)
            if len(data) != len(text):  # (all ASCII: a byte is a character)
                lead = np.zeros(len(data) + 1, dtype=np.int64)
                np.cumsum((data & 0xC0) != 0x80, out=lead[1:])
                lead = lead.tolist()
                spans = [(lead[s + 1] - 1, lead[e]) for s, e in spans]
        return ids, spans

    def encode_batch_with_offsets(self, texts: Sequence[str], unit: str = "char"):
        if unit not in ("char", "byte"):
            raise ValueError(f"unit must be 'char' or 'byte', not {unit!r}")
        return [self.encode_with_offsets(t, unit) for t in texts]

    # ------------------------------------------------------------------ encode with the word index of every id
    def encode_with_words(self, text: str) -> tuple[list[int], list[int], list[bool]]:
        """-> (encode(text), words, special), one entry per id.  The pieces of the (normalised) document, in order, are every
        occurrence of a special token, with an id or without, and every match of the split pattern in the text between them
        -- what _byte_spans walks.  words[k] = the 0-based index of the piece id k was made from, special[k] = that piece is a
        special occurrence.  words never decreases; a special without an id takes an index and emits nothing: a gap.  The
        word_ids() of a tokenizer user: whole-word masking and word-level labels align on it."""
        text = self.normalize(text)
        ids: list[int] = []
        words: list[int] = []
        special: list[bool] = []
        if not text:
            return ids, words, special
        index = 0
        for part in [text] if self._special_pattern is None else self._special_pattern.split(text):
            if not part:
                continue
            if part in self._special_set:
                tid = self._vocab.get(part.encode("utf-8"))
                if tid is not None:
                    ids.append(tid)
                    words.append(index)
                    special.append(True)
                index += 1
                continue
            for pre in self._pattern.findall(part):
                got = self._word_ids(pre)
                ids.extend(got)
                words.extend([index] * len(got))
                special.extend([False] * len(got))
                index += 1
        return ids, words, special

    def encode_batch_with_words(self, texts: Sequence[str]):
        return [self.encode_with_words(t) for t in texts]

    # ------------------------------------------------------------------ masked-language-model batches
    IGNORE_LABEL = -100  # the label of a slot the loss skips

    def _mask_args(self, mask_id, p, seed, whole_word, mask_fraction, random_fraction, n_random, first_doc, have_words: bool):
        """-> (mask id, Ts, Tm, Tr, n_random, seed, first_doc), validated"""
        Ts, Tm, Tr = (self._dropout_threshold(x) for x in (p, mask_fraction, random_fraction))
        if Tm + Tr > 1 << 32:
            raise ValueError(f"mask_fraction + random_fraction must be at most 1, not {mask_fraction!r} + {random_fraction!r}")
        seed, first_doc = self._u64(seed, "seed"), self._u64(first_doc, "first_doc")
        if mask_id is None:
            mask_id = self._vocab.get(b"[MASK]")
            if mask_id is None:
                raise ValueError("mask_id is None and the vocab has no b'[MASK]'")
        mask_id = self._layout_ids(mask_id, None, None)[0]
        if n_random is None:
            n_random = max(self._vocab.values(), default=-1) + 1
        try:
            n_random = operator.index(n_random)
        except TypeError:
            raise ValueError(f"n_random must be an integer in [0, 2^32), not {n_random!r}") from None
        if not 0 <= n_random < 1 << 32:
            raise ValueError(f"n_random must be an integer in [0, 2^32), not {n_random!r}")
        if Tr and not n_random:
            raise ValueError("n_random must be at least 1 when random_fraction > 0")
        if whole_word and not have_words:
            raise ValueError("whole_word=True needs words_batch: the piece index of every id (encode_with_words)")
        return mask_id, Ts, Tm, Tr, n_random, seed, first_doc

    def mask_tokens(self, ids_batch, words_batch=None, special_batch=None, *, mask_id: int | None = None, p: float = 0.15, seed: int = 0,
                    whole_word: bool = False, mask_fraction: float = 0.8, random_fraction: float = 0.1, n_random: int | None = None,
                    first_doc: int = 0) -> tuple[list[list[int]], list[list[int]]]:
        """One dynamic-masking draw of masked-language-model training -> (inputs, labels), shaped as ids_batch.  The result
        depends on (ids, words, special, the arguments) alone: with rnd of synth.py, T(x) = min(2^32, int(x * 2^32)), Ts =
        T(p), Tm = T(mask_fraction), Tr = T(random_fraction) (Tm + Tr > 2^32: ValueError), document d has the key Kd =
        rnd(seed, 0x6d, first_doc + d).  For token j of the document (0-based): the unit is u = j, with whole_word u =
        words[j].  A token whose `special` is true is never selected and draws nothing.  Otherwise r = rnd(Kd, 0x73, u), and
        the token is selected iff (r >> 32) < Ts.  A selected token's label is its id, and x = r & 0xFFFFFFFF decides its
        input: x < Tm: mask_id; Tm <= x < Tm + Tr: rnd(Kd, 0x72, j) % n_random (per token in whole-word mode too); else the id
        stays.  An unselected token keeps its id and has the label -100.  So all tokens of a word share selection and kind.
        mask_id None: the id of b"[MASK]" (none: ValueError); n_random None: max(vocab ids) + 1; whole_word without
        words_batch: ValueError; without special_batch nothing is protected."""
        mid, Ts, Tm, Tr, n_random, seed, first_doc = self._mask_args(mask_id, p, seed, whole_word, mask_fraction, random_fraction, n_random,
                                                                     first_doc, words_batch is not None)
        inputs, labels = [], []
        for d, ids in enumerate(ids_batch):
            kd = rnd_int(seed, 0x6d, first_doc + d)
            words = words_batch[d] if whole_word else None
            special = special_batch[d] if special_batch is not None else None
            row, lab = [], []
            for j, tid in enumerate(ids):
                tid = int(tid)
                new, label = tid, self.IGNORE_LABEL
                if special is None or not special[j]:
                    r = rnd_int(kd, 0x73, int(words[j]) if whole_word else j)
                    if (r >> 32) < Ts:
                        label, x = tid, r & 0xFFFFFFFF
                        if x < Tm:
                            new = mid
                        elif x < Tm + Tr:
                            new = rnd_int(kd, 0x72, j) % n_random
                row.append(new)
                lab.append(label)
            inputs.append(row)
            labels.append(lab)
        return inputs, labels

    def encode_batch_masked(self, texts: Sequence[str], max_length: int | None = None, *, mask_id: int | None = None, p: float = 0.15,
                            seed: int = 0, whole_word: bool = False, mask_fraction: float = 0.8, random_fraction: float = 0.1,
                            n_random: int | None = None, first_doc: int = 0, pad_id: int | None = None, bos_id: int | None = None,
                            eos_id: int | None = None, truncation: str = "right",
                            padding_side: str = "right") -> tuple[list[list[int]], list[list[int]], list[int]]:
        """Masked-language-model rows in one call -> (rows, labels, lengths): encode_batch_with_words, then mask_tokens over the
        whole documents with their words and specials (the mask is drawn before the cut: a token's fate does not depend on
        max_length), then the rows laid out as encode_batch_padded lays them out, and the labels the same way with -100 in
        BOS, EOS and pad slots."""
        L, pad, bos, eos, added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        self._mask_args(mask_id, p, seed, whole_word, mask_fraction, random_fraction, n_random, first_doc, True)  # (refused before any work)
        docs = self.encode_batch_with_words(texts)
        inputs, labels = self.mask_tokens([d[0] for d in docs], [d[1] for d in docs], [d[2] for d in docs], mask_id=mask_id, p=p, seed=seed,
                                          whole_word=whole_word, mask_fraction=mask_fraction, random_fraction=random_fraction,
                                          n_random=n_random, first_doc=first_doc)
        if L is None:
            L = max((len(ids) + added for ids in inputs), default=0)
        ign = self.IGNORE_LABEL
        rows, lengths = self._padded_rows(inputs, L, added, pad, bos, eos, truncation, padding_side)
        lab_rows, _ = self._padded_rows(labels, L, added, ign, None if bos is None else ign, None if eos is None else ign, truncation, padding_side)
        return rows, lab_rows, lengths

    # ------------------------------------------------------------------ span-corruption batches (T5 / UL2 / SpanBERT denoising)
    SPAN_MAX_LEN = 32  # YABPE_SPAN_MAX_LEN

    @staticmethod
    def span_thresholds(p: float = 0.15, mean_span_length: float = 3.0, max_span_length: int = 10) -> tuple[int, list[int]]:
        """The integers the span rule runs on, from the user's numbers -> (To, C), len(C) = max_span_length - 1.  With T(x) =
        min(2^32, int(x * 2^32)): C[k] = T((1 - 1/mean)^(k + 1)), the power by repeated multiplication: a drawn span is longer
        than k + 1 units with probability C[k] / 2^32, a geometric length of mean mean_span_length that is clamped at
        max_span_length.  A unit is noise iff an opener at most max_span_length - 1 units back reaches it, so with an opening
        probability q its density is 1 - prod_{k < Lmax} (1 - q * S_k), S_0 = 1, S_k = C[k - 1] / 2^32; q is what 64 bisection
        steps on [0, 1] leave as the upper end for density p, and To = T(q).  Doubles and + - * / only: every machine
        gets the same integers."""
        if not isinstance(p, numbers.Real) or not 0.0 <= float(p) <= 1.0:  # (NaN compares false)
            raise ValueError(f"p must be a real number in [0, 1], not {p!r}")
        if not isinstance(mean_span_length, numbers.Real) or not 1.0 <= float(mean_span_length) < float("inf"):
            raise ValueError(f"mean_span_length must be a real number of at least 1, not {mean_span_length!r}")
        try:
            Lmax = operator.index(max_span_length)
        except TypeError:
            raise ValueError(f"max_span_length must be an integer in [1, {BBPETokenizer.SPAN_MAX_LEN}], not {max_span_length!r}") from None
        if not 1 <= Lmax <= BBPETokenizer.SPAN_MAX_LEN:
            raise ValueError(f"max_span_length must be an integer in [1, {BBPETokenizer.SPAN_MAX_LEN}], not {max_span_length!r}")
        p, a = float(p), 1.0 - 1.0 / float(mean_span_length)
        C, power = [], 1.0
        for _ in range(Lmax - 1):
            power = power * a
            C.append(min(1 << 32, int(power * 4294967296.0)))
        S = [1.0] + [c / 4294967296.0 for c in C]
        lo, hi = 0.0, 1.0
        for _ in range(64):
            mid = (lo + hi) / 2.0
            clear = 1.0
            for s in S:
                clear = clear * (1.0 - mid * s)
            if 1.0 - clear < p:
                lo = mid
            else:
                hi = mid
        return min(1 << 32, int(hi * 4294967296.0)), C

    def _sentinel_ids(self, sentinels) -> list[int]:
        """ids, or special-token strings that have ids -> ids in [0, 2^32)"""
        if sentinels is None or isinstance(sentinels, (str, bytes)):
            raise ValueError("sentinels must be a sequence of ids or of special-token strings")
        out = []
        for s in sentinels:
            if isinstance(s, str):
                tid = self._vocab.get(s.encode("utf-8")) if s in self._special_set else None
                if tid is None:
                    raise ValueError(f"sentinel {s!r} is not a special token with an id")
                s = tid
            out.append(self._layout_ids(s, None, None)[0])
        return out

    def _span_args(self, sentinels, p, mean_span_length, max_span_length, seed, whole_word, final_sentinel, max_tokens, first_doc, have_words: bool):
        """-> (sentinel ids, To, C, seed, first_doc, max_doc_ids), validated"""
        To, C = self.span_thresholds(p, mean_span_length, max_span_length)
        sent = self._sentinel_ids(sentinels)
        if len(sent) < (2 if final_sentinel else 1):
            raise ValueError(f"{len(sent)} sentinels: at least {2 if final_sentinel else 1} (one for a run" + (", one to end the targets)" if final_sentinel else ")"))
        seed, first_doc = self._u64(seed, "seed"), self._u64(first_doc, "first_doc")
        cut = 0 if max_tokens is None else self._row_length(max_tokens, "max_tokens", 1)
        if cut >= 1 << 64:
            raise ValueError(f"max_tokens must be below 2^64, not {max_tokens!r}")
        if whole_word and not have_words:
            raise ValueError("whole_word=True needs words_batch: the piece index of every id (encode_with_words)")
        return sent, To, C, seed, first_doc, cut

    @staticmethod
    def _span_noise_units(kd: int, To: int, C: list[int]):
        """-> noise(v) of the document with key kd, by the rule's definition: opens(u) and len(u) per unit, cached"""
        Lmax = len(C) + 1

        @lru_cache(maxsize=None)
        def reach(u: int) -> int:  # one past the last unit u's span covers; u itself if u does not open
            r = rnd_int(kd, 0x6f, u)
            if (r >> 32) >= To:
                return u
            x = r & 0xFFFFFFFF
            return u + 1 + sum(1 for k in range(Lmax - 1) if x < C[k])

        def noise(v: int) -> bool:
            return any(reach(u) > v for u in range(max(0, v - Lmax + 1), v + 1))

        return noise

    def corrupt_spans(self, ids_batch, words_batch=None, special_batch=None, *, sentinels, p: float = 0.15, mean_span_length: float = 3.0,
                      max_span_length: int = 10, seed: int = 0, whole_word: bool = False, final_sentinel: bool = True,
                      max_tokens: int | None = None, first_doc: int = 0) -> tuple[list[list[int]], list[list[int]]]:
        """One span-corruption draw of encoder-decoder denoising (T5 / UL2 / SpanBERT) -> (inputs, targets), one ragged
        sequence each per document: spans leave the input, one sentinel stands for each, and the target lists the sentinels
        with the ids they stand for -- "A <s0> B <s1> C" and "<s0> x y <s1> z <s2>".  The result depends on (ids, words,
        special, the arguments) alone.  (To, C) = span_thresholds(p, mean_span_length, max_span_length), Lmax =
        max_span_length; with rnd of synth.py, document d has the key Kd = rnd(seed, 0x63, first_doc + d).  For token j of the
        document (0-based, counted before the cut) the unit is u = j, with whole_word u = words[j].  Per unit r = rnd(Kd, 0x6f,
        u): the unit opens a span iff (r >> 32) < To, of len(u) = 1 + #{k < Lmax - 1 : (r & 0xFFFFFFFF) < C[k]} units.  Unit v
        is noise iff some u in [max(0, v - Lmax + 1), v] opens with u + len(u) > v.  A token is noise iff its unit is noise and
        its `special` is false: specials are never removed, and they split runs.  No draw reads protection, the cut or the
        batch.  max_tokens (None: no cut): tokens j >= max_tokens appear in neither output; a run the cut ends is shorter.
        A run is a maximal stretch of consecutive kept noise tokens, numbered k = 0, 1, ... per document.  `sentinels`: ids,
        or special-token strings that have ids; K = len(sentinels) - (1 if final_sentinel).  inputs: the kept tokens, every run k
        < K replaced by sentinels[k]; targets: per run k < K, sentinels[k] and the run's ids; with final_sentinel then
        sentinels[min(n_runs, K)], if the document keeps a token at all.  An empty document gives two empty sequences.
        Two approximations, on purpose: overlapping and adjacent spans merge, so mean_span_length is the mean of the drawn
        lengths before the max_span_length clamp, not of the merged runs, which are longer (p = 0.15, mean 3, Lmax 10: drawn 2.94,
        runs 3.25); and runs k >= K are not corrupted -- their ids stay in the input and nothing goes to the target -- so with few
        sentinels the density falls below p.  p is the density of noise units, hit to about 0.001."""
        sent, To, C, seed, first_doc, cut = self._span_args(sentinels, p, mean_span_length, max_span_length, seed, whole_word, final_sentinel,
                                                             max_tokens, first_doc, words_batch is not None)
        K = len(sent) - (1 if final_sentinel else 0)
        inputs, targets = [], []
        for d, ids in enumerate(ids_batch):
            noise = self._span_noise_units(rnd_int(seed, 0x63, first_doc + d), To, C)
            words = words_batch[d] if whole_word else None
            special = special_batch[d] if special_batch is not None else None
            row, tgt, n_runs, in_run = [], [], 0, False
            n_kept = min(len(ids), cut) if cut else len(ids)
            for j in range(n_kept):
                tid = int(ids[j])
                if (special is None or not special[j]) and noise(int(words[j]) if whole_word else j):
                    if not in_run:
                        in_run, n_runs = True, n_runs + 1
                        if n_runs <= K:
                            row.append(sent[n_runs - 1])
                            tgt.append(sent[n_runs - 1])
                    (tgt if n_runs <= K else row).append(tid)
                else:
                    in_run = False
                    row.append(tid)
            if final_sentinel and n_kept:
                tgt.append(sent[min(n_runs, K)])
            inputs.append(row)
            targets.append(tgt)
        return inputs, targets

    def encode_batch_span_corrupted(self, texts: Sequence[str], max_length: int | None = None, max_target_length: int | None = None, *,
                                    sentinels, p: float = 0.15, mean_span_length: float = 3.0, max_span_length: int = 10, seed: int = 0,
                                    whole_word: bool = False, final_sentinel: bool = True, max_tokens: int | None = None, first_doc: int = 0,
                                    pad_id: int | None = None, bos_id: int | None = None, eos_id: int | None = None,
                                    truncation: str = "right", padding_side: str = "right"):
        """Encoder-decoder denoising rows in one call -> (rows, labels, lengths, label_lengths): encode_batch_with_words, then
        corrupt_spans over the documents with their words and specials (max_tokens cuts the documents; the draws do not
        depend on it or on the row lengths), then the inputs laid out as encode_batch_padded lays them out in rows of
        max_length (None: the longest), and the targets the same way in rows of max_target_length with -100 in BOS, EOS and
        pad slots."""
        L, pad, bos, eos, added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        LT = None if max_target_length is None else self._row_length(max_target_length, "max_target_length", added)
        kw = {"sentinels": sentinels, "p": p, "mean_span_length": mean_span_length, "max_span_length": max_span_length, "seed": seed,
              "whole_word": whole_word, "final_sentinel": final_sentinel, "max_tokens": max_tokens, "first_doc": first_doc}
        self._span_args(have_words=True, **kw)  # (refused before any work)
        docs = self.encode_batch_with_words(texts)
        inputs, targets = self.corrupt_spans([d[0] for d in docs], [d[1] for d in docs], [d[2] for d in docs], **kw)
        if L is None:
            L = max((len(ids) + added for ids in inputs), default=0)
        if LT is None:
            LT = max((len(ids) + added for ids in targets), default=0)
        ign = self.IGNORE_LABEL
        rows, lengths = self._padded_rows(inputs, L, added, pad, bos, eos, truncation, padding_side)
        lab_rows, lab_lengths = self._padded_rows(targets, LT, added, ign, None if bos is None else ign, None if eos is None else ign, truncation,
                                                  padding_side)
        return rows, lab_rows, lengths, lab_lengths

    # ------------------------------------------------------------------ fill-in-the-middle batches (decoder-only code models)
    FIM_LOSSES = ("all", "middle")
    FIM_LEVELS = ("char", "token")

    def _fim_args(self, pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc, max_length, loss):
        """-> (pre id, suf id, mid id, eot id or None, Tf, Ts, seed, first_doc, max_len (0: no cut), loss == "middle"), validated
        as yabpe_fim validates them"""
        Tf, Ts = self._dropout_threshold(fim_rate), self._dropout_threshold(spm_rate)
        if loss not in self.FIM_LOSSES:
            raise ValueError(f"loss must be 'all' or 'middle', not {loss!r}")
        for name, v in (("pre", pre), ("suf", suf), ("mid", mid)):
            if v is None:
                raise ValueError(f"{name} must be an id or a special-token string")
        pre, suf, mid = self._sentinel_ids([pre, suf, mid])
        eot = None if eot is None else self._sentinel_ids([eot])[0]
        seed, first_doc = self._u64(seed, "seed"), self._u64(first_doc, "first_doc")
        X = 3 + (eot is not None)
        max_len = 0
        if max_length is not None:
            max_len = self._row_length(max_length, "max_length", 0)
            if max_len <= X:
                raise ValueError(f"max_length must be above {X} (the sentinels always survive), not {max_len}: max_len 0 or above {X}")
            if max_len >= 1 << 64:
                raise ValueError(f"max_length must be below 2^64, not {max_length!r}")
        return pre, suf, mid, eot, Tf, Ts, seed, first_doc, max_len, loss == "middle"

    @staticmethod
    def _fim_draw(seed: int, doc: int, n: int, Tf: int, Ts: int) -> tuple[int, int, int]:
        """-> (mode, a, b) of document number `doc` (first_doc + d) with n units"""
        kd = rnd_int(seed, 0x66, doc)
        r = rnd_int(kd, 0x61, 0)
        if (r >> 32) >= Tf:
            return 0, n, n
        x, y = rnd_int(kd, 0x62, 0) % (n + 1), rnd_int(kd, 0x62, 1) % (n + 1)
        return (2 if (r & 0xFFFFFFFF) < Ts else 1), min(x, y), max(x, y)

    def _fim_sequence(self, mode: int, P: list[int], M: list[int], S: list[int], pre, suf, mid, eot, max_len: int, loss_middle: bool):
        """One document from its three pieces -> (sequence, labels, (mode, p, m, s) after the cut)"""
        ign = self.IGNORE_LABEL
        if mode == 0:
            ids = P + M + S
            if max_len:
                ids = ids[:max_len]
            p = min(len(P), len(ids))
            m = min(len(M), len(ids) - p)
            return ids, list(ids), (0, p, m, len(ids) - p - m)
        X = 3 + (eot is not None)
        if max_len:
            e = max(0, len(P) + len(M) + len(S) - (max_len - X))
            t = min(e, len(S))
            S, e = S[:len(S) - t], e - t
            t = min(e, len(P))
            P, e = P[t:], e - t
            M = M[:len(M) - e]
        tail = [] if eot is None else [eot]
        if mode == 1:
            parts = [([pre], 0), (P, 0), ([suf], 0), (S, 0), ([mid], 0), (M, 1), (tail, 1)]
        else:
            parts = [([pre], 0), ([suf], 0), (S, 0), ([mid], 0), (P, 0), (M, 1), (tail, 1)]
        seq, lab = [], []
        for ids, in_loss in parts:
            seq.extend(ids)
            lab.extend(ids if in_loss or not loss_middle else [ign] * len(ids))
        return seq, lab, (mode, len(P), len(M), len(S))

    def fim_tokens(self, ids_batch, *, pre, suf, mid, eot=None, fim_rate: float = 0.5, spm_rate: float = 0.5, seed: int = 0, first_doc: int = 0,
                   max_length: int | None = None, loss: str = "all") -> tuple[list[list[int]], list[list[int]], list[tuple[int, int, int, int]]]:
        """One fill-in-the-middle draw (Bavarian et al., 2022) at token level -> (sequences, labels, info), one entry each per
        document.  The result depends on (ids, the arguments) alone.  With rnd of synth.py and T(x) = min(2^32, int(x * 2^32)),
        Tf = T(fim_rate), Ts = T(spm_rate): document d has the key Kd = rnd(seed, 0x66, first_doc + d); r = rnd(Kd, 0x61, 0); the
        document is transformed iff (r >> 32) < Tf, and then SPM iff (r & 0xFFFFFFFF) < Ts, else PSM.  With n ids: x = rnd(Kd,
        0x62, 0) % (n + 1), y = rnd(Kd, 0x62, 1) % (n + 1), a = min(x, y), b = max(x, y); P = ids[:a], M = ids[a:b], S = ids[b:].
        PSM: pre P suf S mid M [eot]; SPM: pre suf S mid P M [eot] (prefix and middle adjacent); a document left alone: its ids.
        pre, suf, mid, eot: ids, or special-token strings that have ids; eot None: nothing is appended.
        max_length (None: no cut; else above X = 3 + (1 with eot)): the excess over max_length - X leaves from the end of S, then
        from the start of P, then from the end of M; the sentinels always survive.  A document left alone keeps its first
        max_length ids.  labels: the id of every slot; with loss "middle" -100 everywhere but on M and the eot of a transformed
        document (a document left alone keeps all its labels).  info[d] = (mode, len(P), len(M), len(S)) after the cut, mode 0
        (left alone: (0, kept ids, 0, 0)), 1 (PSM) or 2 (SPM)."""
        pre, suf, mid, eot, Tf, Ts, seed, first_doc, max_len, loss_middle = self._fim_args(pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc,
                                                                                           max_length, loss)
        seqs, labels, info = [], [], []
        for d, ids in enumerate(ids_batch):
            ids = [int(t) for t in ids]
            mode, a, b = self._fim_draw(seed, first_doc + d, len(ids), Tf, Ts)
            seq, lab, inf = self._fim_sequence(mode, ids[:a], ids[a:b], ids[b:], pre, suf, mid, eot, max_len, loss_middle)
            seqs.append(seq)
            labels.append(lab)
            info.append(inf)
        return seqs, labels, info

    def fim_cuts(self, texts: Sequence[str], *, fim_rate: float = 0.5, spm_rate: float = 0.5, seed: int = 0,
                 first_doc: int = 0) -> list[tuple[int, int, int]]:
        """The character-level cuts of fill-in-the-middle -> (mode, a, b) per document, in code points of t = normalize(text):
        the draws of fim_tokens with n = len(t); prefix t[:a], middle t[a:b], suffix t[b:]."""
        Tf, Ts = self._dropout_threshold(fim_rate), self._dropout_threshold(spm_rate)
        seed, first_doc = self._u64(seed, "seed"), self._u64(first_doc, "first_doc")
        return [self._fim_draw(seed, first_doc + d, len(self.normalize(t)), Tf, Ts) for d, t in enumerate(texts)]

    def _fim_level(self, level) -> bool:
        if level not in self.FIM_LEVELS:
            raise ValueError(f"level must be 'char' or 'token', not {level!r}")
        return level == "char"

    def _fim_row_args(self, max_length, pad_id, bos_id, eos_id, truncation, padding_side, pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc, loss):
        """-> (_padded_args' results, _fim_args' results): the sequences are cut to max_length minus BOS and EOS"""
        L, pad, bos, eos, added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        fim = self._fim_args(pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc, None if L is None else L - added, loss)
        return (L, pad, bos, eos, added), fim

    def encode_batch_fim(self, texts: Sequence[str], max_length: int | None = None, *, level: str = "char", pre, suf, mid, eot=None,
                         fim_rate: float = 0.5, spm_rate: float = 0.5, seed: int = 0, first_doc: int = 0, loss: str = "all",
                         pad_id: int | None = None, bos_id: int | None = None, eos_id: int | None = None, truncation: str = "right",
                         padding_side: str = "right"):
        """Fill-in-the-middle rows in one call -> (input_ids, labels, lengths, info).  level "token": fim_tokens over
        encode_batch(texts).  level "char" (the paper's recommended form: a cut through a word shows the model sub-token
        boundaries): t = normalize(text), (mode, a, b) = fim_cuts, and the three pieces t[:a], t[a:b], t[b:] are encoded each
        on its own without normalising again; info then counts the pieces' ids.  A special token that a cut runs through is plain
        text in both pieces; one that lies inside a piece is a special.  (A normaliser is not applied across a cut either: the
        pieces are cut out of the normalised text.)  The sequences are cut by the rule of fim_tokens to max_length minus BOS and
        EOS (None: no cut), so the sentinels survive and `truncation` has nothing left to cut; the rows are laid out as
        encode_batch_padded lays them out (max_length None: the longest), labels with -100 in BOS, EOS and pad slots and
        wherever the loss skips."""
        (L, pad, bos, eos, added), (pre, suf, mid, eot, Tf, Ts, seed, first_doc, max_len, loss_middle) = self._fim_row_args(
            max_length, pad_id, bos_id, eos_id, truncation, padding_side, pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc, loss)
        chars = self._fim_level(level)
        seqs, labels, info = [], [], []
        for d, text in enumerate(texts):
            if chars:
                t = self.normalize(text)
                mode, a, b = self._fim_draw(seed, first_doc + d, len(t), Tf, Ts)
                P, M, S = (self._encode_normalized(x) for x in (t[:a], t[a:b], t[b:]))
            else:
                ids = self.encode(text)
                mode, a, b = self._fim_draw(seed, first_doc + d, len(ids), Tf, Ts)
                P, M, S = ids[:a], ids[a:b], ids[b:]
            seq, lab, inf = self._fim_sequence(mode, P, M, S, pre, suf, mid, eot, max_len, loss_middle)
            seqs.append(seq)
            labels.append(lab)
            info.append(inf)
        if L is None:
            L = max((len(ids) + added for ids in seqs), default=0)
        ign = self.IGNORE_LABEL
        rows, lengths = self._padded_rows(seqs, L, added, pad, bos, eos, truncation, padding_side)
        lab_rows, _ = self._padded_rows(labels, L, added, ign, None if bos is None else ign, None if eos is None else ign, truncation, padding_side)
        return rows, lab_rows, lengths, info

    # ------------------------------------------------------------------ fixed-shape batches
    def _layout_ids(self, pad_id, bos_id, eos_id) -> tuple[int, int | None, int | None, int]:
        """-> (pad id, bos id or None, eos id or None, n_added); every id given must be an integer in [0, 2^32)"""
        if pad_id is None:
            pad_id = self._vocab.get(b"[PAD]", 0)
        out = []
        for name, v in (("pad_id", pad_id), ("bos_id", bos_id), ("eos_id", eos_id)):
            if v is not None:
                try:
                    v = operator.index(v)
                except TypeError:
                    raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}") from None
                if not 0 <= v < 1 << 32:
                    raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
            out.append(v)
        return out[0], out[1], out[2], (bos_id is not None) + (eos_id is not None)

    @staticmethod
    def _row_length(value, name: str, least: int) -> int:
        try:
            value = operator.index(value)
        except TypeError:
            raise ValueError(f"{name} must be an integer, not {value!r}") from None
        if value < least:
            raise ValueError(f"{name} must be at least {least}, not {value}")
        return value

    def _padded_args(self, max_length, pad_id, bos_id, eos_id, truncation, padding_side):
        pad, bos, eos, added = self._layout_ids(pad_id, bos_id, eos_id)
        for name, v in (("truncation", truncation), ("padding_side", padding_side)):
            if v not in ("left", "right"):
                raise ValueError(f"{name} must be 'left' or 'right', not {v!r}")
        if max_length is not None:
            max_length = self._row_length(max_length, "max_length", added)  # (BOS and EOS always survive the cut)
        return max_length, pad, bos, eos, added

    def encode_batch_padded(self, texts: Sequence[str], max_length: int | None = None, *, pad_id: int | None = None,
                            bos_id: int | None = None, eos_id: int | None = None, truncation: str = "right",
                            padding_side: str = "right", dropout: float = 0.0, seed: int = 0) -> tuple[list[list[int]], list[int]]:
        """One row of L = max_length ids per text (None: the longest sequence, 0 without texts) -> (rows, lengths).
        seq(d) = [bos_id] + encode(texts[d]) + [eos_id] (each only if given).  A seq longer than L loses content ids from its
        end (truncation "left": from its start); BOS and EOS always survive.  lengths[d] = the length after the cut; the kept
        sequence sits at the left end of its row (padding_side "left": at the right end), pad_id (None: the id of b"[PAD]",
        else 0) everywhere else.  Ids are any integers in [0, 2^32), in the vocab or not.  dropout > 0: the content ids are
        encode_batch_dropout(texts, dropout, seed)."""
        L, pad, bos, eos, added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        docs = self._encode_batch_for_layout(texts, dropout, seed)
        if L is None:
            L = max((len(ids) + added for ids in docs), default=0)
        return self._padded_rows(docs, L, added, pad, bos, eos, truncation, padding_side)

    @staticmethod
    def _padded_rows(docs, L: int, added: int, pad, bos, eos, truncation: str, padding_side: str) -> tuple[list[list[int]], list[int]]:
        """the rows of encode_batch_padded from the content of every document (ids, or the labels of encode_batch_masked)"""
        rows, lengths = [], []
        for ids in docs:
            keep = min(len(ids), L - added)
            content = ids[:keep] if truncation == "right" else ids[len(ids) - keep:]
            seq = ([bos] if bos is not None else []) + content + ([eos] if eos is not None else [])
            fill = [pad] * (L - len(seq))
            rows.append(seq + fill if padding_side == "right" else fill + seq)
            lengths.append(len(seq))
        return rows, lengths

    def encode_batch_packed(self, texts: Sequence[str], seq_len: int, *, pad_id: int | None = None, bos_id: int | None = None,
                            eos_id: int | None = None, drop_last: bool = False, dropout: float = 0.0,
                            seed: int = 0) -> tuple[list[list[int]], list[list[int]], list[list[int]]]:
        """All seq(d) = [bos_id] + encode(texts[d]) + [eos_id] end to end in document order, cut into rows of seq_len
        -> (ids, doc, pos), each ceil(stream / seq_len) rows (drop_last: floor -- the last partial row is dropped).
        doc[r][c] = the index into texts of the document the slot came from, pos[r][c] = the slot's index inside seq(d) (BOS is
        0).  The slots of the last row past the end of the stream hold pad_id, document 0xFFFFFFFF and position 0.
        dropout > 0: the content ids are encode_batch_dropout(texts, dropout, seed)."""
        pad, bos, eos, _added = self._layout_ids(pad_id, bos_id, eos_id)
        seq_len = self._row_length(seq_len, "seq_len", 1)
        stream, doc, pos = [], [], []
        for d, ids in enumerate(self._encode_batch_for_layout(texts, dropout, seed)):
            seq = ([bos] if bos is not None else []) + ids + ([eos] if eos is not None else [])
            stream += seq
            doc += [d] * len(seq)
            pos += range(len(seq))
        n_rows = len(stream) // seq_len if drop_last else -(-len(stream) // seq_len)
        fill = max(0, n_rows * seq_len - len(stream))
        cut = lambda flat, filler: [(flat + [filler] * fill)[r * seq_len:(r + 1) * seq_len] for r in range(n_rows)]  # noqa: E731
        return cut(stream, pad), cut(doc, 0xFFFFFFFF), cut(pos, 0)

    def encode_batch_fit(self, texts: Sequence[str], seq_len: int, *, pad_id: int | None = None, bos_id: int | None = None,
                         eos_id: int | None = None, dropout: float = 0.0,
                         seed: int = 0) -> tuple[list[list[int]], list[list[int]], list[list[int]], list[int]]:
        """Whole documents in rows of C = seq_len slots, packed by best-fit decreasing: no seq(d) = [bos_id] + encode(texts[d]) +
        [eos_id] is cut across two rows -> (ids, doc, pos, used).  A seq longer than C loses content ids from its end (BOS and
        EOS survive, as in encode_batch_padded); n_d = its length after that; a document with n_d == 0 is in no row.
        Plan, on H[k] = the documents with n_d == k: the state maps a shape -- the lengths of a row's sequences in placement
        order, non-increasing, room = C - their sum -- to the rows that have it.  For k = C .. 1 with n = H[k] sequences left:
        among the shapes with a row left and room >= k the one with the smallest room, of several the greatest tuple; t = room
        // k; min(rows, n // t) of its rows take t sequences each, then, if rows of it and sequences remain, one more row takes
        the rest; with no such shape n // t rows of t = C // k sequences open and one row of the n % t left.
        Rows: the shapes in descending tuple order, the rows of a shape consecutive; a row holds its sequences end to end from
        column 0.  For every k the documents with n_d == k, in ascending d, take the places of length k in row order, within a
        row left to right.  doc and pos are encode_batch_packed's; pad slots hold pad_id, 0xFFFFFFFF and 0; used[r] = the filled
        slots of row r.  dropout > 0: the content ids are encode_batch_dropout(texts, dropout, seed)."""
        pad, bos, eos, added = self._layout_ids(pad_id, bos_id, eos_id)
        C = self._row_length(seq_len, "seq_len", max(1, added))
        seqs = []
        for ids in self._encode_batch_for_layout(texts, dropout, seed):
            seqs.append(([bos] if bos is not None else []) + ids[:max(0, C - added)] + ([eos] if eos is not None else []))
        by_len: dict[int, list[int]] = {}
        for d, seq in enumerate(seqs):
            by_len.setdefault(len(seq), []).append(d)
        count: dict[tuple, int] = {}  # shape -> rows

        def move(src, dst, m):
            if src is not None:
                count[src] -= m
                if not count[src]:
                    del count[src]
            if m:
                count[dst] = count.get(dst, 0) + m

        for k in range(C, 0, -1):
            n = len(by_len.get(k, ()))
            while n:
                fits = [s for s in count if C - sum(s) >= k]
                if not fits:
                    t = C // k
                    move(None, (k,) * t, n // t)
                    if n % t:
                        move(None, (k,) * (n % t), 1)
                    n = 0
                    continue
                least = min(C - sum(s) for s in fits)
                s = max(s for s in fits if C - sum(s) == least)
                t, m = least // k, count[s]
                full = min(m, n // t)
                move(s, s + (k,) * t, full)
                n -= full * t
                if full < m and n:
                    move(s, s + (k,) * n, 1)
                    n = 0
        shapes = [s for s in sorted(count, reverse=True) for _ in range(count[s])]
        taken = {k: iter(docs) for k, docs in by_len.items()}  # the next document of every length
        rows = [[next(taken[k]) for k in s] for s in shapes]
        out_ids, out_doc, out_pos, used = [], [], [], []
        for row in rows:
            fill = C - sum(len(seqs[d]) for d in row)
            out_ids.append([i for d in row for i in seqs[d]] + [pad] * fill)
            out_doc.append([d for d in row for _ in seqs[d]] + [0xFFFFFFFF] * fill)
            out_pos.append([p for d in row for p in range(len(seqs[d]))] + [0] * fill)
            used.append(C - fill)
        return out_ids, out_doc, out_pos, used

    def _windows_args(self, max_length, stride, pad_id, bos_id, eos_id, padding_side, offsets, dropout, seed):
        pad, bos, eos, added = self._layout_ids(pad_id, bos_id, eos_id)
        max_length = self._row_length(max_length, "max_length", added + 1)  # (at least one content slot a row)
        try:
            stride = operator.index(stride)
        except TypeError:
            raise ValueError(f"stride must be an integer, not {stride!r}") from None
        if not 0 <= stride < max_length - added:
            raise ValueError(f"stride must be in [0, {max_length - added - 1}] (max_length less BOS, EOS and one), not {stride}")
        if padding_side not in ("left", "right"):
            raise ValueError(f"padding_side must be 'left' or 'right', not {padding_side!r}")
        if offsets not in (None, "char", "byte"):
            raise ValueError(f"offsets must be None, 'char' or 'byte', not {offsets!r}")
        T, seed = self._dropout_threshold(dropout), self._u64(seed, "seed")
        if offsets is not None and T:
            raise ValueError("offsets cannot be combined with dropout > 0: the dropout encoder produces no spans")
        return max_length, stride, pad, bos, eos, added

    def encode_batch_windows(self, texts: Sequence[str], max_length: int, stride: int = 0, *, pad_id: int | None = None,
                             bos_id: int | None = None, eos_id: int | None = None, padding_side: str = "right",
                             offsets: str | None = None, dropout: float = 0.0, seed: int = 0):
        """Rows of max_length ids in which a long text takes several rows (the stride / overflowing-tokens form)
        -> (rows, row_doc, row_start, lengths), with offsets "char" or "byte" also the spans of every slot.
        With C = max_length - n_added content slots a row and step = C - stride: row k = 0, 1, ... of text d holds
        [bos_id] + encode(texts[d])[k * step : k * step + C] + [eos_id], padded with pad_id to max_length at its right end
        (padding_side "left": at its left end); the last row is the first one with k * step + C >= n.  So every text, an empty
        one included, has at least one row -- 1 for n <= C, else 1 + ceil((n - C) / step) -- every row but a text's last is
        full, and consecutive rows of a text share exactly `stride` content ids.  Rows are in text order, in window order
        within a text.  row_doc[r] = the index into texts, row_start[r] = k * step (the index of the row's first content id in
        encode(texts[d])), lengths[r] = the row's length before padding, BOS / EOS included.
        offsets: a fifth result, offsets[r][c] = (start, end) of the slot's id as encode_with_offsets(texts[d], offsets) gives
        it, (0, 0) in BOS, EOS and pad slots.  dropout > 0 (not with offsets): the content ids are
        encode_batch_dropout(texts, dropout, seed)."""
        L, stride, pad, bos, eos, added = self._windows_args(max_length, stride, pad_id, bos_id, eos_id, padding_side, offsets, dropout, seed)
        if offsets is None:
            docs = [(ids, None) for ids in self._encode_batch_for_layout(texts, dropout, seed)]
        else:
            docs = self.encode_batch_with_offsets(texts, offsets)
        C = L - added
        step = C - stride
        rows, row_doc, row_start, lengths, spans = [], [], [], [], []
        for d, (ids, sp) in enumerate(docs):
            for s in range(0, len(ids) + step, step):  # (left by the break below: the first row that reaches the end)
                seq = ([bos] if bos is not None else []) + list(ids[s:s + C]) + ([eos] if eos is not None else [])
                fill = L - len(seq)
                rows.append(seq + [pad] * fill if padding_side == "right" else [pad] * fill + seq)
                row_doc.append(d)
                row_start.append(s)
                lengths.append(len(seq))
                if sp is not None:
                    seq_sp = [(0, 0)] * (bos is not None) + [tuple(p) for p in sp[s:s + C]] + [(0, 0)] * (eos is not None)
                    spans.append(seq_sp + [(0, 0)] * fill if padding_side == "right" else [(0, 0)] * fill + seq_sp)
                if s + C >= len(ids):
                    break
        out = (rows, row_doc, row_start, lengths)
        return out if offsets is None else out + (spans,)

    PAIR_TRUNCATIONS = ("longest_first", "only_first", "only_second", "windows")

    @staticmethod
    def _pair_texts(firsts, seconds) -> tuple[list[str], list[str]]:
        """the two sides as lists: sequences of str of equal length (one str is not a sequence of texts)"""
        sides = []
        for name, side in (("firsts", firsts), ("seconds", seconds)):
            if isinstance(side, (str, bytes, bytearray, memoryview)):
                raise ValueError(f"{name} must be a sequence of str, not one {type(side).__name__}")
            try:
                side = list(side)
            except TypeError:
                raise ValueError(f"{name} must be a sequence of str, not {side!r}") from None
            if not all(isinstance(t, str) for t in side):
                raise ValueError(f"{name} must hold str only")
            sides.append(side)
        if len(sides[0]) != len(sides[1]):
            raise ValueError(f"firsts and seconds must be equally long: {len(sides[0])} and {len(sides[1])} texts")
        return sides[0], sides[1]

    def _pairs_args(self, max_length, truncation, stride, sep_id, n_sep, pad_id, bos_id, eos_id, padding_side, offsets):
        """-> (max_length, stride, pad, bos, eos, sep or None, n_sep that counts, n_added)"""
        pad, bos, eos, added = self._layout_ids(pad_id, bos_id, eos_id)
        sep = None if sep_id is None else self._layout_ids(sep_id, None, None)[0]  # (validated as the other ids are)
        if isinstance(n_sep, bool) or n_sep not in (0, 1, 2):
            raise ValueError(f"n_sep must be 0, 1 or 2, not {n_sep!r}")
        n_sep = int(n_sep) if sep is not None else 0
        if n_sep == 0:
            sep = None
        added += n_sep
        if truncation not in self.PAIR_TRUNCATIONS:
            raise ValueError(f"truncation must be one of {self.PAIR_TRUNCATIONS}, not {truncation!r}")
        max_length = self._row_length(max_length, "max_length", added + 1)  # (at least one content slot a row)
        try:
            stride = operator.index(stride)
        except TypeError:
            raise ValueError(f"stride must be an integer, not {stride!r}") from None
        if truncation != "windows" and stride != 0:
            raise ValueError(f"stride must be 0 with truncation {truncation!r}: only 'windows' makes several rows of a pair")
        if not 0 <= stride < max_length - added:
            raise ValueError(f"stride must be in [0, {max_length - added - 1}] (max_length less the added ids and one), not {stride}")
        if padding_side not in ("left", "right"):
            raise ValueError(f"padding_side must be 'left' or 'right', not {padding_side!r}")
        if offsets not in (None, "char", "byte"):
            raise ValueError(f"offsets must be None, 'char' or 'byte', not {offsets!r}")
        return max_length, stride, pad, bos, eos, sep, n_sep, added

    def encode_batch_pairs(self, firsts: Sequence[str], seconds: Sequence[str], max_length: int, *, truncation: str = "longest_first",
                           stride: int = 0, sep_id: int | None = None, n_sep: int = 1, pad_id: int | None = None,
                           bos_id: int | None = None, eos_id: int | None = None, padding_side: str = "right",
                           offsets: str | None = None):
        """Two texts in one row (the text_pair form: question + context, query + passage)
        -> (rows, type_ids, row_pair, row_start, first_len, second_len), with offsets "char" or "byte" also the spans of every
        slot.  firsts and seconds are sequences of str of equal length.  With A = encode(firsts[p]), B = encode(seconds[p]), la
        and lb their lengths, n_added = (bos given) + (eos given) + n_sep (n_sep 0, 1 or 2; it counts only with a sep_id) and C
        = max_length - n_added >= 1 content slots, a row is [bos_id] + A[:ka] + [sep_id] * n_sep + B[s : s + kb] + [eos_id],
        padded with pad_id to max_length at its right end (padding_side "left": at its left end).  pad_id, bos_id, eos_id and
        sep_id as encode_batch_padded takes its ids.
        The truncation modes give one row per pair (row p is pair p, s = 0, stride must be 0); ids leave from the END of a side,
        every row fits and nothing raises because a side is too long:
          "longest_first"  while ka + kb > C: drop the last id of the longer side, of the second when both are equally long;
          "only_first"     the first gives up the excess la + lb - C, down to zero ids; a second alone longer than C is cut to C;
          "only_second"    the mirror image.
        "windows" (0 <= stride <= C - 1; the extractive-QA form): ka = min(la, C - stride - 1) in every row of the pair, and
        the second side is windowed as encode_batch_windows does with Cb = C - ka content slots and step = Cb - stride: row k has
        s = k * step and kb = min(Cb, lb - s), the last row is the first with s + Cb >= lb; every pair has at least one row.
        Rows are in pair order, in window order within a pair.
        type_ids[r][c] = 0 in BOS, the first side, the separators and padding, 1 in the second side and EOS.  row_pair[r] = the
        pair, row_start[r] = s, first_len[r] = ka, second_len[r] = kb (the length before padding is ka + kb + n_added).
        offsets: spans[r][c] = (start, end) of the slot's id IN ITS OWN TEXT, as encode_with_offsets gives it (type_ids says
        which text that is), (0, 0) in BOS, separator, EOS and pad slots.
        Out of scope: max_length=None, dropout, truncation from the left, windows over the first side."""
        L, stride, pad, bos, eos, sep, n_sep, added = self._pairs_args(max_length, truncation, stride, sep_id, n_sep, pad_id, bos_id, eos_id,
                                                                       padding_side, offsets)
        firsts, seconds = self._pair_texts(firsts, seconds)
        if offsets is None:
            sides = [[(ids, None) for ids in self.encode_batch(side)] for side in (firsts, seconds)]
        else:
            sides = [self.encode_batch_with_offsets(side, offsets) for side in (firsts, seconds)]
        C = L - added
        rows, types, row_pair, row_start, first_len, second_len, spans = [], [], [], [], [], [], []
        for p, ((A, spa), (B, spb)) in enumerate(zip(*sides)):
            la, lb = len(A), len(B)
            if truncation == "windows":
                ka = min(la, C - stride - 1)
                Cb = C - ka
                step = Cb - stride
                cuts = []
                for s in range(0, lb + step, step):  # (left by the break below: the first row that reaches the end)
                    cuts.append((s, min(Cb, lb - s)))
                    if s + Cb >= lb:
                        break
            else:
                ka, kb = la, lb
                if truncation == "longest_first":
                    while ka + kb > C:
                        if ka > kb:
                            ka -= 1
                        else:
                            kb -= 1
                else:
                    excess = max(0, la + lb - C)
                    if truncation == "only_first":
                        ka, kb = max(0, la - excess), min(lb, C)
                    else:
                        ka, kb = min(la, C), max(0, lb - excess)
                cuts = [(0, kb)]
            n_bos, n_eos = int(bos is not None), int(eos is not None)
            for s, kb in cuts:
                seq = [bos] * n_bos + list(A[:ka]) + [sep] * n_sep + list(B[s:s + kb]) + [eos] * n_eos
                typ = [0] * (n_bos + ka + n_sep) + [1] * (kb + n_eos)
                fill = L - len(seq)
                rows.append(seq + [pad] * fill if padding_side == "right" else [pad] * fill + seq)
                types.append(typ + [0] * fill if padding_side == "right" else [0] * fill + typ)
                row_pair.append(p)
                row_start.append(s)
                first_len.append(ka)
                second_len.append(kb)
                if offsets is not None:
                    seq_sp = ([(0, 0)] * n_bos + [tuple(x) for x in spa[:ka]] + [(0, 0)] * n_sep + [tuple(x) for x in spb[s:s + kb]]
                              + [(0, 0)] * n_eos)
                    spans.append(seq_sp + [(0, 0)] * fill if padding_side == "right" else [(0, 0)] * fill + seq_sp)
        out = (rows, types, row_pair, row_start, first_len, second_len)
        return out if offsets is None else out + (spans,)

    # ------------------------------------------------------------------ encode on the GPU (yabpe_encode; same ids as encode)
    def _device(self, model: str = "encode"):
        if self._device_ctx is None:
            from . import _native

            self._device_ctx = _native.Context()
            settings = BBPETrainerConfig(special_tokens=(), digit_group=self._digit_group, pretokenizer=self._pretokenizer)
            for name, value in device_options(settings).items():  # (read by every encode call of the context)
                self._device_ctx.set_option(name, value)
        if model not in self._device_models:
            if model == "encode":
                ordered = sorted(self._special_tokens, key=len, reverse=True)  # the split pattern's order
                self._device_ctx.encode_set_model(self._vocab, self._merges, ordered, self._vocab.get(b"[UNK]", 0))
            else:
                self._device_ctx.decode_set_model(self._vocab)
            self._device_models.add(model)
        return self._device_ctx

    @staticmethod
    def _device_input(texts):
        """-> (the documents' bytes back to back, their starts), or None for an empty sequence"""
        if isinstance(texts, (bytes, bytearray, memoryview)):
            return bytes(texts), [0]
        blobs = [t.encode("utf-8") for t in texts]
        if not blobs:
            return None
        starts = np.zeros(len(blobs), dtype=np.uint64)
        starts[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)[:-1]
        return b"".join(blobs), starts

    def _device_text(self, ctx, inp, errors: str = "strict"):
        """What the encode calls of ctx take as (text, n_bytes, doc_starts) for _device_input's buffer: the buffer itself, or what
        trainer.device_text_front makes of it, document by document, with errors = "replace" / "ignore", lowercase and the
        normaliser."""
        return device_text_front(ctx, np.frombuffer(inp[0], dtype=np.uint8), None, inp[1], repair=check_errors(errors),
                                 lower=self._lowercase, form=check_normalizer(self._normalizer))

    def normalize_array(self, texts, *, errors: str = "strict") -> tuple[np.ndarray, np.ndarray]:
        """normalize() of every document on the GPU: `texts` as encode_array takes them -> (text np.uint8[n], text_off
        np.uint64[n_docs + 1]): text[text_off[d]:text_off[d + 1]] is normalize(texts[d]) as UTF-8 -- the documents the spans of
        encode_array_with_offsets refer to.  Without a normaliser and without lowercase the documents come back as they are.  errors: as encode_array
        takes it -- the document is then normalize(data.decode("utf-8", errors)), the repaired and then normalised one."""
        inp = self._device_input(texts)
        if inp is None:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
        repair, form = check_errors(errors), check_normalizer(self._normalizer)
        if not form and not repair and not self._lowercase:
            return np.frombuffer(inp[0], dtype=np.uint8).copy(), np.append(np.asarray(inp[1], dtype=np.uint64), np.uint64(len(inp[0])))
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp, errors)
        if n_bytes is None:  # (nothing to do on the device, or nothing left)
            return np.ascontiguousarray(text).copy(), np.append(np.asarray(starts, dtype=np.uint64), np.uint64(len(text)))
        return ctx.d2h(text, n_bytes), np.append(np.asarray(starts, dtype=np.uint64), np.uint64(n_bytes))

    def encode_array(self, texts, *, errors: str = "strict") -> tuple[np.ndarray, np.ndarray]:
        """Encodes on the GPU: `texts` is a sequence of str (one document each) or one bytes buffer (one document).
        -> (ids np.uint32[n], doc_off np.uint64[n_docs + 1]): document d's ids are ids[doc_off[d]:doc_off[d + 1]], equal to
        encode(texts[d]).  Malformed UTF-8 in a bytes buffer raises _native.Utf8Error (.position = UnicodeDecodeError.start)
        under errors = "strict"; with "replace" or "ignore" the result is encode(data.decode("utf-8", errors)), repaired on the
        GPU (a str cannot hold ill-formed UTF-8, so the option only matters for a bytes buffer)."""
        inp = self._device_input(texts)
        if inp is None:
            check_errors(errors)
            return np.zeros(0, np.uint32), np.zeros(1, np.uint64)
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp, errors)
        return ctx.encode_to_host(text, n_bytes, doc_starts=starts)

    def encode_batch_device(self, texts: Sequence[str]) -> list[list[int]]:
        """encode_batch(texts), computed on the GPU in one call."""
        ids, off = self.encode_array(texts)
        ids, off = ids.tolist(), off.tolist()
        return [ids[off[d]:off[d + 1]] for d in range(len(off) - 1)]

    def encode_array_with_offsets(self, texts, unit: str = "char", *, errors: str = "strict") -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """encode_array(texts) plus every id's span, computed on the GPU in the same call.
        -> (ids np.uint32[n], doc_off np.uint64[n_docs + 1], offsets np.uint64[n, 2]): offsets[k] = (start, end) of id k in its
        own document, as encode_with_offsets(texts[d], unit) gives them.  errors: as encode_array takes it; the spans refer to
        the repaired, then normalised document, which normalize_array(texts, errors=errors) returns."""
        if unit not in ("char", "byte"):
            raise ValueError(f"unit must be 'char' or 'byte', not {unit!r}")
        inp = self._device_input(texts)
        if inp is None:
            check_errors(errors)
            return np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint64)
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp, errors)
        return ctx.encode_spans_to_host(text, n_bytes, doc_starts=starts, chars=unit == "char")

    def encode_batch_device_with_offsets(self, texts: Sequence[str], unit: str = "char"):
        """encode_batch_with_offsets(texts, unit), computed on the GPU in one call."""
        ids, off, spans = self.encode_array_with_offsets(texts, unit)
        ids, off, spans = ids.tolist(), off.tolist(), [tuple(p) for p in spans.tolist()]
        return [(ids[off[d]:off[d + 1]], spans[off[d]:off[d + 1]]) for d in range(len(off) - 1)]

    def encode_array_with_words(self, texts, *, errors: str = "strict") -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """encode_array(texts) plus the piece every id was made from, computed on the GPU in the same call (yabpe_encode_words).
        -> (ids np.uint32[n], doc_off np.uint64[n_docs + 1], words np.uint32[n], special bool[n]): words[k] and special[k] as
        encode_with_words(texts[d]) gives them for id k of document d.  errors: as encode_array takes it."""
        inp = self._device_input(texts)
        if inp is None:
            check_errors(errors)
            return np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, bool)
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp, errors)
        return ctx.encode_words_to_host(text, n_bytes, doc_starts=starts)

    def encode_batch_device_with_words(self, texts: Sequence[str]):
        """encode_batch_with_words(texts), computed on the GPU in one call."""
        ids, off, words, special = self.encode_array_with_words(texts)
        ids, off, words, special = ids.tolist(), off.tolist(), words.tolist(), special.tolist()
        return [(ids[off[d]:off[d + 1]], words[off[d]:off[d + 1]], special[off[d]:off[d + 1]]) for d in range(len(off) - 1)]

    def mask_array(self, ids, doc_off, words=None, special=None, *, mask_id: int | None = None, p: float = 0.15, seed: int = 0,
                   whole_word: bool = False, mask_fraction: float = 0.8, random_fraction: float = 0.1, n_random: int | None = None,
                   first_doc: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """mask_tokens on the GPU (yabpe_mask), bit for bit: ids, doc_off, words and special as encode_array_with_words returns
        them (words / special None: as mask_tokens without that batch) -> (inputs np.uint32[n], labels np.int32[n])."""
        mid, Ts, Tm, Tr, n_random, seed, first_doc = self._mask_args(mask_id, p, seed, whole_word, mask_fraction, random_fraction, n_random,
                                                                     first_doc, words is not None)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.asarray(doc_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0):
            raise ValueError("doc_off must be n_docs + 1 ascending offsets from 0 to len(ids)")
        packed = None
        if words is not None or special is not None:
            packed = np.zeros(len(ids), np.uint32) if words is None else np.array(words, dtype=np.uint32)
            if len(packed) != len(ids) or (special is not None and len(special) != len(ids)):
                raise ValueError("words and special must hold one entry per id")
            if np.any(packed >> 31):
                raise ValueError("a word index must be below 2^31")
            if special is not None:
                packed |= np.asarray(special, dtype=bool).astype(np.uint32) << 31
        from . import _native

        return self._device().mask_to_host(ids, None, off[:-1].astype(np.uint64), None, packed, seed=seed, first_doc=first_doc, select=Ts, mask=Tm,
                                           random=Tr, mask_id=mid, n_random=n_random, ignore=_native.MASK_IGNORE, whole_word=whole_word)

    def encode_array_masked(self, texts, max_length: int | None = None, *, mask_id: int | None = None, p: float = 0.15, seed: int = 0,
                            whole_word: bool = False, mask_fraction: float = 0.8, random_fraction: float = 0.1,
                            n_random: int | None = None, first_doc: int = 0, pad_id: int | None = None, bos_id: int | None = None,
                            eos_id: int | None = None, truncation: str = "right",
                            padding_side: str = "right") -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """encode_batch_masked(texts, ...), computed on the GPU: yabpe_encode_words, then yabpe_mask on its device results, then
        yabpe_layout_pad over the masked ids and, once those rows are copied out, over the labels with the ignore value as pad,
        BOS and EOS id (the ragged arrays never visit the host).  `texts` as encode_array takes them.
        -> (rows np.uint32[n_docs, L], labels np.int32[n_docs, L], lengths np.uint32[n_docs])."""
        L, pad, bos, eos, _added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        mid, Ts, Tm, Tr, n_random, seed, first_doc = self._mask_args(mask_id, p, seed, whole_word, mask_fraction, random_fraction, n_random,
                                                                     first_doc, True)
        inp = self._device_input(texts)
        n_docs = 0 if inp is None else len(inp[1])
        if inp is None or L == 0:  # (no rows, or rows of no slots: with BOS / EOS L is at least 1)
            return np.zeros((n_docs, L or 0), np.uint32), np.zeros((n_docs, L or 0), np.int32), np.zeros(n_docs, np.uint32)
        from . import _native

        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp)
        di, dd, dw, ni = ctx.encode_words(text, n_bytes, doc_starts=starts)
        mi, ml = ctx.mask(di, ni, dd, n_docs, dw, seed=seed, first_doc=first_doc, select=Ts, mask=Tm, random=Tr, mask_id=mid, n_random=n_random,
                          ignore=_native.MASK_IGNORE, whole_word=whole_word)
        cut = {"trunc_left": truncation == "left", "pad_left": padding_side == "left"}
        rows, lengths = ctx.layout_pad_to_host(mi, ni, dd, n_docs, row_len=L or 0, pad_id=pad, bos_id=bos, eos_id=eos, **cut)
        ign = _native.MASK_IGNORE
        if rows.shape[1] == 0:  # (only empty documents and neither BOS nor EOS)
            return rows, np.zeros(rows.shape, np.int32), lengths
        labels, _lengths = ctx.layout_pad_to_host(ml, ni, dd, n_docs, row_len=rows.shape[1], pad_id=ign, bos_id=None if bos is None else ign,
                                                  eos_id=None if eos is None else ign, **cut)
        return rows, labels.view(np.int32), lengths

    @staticmethod
    def _span_native_args(sent, To, C, seed, first_doc, cut, whole_word, final_sentinel) -> dict:
        return {"sentinels": np.asarray(sent, dtype=np.uint32), "seed": seed, "first_doc": first_doc, "open": To, "lens": C, "max_doc_ids": cut,
                "whole_word": whole_word, "final_sentinel": final_sentinel}

    def corrupt_spans_array(self, ids, doc_off, words=None, special=None, *, sentinels, p: float = 0.15, mean_span_length: float = 3.0,
                            max_span_length: int = 10, seed: int = 0, whole_word: bool = False, final_sentinel: bool = True,
                            max_tokens: int | None = None, first_doc: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """corrupt_spans on the GPU (yabpe_span_corrupt), bit for bit: ids, doc_off, words and special as
        encode_array_with_words returns them (words / special None: as corrupt_spans without that batch)
        -> (in_ids np.uint32[n_in], in_off np.uint64[n_docs + 1], tgt_ids np.uint32[n_tgt], tgt_off np.uint64[n_docs + 1]):
        document d's inputs are in_ids[in_off[d]:in_off[d + 1]], its targets tgt_ids[tgt_off[d]:tgt_off[d + 1]]."""
        sent, To, C, seed, first_doc, cut = self._span_args(sentinels, p, mean_span_length, max_span_length, seed, whole_word, final_sentinel,
                                                             max_tokens, first_doc, words is not None)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.asarray(doc_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0):
            raise ValueError("doc_off must be n_docs + 1 ascending offsets from 0 to len(ids)")
        packed = None
        if words is not None or special is not None:
            packed = np.zeros(len(ids), np.uint32) if words is None else np.array(words, dtype=np.uint32)
            if len(packed) != len(ids) or (special is not None and len(special) != len(ids)):
                raise ValueError("words and special must hold one entry per id")
            if np.any(packed >> 31):
                raise ValueError("a word index must be below 2^31")
            if special is not None:
                packed |= np.asarray(special, dtype=bool).astype(np.uint32) << 31
        return self._device().span_corrupt_to_host(ids, None, off[:-1].astype(np.uint64), None, packed,
                                                   **self._span_native_args(sent, To, C, seed, first_doc, cut, whole_word, final_sentinel))

    def encode_array_span_corrupted(self, texts, max_length: int | None = None, max_target_length: int | None = None, *, sentinels,
                                    p: float = 0.15, mean_span_length: float = 3.0, max_span_length: int = 10, seed: int = 0,
                                    whole_word: bool = False, final_sentinel: bool = True, max_tokens: int | None = None, first_doc: int = 0,
                                    pad_id: int | None = None, bos_id: int | None = None, eos_id: int | None = None,
                                    truncation: str = "right", padding_side: str = "right"):
        """encode_batch_span_corrupted(texts, ...), computed on the GPU: yabpe_encode_words, then yabpe_span_corrupt on its
        device results, then yabpe_layout_pad over the inputs and, once those rows are copied out, over the targets with the
        ignore value as pad, BOS and EOS id (the ragged arrays never visit the host).  `texts` as encode_array takes them.
        -> (rows np.uint32[n_docs, L], labels np.int32[n_docs, LT], lengths np.uint32[n_docs], label_lengths np.uint32[n_docs])."""
        L, pad, bos, eos, added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        LT = None if max_target_length is None else self._row_length(max_target_length, "max_target_length", added)
        sent, To, C, seed, first_doc, cut = self._span_args(sentinels, p, mean_span_length, max_span_length, seed, whole_word, final_sentinel,
                                                             max_tokens, first_doc, True)
        inp = self._device_input(texts)
        n_docs = 0 if inp is None else len(inp[1])

        def empty(width):
            return np.zeros((n_docs, width or 0), np.uint32), np.zeros(n_docs, np.uint32)

        if inp is None:
            return empty(L)[0], empty(LT)[0].view(np.int32), empty(L)[1], empty(LT)[1]
        from . import _native

        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp)
        di, dd, dw, ni = ctx.encode_words(text, n_bytes, doc_starts=starts)
        si, sio, n_in, st, sto, n_tgt, _nd = ctx.span_corrupt(di, ni, dd, n_docs, dw, **self._span_native_args(sent, To, C, seed, first_doc, cut,
                                                                                                            whole_word, final_sentinel))
        cut_kw = {"trunc_left": truncation == "left", "pad_left": padding_side == "left"}
        ign = _native.MASK_IGNORE
        # (rows of no slots -- asked for, or only empty sequences and neither BOS nor EOS -- need no layout call)
        rows, lengths = empty(L) if L == 0 else ctx.layout_pad_to_host(si, n_in, sio, n_docs, row_len=L or 0, pad_id=pad, bos_id=bos, eos_id=eos, **cut_kw)
        labels, label_lengths = empty(LT) if LT == 0 else ctx.layout_pad_to_host(st, n_tgt, sto, n_docs, row_len=LT or 0, pad_id=ign,
                                                                                 bos_id=None if bos is None else ign,
                                                                                 eos_id=None if eos is None else ign, **cut_kw)
        return rows, labels.view(np.int32), lengths, label_lengths

    @staticmethod
    def _fim_native_args(pre, suf, mid, eot, Tf, Ts, seed, first_doc, max_len, loss_middle) -> dict:
        from . import _native

        return {"seed": seed, "first_doc": first_doc, "fim": Tf, "spm": Ts, "pre_id": pre, "suf_id": suf, "mid_id": mid, "eot_id": eot,
                "ignore": _native.MASK_IGNORE, "max_len": max_len, "loss_middle": loss_middle}

    def fim_array(self, ids, doc_off, *, pre, suf, mid, eot=None, fim_rate: float = 0.5, spm_rate: float = 0.5, seed: int = 0, first_doc: int = 0,
                  max_length: int | None = None, loss: str = "all", cuts=None) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """fim_tokens on the GPU (yabpe_fim), bit for bit: ids and doc_off as encode_array returns them
        -> (seq_ids np.uint32[n_out], labels np.int32[n_out], off np.uint64[n_docs + 1], info np.uint32[n_docs, 4]): document
        d's sequence is seq_ids[off[d]:off[d + 1]].  cuts (np.uint64[n, 3], what fim_cuts_array returns as cuts): the
        documents are then the 3 n separately encoded pieces of n documents, three in a row each, and only the modes are read."""
        args = self._fim_args(pre, suf, mid, eot, fim_rate, spm_rate, seed, first_doc, max_length, loss)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.asarray(doc_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0):
            raise ValueError("doc_off must be n_docs + 1 ascending offsets from 0 to len(ids)")
        if cuts is not None:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            if cuts.size != len(off) - 1:
                raise ValueError(f"cuts must hold (mode, a, b) per document: {cuts.size} values for {len(off) - 1} pieces")
        return self._device().fim_to_host(ids, None, off[:-1].astype(np.uint64), None, cuts, pieces=cuts is not None, **self._fim_native_args(*args))

    def fim_cuts_array(self, texts, *, fim_rate: float = 0.5, spm_rate: float = 0.5, seed: int = 0, first_doc: int = 0,
                       errors: str = "strict") -> tuple[np.ndarray, np.ndarray]:
        """fim_cuts on the GPU (yabpe_fim_cuts behind the text front): `texts` as encode_array takes them
        -> (cuts np.uint64[n_docs, 3], piece_off np.uint64[n_docs, 3]): (mode, a, b) in code points of normalize(texts[d]), and
        the byte starts of (document, middle, suffix) in the normalised text that normalize_array returns."""
        Tf, Ts = self._dropout_threshold(fim_rate), self._dropout_threshold(spm_rate)
        seed, first_doc = self._u64(seed, "seed"), self._u64(first_doc, "first_doc")
        inp = self._device_input(texts)
        if inp is None:
            check_errors(errors)
            return np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint64)
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp, errors)
        piece_off, cuts = ctx.fim_cuts_to_host(text, n_bytes, starts, seed=seed, first_doc=first_doc, fim=Tf, spm=Ts)
        return cuts, piece_off

    def encode_array_fim(self, texts, max_length: int | None = None, *, level: str = "char", pre, suf, mid, eot=None, fim_rate: float = 0.5,
                         spm_rate: float = 0.5, seed: int = 0, first_doc: int = 0, loss: str = "all", pad_id: int | None = None,
                         bos_id: int | None = None, eos_id: int | None = None, truncation: str = "right", padding_side: str = "right"):
        """encode_batch_fim(texts, ...), computed on the GPU.  level "char": yabpe_fim_cuts on the device text, the 3 n piece
        starts copied to the host (24 bytes a document: yabpe_encode takes host starts), one yabpe_encode over the 3 n pieces,
        yabpe_fim with pieces; level "token": yabpe_encode, then yabpe_fim.  Then yabpe_layout_pad over the sequences and, once
        those rows are copied out, over the labels with the ignore value as pad, BOS and EOS id (the ragged arrays never visit
        the host).  `texts` as encode_array takes them.
        -> (rows np.uint32[n_docs, L], labels np.int32[n_docs, L], lengths np.uint32[n_docs], info np.uint32[n_docs, 4])."""
        (L, pad, bos, eos, _added), args = self._fim_row_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side, pre, suf, mid, eot,
                                                              fim_rate, spm_rate, seed, first_doc, loss)
        chars = self._fim_level(level)
        inp = self._device_input(texts)
        if inp is None:
            return np.zeros((0, L or 0), np.uint32), np.zeros((0, L or 0), np.int32), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint32)
        from . import _native

        ctx = self._device()
        n_docs = len(inp[1])
        native = self._fim_native_args(*args)
        text, n_bytes, starts = self._device_text(ctx, inp)
        if chars:
            dpo, dcuts, _nd = ctx.fim_cuts(text, n_bytes, starts, seed=native["seed"], first_doc=native["first_doc"], fim=native["fim"], spm=native["spm"])
            piece_off = ctx.d2h(dpo, 24 * n_docs, np.uint64)
            di, dd, ni = ctx.encode(text, n_bytes, doc_starts=piece_off)
            fi, fl, fo, fn, n_out, _nd = ctx.fim(di, ni, dd, 3 * n_docs, dcuts, pieces=True, **native)
        else:
            di, dd, ni = ctx.encode(text, n_bytes, doc_starts=starts)
            fi, fl, fo, fn, n_out, _nd = ctx.fim(di, ni, dd, n_docs, None, **native)
        info = ctx.d2h(fn, 16 * n_docs, np.uint32).reshape(n_docs, 4)
        cut = {"trunc_left": truncation == "left", "pad_left": padding_side == "left"}
        ign = _native.MASK_IGNORE
        rows, lengths = ctx.layout_pad_to_host(fi, n_out, fo, n_docs, row_len=L or 0, pad_id=pad, bos_id=bos, eos_id=eos, **cut)
        if rows.shape[1] == 0:  # (only empty sequences and neither BOS nor EOS)
            return rows, np.zeros(rows.shape, np.int32), lengths, info
        labels, _lengths = ctx.layout_pad_to_host(fl, n_out, fo, n_docs, row_len=rows.shape[1], pad_id=ign, bos_id=None if bos is None else ign,
                                                  eos_id=None if eos is None else ign, **cut)
        return rows, labels.view(np.int32), lengths, info

    def _device_encode_for_layout(self, ctx, inp, dropout=0.0, seed=0, offsets=None):
        """-> (ids pointer, document starts pointer, n_ids, spans): the device results the layout passes read -- yabpe_encode's,
        yabpe_encode_dropout's when dropout > 0, or with offsets ("char" / "byte") yabpe_encode_spans'.  spans: None without
        offsets, else the pointer, or the empty [0, 2] array when there are no ids."""
        T, seed = self._dropout_threshold(dropout), self._u64(seed, "seed")
        text, n_bytes, starts = self._device_text(ctx, inp)
        if offsets is not None:
            di, dd, ds, ni = ctx.encode_spans(text, n_bytes, doc_starts=starts, chars=offsets == "char")
            return di, dd, ni, ds or np.zeros((0, 2), np.uint64)
        if T == 0:
            return ctx.encode(text, n_bytes, doc_starts=starts) + (None,)
        return ctx.encode_dropout(text, T, seed, n_bytes, doc_starts=starts) + (None,)

    def encode_array_dropout(self, texts, p: float, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """encode_batch_dropout(texts, p, seed) on the GPU, id for id: `texts` and the results as encode_array's (one bytes
        buffer is document 0)."""
        T, seed = self._dropout_threshold(p), self._u64(seed, "seed")
        inp = self._device_input(texts)
        if inp is None:
            return np.zeros(0, np.uint32), np.zeros(1, np.uint64)
        ctx = self._device()
        text, n_bytes, starts = self._device_text(ctx, inp)
        return ctx.encode_dropout_to_host(text, T, seed, n_bytes, doc_starts=starts)

    def encode_batch_device_dropout(self, texts: Sequence[str], p: float, seed: int = 0) -> list[list[int]]:
        """encode_batch_dropout(texts, p, seed), computed on the GPU in one call."""
        ids, off = self.encode_array_dropout(texts, p, seed)
        ids, off = ids.tolist(), off.tolist()
        return [ids[off[d]:off[d + 1]] for d in range(len(off) - 1)]

    def encode_array_padded(self, texts, max_length: int | None = None, *, pad_id: int | None = None, bos_id: int | None = None,
                            eos_id: int | None = None, truncation: str = "right", padding_side: str = "right",
                            dropout: float = 0.0, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """encode_batch_padded(texts, ...), computed on the GPU: yabpe_encode (dropout > 0: yabpe_encode_dropout with
        this seed -- the form a training loop calls every epoch), then yabpe_layout_pad on its device results (the ragged ids
        never visit the host).  `texts` as encode_array takes them.
        -> (ids np.uint32[n_docs, L], lengths np.uint32[n_docs])."""
        L, pad, bos, eos, _added = self._padded_args(max_length, pad_id, bos_id, eos_id, truncation, padding_side)
        inp = self._device_input(texts)
        n_docs = 0 if inp is None else len(inp[1])
        if inp is None or L == 0:  # (no rows, or rows of no slots: with BOS / EOS L is at least 1)
            return np.zeros((n_docs, L or 0), np.uint32), np.zeros(n_docs, np.uint32)
        ctx = self._device()
        di, dd, ni, _spans = self._device_encode_for_layout(ctx, inp, dropout, seed)
        return ctx.layout_pad_to_host(di, ni, dd, n_docs, row_len=L or 0, pad_id=pad, bos_id=bos, eos_id=eos,
                                      trunc_left=truncation == "left", pad_left=padding_side == "left")

    def encode_array_packed(self, texts, seq_len: int, *, pad_id: int | None = None, bos_id: int | None = None,
                            eos_id: int | None = None, drop_last: bool = False, dropout: float = 0.0,
                            seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """encode_batch_packed(texts, ...), computed on the GPU: yabpe_encode (dropout > 0: yabpe_encode_dropout with
        this seed), then yabpe_layout_pack on its device results.  `texts` as encode_array takes them.
        -> (ids, doc, pos), each np.uint32[n_rows, seq_len]."""
        pad, bos, eos, _added = self._layout_ids(pad_id, bos_id, eos_id)
        seq_len = self._row_length(seq_len, "seq_len", 1)
        inp = self._device_input(texts)
        if inp is None:
            return tuple(np.zeros((0, seq_len), np.uint32) for _ in range(3))
        ctx = self._device()
        di, dd, ni, _spans = self._device_encode_for_layout(ctx, inp, dropout, seed)
        return ctx.layout_pack_to_host(di, ni, dd, len(inp[1]), row_len=seq_len, pad_id=pad, bos_id=bos, eos_id=eos, drop_last=drop_last)

    def encode_array_fit(self, texts, seq_len: int, *, pad_id: int | None = None, bos_id: int | None = None,
                         eos_id: int | None = None, dropout: float = 0.0,
                         seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """encode_batch_fit(texts, ...), computed on the GPU: yabpe_encode (dropout > 0: yabpe_encode_dropout with this seed),
        then yabpe_layout_fit on its device results.  `texts` as encode_array takes them.
        -> (ids, doc, pos: np.uint32[n_rows, seq_len] each, used np.uint32[n_rows])."""
        pad, bos, eos, added = self._layout_ids(pad_id, bos_id, eos_id)
        seq_len = self._row_length(seq_len, "seq_len", max(1, added))
        self._dropout_threshold(dropout), self._u64(seed, "seed")  # (refused before any device work)
        inp = self._device_input(texts)
        if inp is None:
            return tuple(np.zeros((0, seq_len), np.uint32) for _ in range(3)) + (np.zeros(0, np.uint32),)
        ctx = self._device()
        di, dd, ni, _spans = self._device_encode_for_layout(ctx, inp, dropout, seed)
        return ctx.layout_fit_to_host(di, ni, dd, len(inp[1]), row_len=seq_len, pad_id=pad, bos_id=bos, eos_id=eos)

    def encode_array_windows(self, texts, max_length: int, stride: int = 0, *, pad_id: int | None = None, bos_id: int | None = None,
                             eos_id: int | None = None, padding_side: str = "right", offsets: str | None = None,
                             dropout: float = 0.0, seed: int = 0):
        """encode_batch_windows(texts, ...), computed on the GPU: yabpe_encode (offsets: yabpe_encode_spans; dropout > 0:
        yabpe_encode_dropout with this seed), then yabpe_layout_windows on its device results.  `texts` as encode_array takes
        them.  -> (ids np.uint32[n_rows, max_length], row_doc, row_start, lengths: np.uint32[n_rows] each), with offsets also
        np.uint64[n_rows, max_length, 2] -- with a normaliser the spans refer to the normalised text, as
        encode_array_with_offsets' do."""
        L, stride, pad, bos, eos, _added = self._windows_args(max_length, stride, pad_id, bos_id, eos_id, padding_side, offsets, dropout, seed)
        inp = self._device_input(texts)
        if inp is None:
            out = (np.zeros((0, L), np.uint32),) + tuple(np.zeros(0, np.uint32) for _ in range(3))
            return out if offsets is None else out + (np.zeros((0, L, 2), np.uint64),)
        ctx = self._device()
        di, dd, ni, spans = self._device_encode_for_layout(ctx, inp, dropout, seed, offsets)
        return ctx.layout_windows_to_host(di, ni, dd, len(inp[1]), spans, row_len=L, stride=stride, pad_id=pad, bos_id=bos, eos_id=eos,
                                          pad_left=padding_side == "left")

    def encode_array_pairs(self, firsts: Sequence[str], seconds: Sequence[str], max_length: int, *, truncation: str = "longest_first",
                           stride: int = 0, sep_id: int | None = None, n_sep: int = 1, pad_id: int | None = None,
                           bos_id: int | None = None, eos_id: int | None = None, padding_side: str = "right",
                           offsets: str | None = None):
        """encode_batch_pairs(firsts, seconds, ...), computed on the GPU: ONE yabpe_encode call (offsets: yabpe_encode_spans)
        over the 2 n texts first, second, first, second, ..., then yabpe_layout_pairs on its device results (the ragged ids
        never visit the host).  -> (ids np.uint32[n_rows, max_length], type_ids np.uint8[n_rows, max_length], row_pair,
        row_start, first_len, second_len: np.uint32[n_rows] each), with offsets also np.uint64[n_rows, max_length, 2] -- with
        a normaliser the spans refer to the normalised texts, as encode_array_with_offsets' do."""
        L, stride, pad, bos, eos, sep, n_sep, _added = self._pairs_args(max_length, truncation, stride, sep_id, n_sep, pad_id, bos_id, eos_id,
                                                                        padding_side, offsets)
        firsts, seconds = self._pair_texts(firsts, seconds)
        inp = self._device_input([t for pair in zip(firsts, seconds) for t in pair])
        if inp is None:
            out = (np.zeros((0, L), np.uint32), np.zeros((0, L), np.uint8)) + tuple(np.zeros(0, np.uint32) for _ in range(4))
            return out if offsets is None else out + (np.zeros((0, L, 2), np.uint64),)
        ctx = self._device()
        di, dd, ni, spans = self._device_encode_for_layout(ctx, inp, offsets=offsets)
        return ctx.layout_pairs_to_host(di, ni, dd, len(inp[1]), spans, row_len=L, mode=truncation, stride=stride, sep_id=sep, n_sep=n_sep,
                                        pad_id=pad, bos_id=bos, eos_id=eos, pad_left=padding_side == "left")

    # ------------------------------------------------------------------ decode (tokenizer.py:324-349)
    def decode(self, ids: Sequence[int]) -> str:
        if not ids:
            return ""
        inv = self._vocab_inv
        data = b"".join(inv[i] for i in ids if i in inv)  # unknown ids are skipped
        try:
            return data.decode("utf-8")
        except UnicodeDecodeError:
            return data.decode("utf-8", errors="replace")

    def decode_batch(self, ids_batch: Sequence[Sequence[int]]) -> list[str]:
        return [self.decode(ids) for ids in ids_batch]

    # ------------------------------------------------------------------ decode on the GPU (yabpe_decode; same text as decode)
    def decode_array(self, ids, doc_off=None) -> tuple[np.ndarray, np.ndarray]:
        """Decodes on the GPU: document d = ids[doc_off[d]:doc_off[d + 1]] (encode_array's layout: n_docs + 1 offsets, the
        last one len(ids)); doc_off None: all of ids is one document.  -> (text np.uint8[n], text_off np.uint64[n_docs + 1]):
        text[text_off[d]:text_off[d + 1]] is decode(ids[doc_off[d]:doc_off[d + 1]]) as UTF-8."""
        if doc_off is None:
            doc_off = [0, len(ids)]
        off = np.asarray(doc_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0):
            raise ValueError("doc_off must be n_docs + 1 ascending offsets from 0 to len(ids)")
        arr = ids if isinstance(ids, np.ndarray) and ids.dtype == np.uint32 else _u32_ids(ids)
        if len(arr) != len(ids):  # ids no vocab can hold were dropped: move the document offsets with them
            keep = _u32_mask(ids)
            kept = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
            off = kept[off]
        return self._device("decode").decode_to_host(arr, doc_starts=off[:-1].astype(np.uint64))

    def decode_batch_device(self, ids_batch: Sequence[Sequence[int]]) -> list[str]:
        """decode_batch(ids_batch), computed on the GPU in one call."""
        if not len(ids_batch):
            return []
        flat = [i for ids in ids_batch for i in ids]
        off = np.zeros(len(ids_batch) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(ids) for ids in ids_batch])
        text, toff = self.decode_array(flat, off)
        data, toff = text.tobytes(), toff.tolist()
        return [data[toff[d]:toff[d + 1]].decode("utf-8") for d in range(len(ids_batch))]

    # ------------------------------------------------------------------ introspection
    @property
    def vocab_size(self) -> int:
        return len(self._vocab)

    @property
    def digit_group(self) -> int | None:
        return self._digit_group

    @property
    def pretokenizer(self) -> str:
        return self._pretokenizer

    @property
    def normalizer(self) -> str | None:
        return self._normalizer

    @property
    def lowercase(self) -> bool:
        return self._lowercase

    @property
    def special_tokens(self) -> list[str]:
        return list(self._special_tokens)

    def get_vocab(self) -> dict[str, int]:
        return {t.decode("latin-1"): i for t, i in self._vocab.items()}

    def clear_cache(self) -> None:
        self._word_ids.cache_clear()

    def cache_info(self) -> str:
        info = self._word_ids.cache_info()
        return f"hits={info.hits}, misses={info.misses}, size={info.currsize}/{info.maxsize}"


def _u32_mask(ids) -> np.ndarray:
    """Which ids lie in [0, 2^32) (Python ints of any size, or an integer array)."""
    try:
        a = np.asarray(ids, dtype=np.int64) if not isinstance(ids, np.ndarray) else ids
    except OverflowError:
        return np.fromiter((0 <= i < 1 << 32 for i in ids), dtype=bool, count=len(ids))
    if a.dtype.kind == "u":
        return a < (1 << 32)
    return (a >= 0) & (a < (1 << 32))


def _u32_ids(ids) -> np.ndarray:
    """ids as u32, without those outside [0, 2^32): no vocab the device can hold names them, and decode skips what its
    vocab does not name."""
    try:
        a = np.asarray(ids, dtype=np.int64) if not isinstance(ids, np.ndarray) else ids
    except OverflowError:
        return np.asarray([i for i in ids if 0 <= i < 1 << 32], dtype=np.uint32)
    return a[_u32_mask(a)].astype(np.uint32)
