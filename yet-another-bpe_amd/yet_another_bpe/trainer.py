"""Byte-level BPE trainer: host-side mirror of the reference interface over the MI355X HIP hot path.

Same names, arguments, defaults and error behaviour as DreamOneX/yet-another-bpe
`src/yet_another_bpe/trainer.py` (BBPETrainerConfig :17-38, BBPEModel :41-52, BBPETrainer :55-302);
the merge loop itself (:216-302) runs on the GPU through the C ABI in include/yabpe.h (libyabpe.so,
loaded with ctypes by `_native`).  There is no CPU fallback: without the built library and a GPU,
`_merge_loop` raises.

Host-only steps (file chunking, save format) stay in Python as in the reference.  Pre-tokenisation (UTF-8 decode +
GPT-2 regex, trainer.py:136-214; with BBPETrainerConfig(pretokenizer="cl100k") the GPT-4 / Llama-3 pattern, with "o200k_base"
the GPT-4o pattern) exists twice with
identical results: `_preprocess_corpus` runs the `regex` module on the host and returns Python lists, as the reference's
method does; on a corpus of 1 MiB or more (or with YABPE_PRETOKENIZE=gpu; YABPE_PRETOKENIZE=host forces the host path) the raw
file bytes go to `yabpe_pretokenize` instead and no Python object is built per pre-token.  With `batch_bytes` (or
YABPE_BATCH_BYTES) the device path reads the files batch by batch and pools each batch's pre-tokens into the context's word
pool (`yabpe_pool_add`), so neither the host nor the device ever holds more text than one batch; the merge loop is loaded
from the pool.

One route from the corpus to the loaded words, for `train` and `train_from` alike: `BBPETrainer._train` chooses host, device
or batched, `_device_words` reads file chunks `(path, start, stop)` with `read_chunks` and names the file of an invalid byte
with `utf8_error`, `_run` is the one tail (vocabulary, load -- the resumed load for a continued model --, merge loop, stats).
`device_options` is the one place a config field becomes an option of the library; the sharded drivers (distributed.py) and
BBPETokenizer's device context take theirs from it too.  `device_text_front` is the one chain of text passes in front of the
pre-tokeniser and the encoders (errors=, lowercase, normalizer): `_device_words`, the sharded driver and BBPETokenizer call it.
"""
from __future__ import annotations

import codecs
import json
import os
import threading
import unicodedata
from collections import Counter
from collections.abc import Mapping, Sequence
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import regex

# GPT-2 pre-tokenisation pattern (reference trainer.py:163)
_GPT2_SPLIT = r"""'(?:[sdmt]|ll|ve|re)| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""
# the split of cl100k_base (GPT-4), Llama-3 (G = 3) and Qwen2 (G = 1); %d: the digit group
_CL100K_SPLIT = r"""(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,%d}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"""
# the split of o200k_base (GPT-4o, o-series, gpt-oss): case-aware words that keep their contraction, "/" behind the newlines of
# a punctuation run; %d: the digit group
_O200K_SUFFIX = r"""(?i:'s|'t|'re|'ve|'m|'ll|'d)?"""
_O200K_SPLIT = (r"""[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+""" + _O200K_SUFFIX
                + r"""|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*""" + _O200K_SUFFIX
                + r"""|\p{N}{1,%d}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+""")
PRETOKENIZERS = ("gpt2", "cl100k", "o200k_base")
# name -> the library's option `split_pattern` (2 is reserved and refused by the library), and back
SPLIT_PATTERN_VALUES = {"gpt2": 0, "cl100k": 1, "o200k_base": 3}
PRETOKENIZER_NAMES = {v: k for k, v in SPLIT_PATTERN_VALUES.items()}
CL100K_DIGIT_GROUP = 3  # digit_group=None with the cl100k or the o200k_base pattern
# {"digit_group": G} (GPT-2 pattern with a group) or {"pattern": "cl100k" / "o200k_base", "digit_group": G}, written next to a
# saved model; the plain GPT-2 pattern writes no file
PRETOKENIZER_FILE = "pretokenizer.json"
# the normalisers: None, or "nfc" -- every chunk (training) and every document (encoding) is replaced by its Unicode NFC form
# (unicodedata.normalize("NFC", ...)) before anything else looks at it; pretokenizer.json gains "normalizer": "nfc"
NORMALIZERS = (None, "nfc")


def split_pattern(group: int | None = None, pretokenizer: str = "gpt2") -> str:
    """The one place the pattern string is built.  "gpt2": the GPT-2 pattern; with a digit group G, \\p{N}+ replaced by
    \\p{N}{1,G}.  "cl100k": the GPT-4 / Llama-3 pattern with \\p{N}{1,G} (None: 3).  "o200k_base": the GPT-4o pattern, likewise."""
    value = check_pretokenizer(pretokenizer)
    if value:
        return (_CL100K_SPLIT if value == 1 else _O200K_SPLIT) % (group or CL100K_DIGIT_GROUP)
    return _GPT2_SPLIT if not group else _GPT2_SPLIT.replace(r"\p{N}+", r"\p{N}{1,%d}" % group, 1)


def check_pretokenizer(name) -> int:
    """A pre-tokeniser name as the library's option `split_pattern` (0: "gpt2", 1: "cl100k", 3: "o200k_base").  ValueError for
    anything else."""
    if not isinstance(name, str) or name not in SPLIT_PATTERN_VALUES:
        raise ValueError(f"pretokenizer must be one of {PRETOKENIZERS!r}, got {name!r}")
    return SPLIT_PATTERN_VALUES[name]


def read_pretokenizer(model_dir: str | Path) -> tuple[str, int | None]:
    """(pretokenizer, digit_group) a saved model was trained with: pretokenizer.json in its directory; ("gpt2", None) when
    there is none."""
    f = Path(model_dir) / PRETOKENIZER_FILE
    if not f.exists():
        return "gpt2", None
    with open(f, encoding="utf-8") as fh:
        d = json.load(fh)
    name = d.get("pattern", "gpt2")
    group = check_digit_group(d.get("digit_group")) or None
    return name, (group or CL100K_DIGIT_GROUP) if check_pretokenizer(name) else group


def check_normalizer(name) -> int:
    """A normaliser name as the form argument of the library's yabpe_normalize (0: none, 1: "nfc").  ValueError for anything
    but None or "nfc"."""
    if name is None:
        return 0
    if not isinstance(name, str) or name != "nfc":
        raise ValueError(f"normalizer must be one of {NORMALIZERS!r}, got {name!r}")
    return 1


ERRORS = ("strict", "replace", "ignore")  # BBPETrainerConfig.errors; the index is the mode of the library's yabpe_utf8_repair


def check_errors(name) -> int:
    """An errors= name as the mode argument of the library's yabpe_utf8_repair (0: "strict", no repair; 1: "replace";
    2: "ignore").  ValueError for anything else."""
    if not isinstance(name, str) or name not in ERRORS:
        raise ValueError(f"errors must be one of {ERRORS!r}, got {name!r}")
    return ERRORS.index(name)


_DECODE_COUNT = threading.local()


def _counting_handler(replacement: str):
    def handler(e):
        _DECODE_COUNT.n = getattr(_DECODE_COUNT, "n", 0) + 1
        return replacement, e.end
    return handler


# bytes.decode's "replace" and "ignore" handlers, counting their calls (one per maximal subpart) per thread
codecs.register_error("yabpe_replace", _counting_handler("\ufffd"))
codecs.register_error("yabpe_ignore", _counting_handler(""))


def decode_counting(raw: bytes, errors: str) -> tuple[str, int]:
    """raw.decode("utf-8", errors) for errors = "replace" or "ignore", and the number of subparts replaced or dropped."""
    _DECODE_COUNT.n = 0
    text = raw.decode("utf-8", errors="yabpe_" + errors)
    return text, _DECODE_COUNT.n


def check_normalized_specials(tokens: Sequence[str], name) -> None:
    """With a normaliser the specials are matched in the normalised text, so a special that is not normalised itself could
    never match: ValueError."""
    if check_normalizer(name):
        for tok in tokens:
            if unicodedata.normalize("NFC", tok) != tok:
                raise ValueError(f"special token {tok!r} is not in NFC: with normalizer = 'nfc' it could never match the normalised text")


def normalize_text(text: str, name) -> str:
    """THE host-side normaliser: `text` as the normaliser `name` leaves it (None: as it is)."""
    return unicodedata.normalize("NFC", text) if name else text


def check_lowercase(flag) -> bool:
    """The lowercase setting: a bool and nothing else (1, "true" and None are a ValueError)."""
    if not isinstance(flag, bool):
        raise ValueError(f"lowercase must be True or False, got {flag!r}")
    return flag


def check_lowercase_specials(tokens: Sequence[str], flag) -> None:
    """With lowercase the specials are matched in the lowered text, so a special that is not lower case itself could never
    match: ValueError."""
    if check_lowercase(flag):
        for tok in tokens:
            if tok.lower() != tok:
                raise ValueError(f"special token {tok!r} is not lower case: with lowercase = True it could never match the lowered text "
                                 "(the default special_tokens [PAD], [UNK], [BOS], [EOS] are upper case: pass lower-case ones)")


def lowercase_text(text: str, flag) -> str:
    """THE host-side lower-casing: `text` as the setting leaves it (False: as it is).  It runs before normalize_text."""
    return text.lower() if flag else text


def device_text_front(ctx, text, n_bytes, starts, *, repair: int, lower: bool, form: int):
    """THE chain of text passes in front of yabpe_pretokenize and the encoders, part by part (a chunk in training, a document
    in encoding): with `repair` (check_errors) yabpe_utf8_repair, then with `lower` (check_lowercase) yabpe_lowercase, then with
    `form` (check_normalizer) yabpe_normalize.  `text`: a host u8 array (n_bytes None) or a device address; `starts`: the
    parts' starts in it.  -> (text, n_bytes, starts) as the next call takes them: the last pass's text in device memory (the
    context's until that pass's next call or its *_free; the words or ids made from it are offsets into it) and the parts'
    starts in it, read back after every pass; a text with nothing left is (an empty host array, None, starts).  The repair
    runs on an empty text too; the other two are skipped once no bytes are left.  _native.Utf8Error (the first pass that reads
    the text validates it: positions in the input) passes through; _native.SegmentTooLong leaves with .read_starts (the
    parts' starts in the text the normaliser read: repaired and lowered, so not the ones that came in) and .repaired (whether
    a repair ran in front of it)."""
    from . import _native

    n_parts = len(starts)
    if repair:
        text, dev_starts, n_bytes = ctx.utf8_repair(text, n_bytes=n_bytes, part_starts=starts, mode=repair)
        starts = ctx.d2h(dev_starts, 8 * n_parts, np.uint64)
    if lower and (n_bytes is None or n_bytes):
        text, dev_starts, n_bytes = ctx.lowercase(text, n_bytes=n_bytes, part_starts=starts)
        starts = ctx.d2h(dev_starts, 8 * n_parts, np.uint64)
    if form and (n_bytes is None or n_bytes):
        try:
            text, dev_starts, n_bytes = ctx.normalize(text, n_bytes=n_bytes, part_starts=starts, form=form)
        except _native.SegmentTooLong as e:
            e.read_starts, e.repaired = [int(s0) for s0 in starts], bool(repair)
            raise
        starts = ctx.d2h(dev_starts, 8 * n_parts, np.uint64)
    if n_bytes == 0:  # (every byte was dropped)
        text, n_bytes = np.zeros(0, np.uint8), None
    return text, n_bytes, starts


def read_lowercase(model_dir: str | Path) -> bool:
    """Whether a saved model was trained on lowered text: pretokenizer.json in its directory, False when it does not say."""
    f = Path(model_dir) / PRETOKENIZER_FILE
    if not f.exists():
        return False
    with open(f, encoding="utf-8") as fh:
        flag = json.load(fh).get("lowercase", False)
    return check_lowercase(flag)


def read_normalizer(model_dir: str | Path) -> str | None:
    """The normaliser a saved model was trained with: pretokenizer.json in its directory, None when it names none."""
    f = Path(model_dir) / PRETOKENIZER_FILE
    if not f.exists():
        return None
    with open(f, encoding="utf-8") as fh:
        name = json.load(fh).get("normalizer")
    check_normalizer(name)
    return name


def read_digit_group(model_dir: str | Path) -> int | None:
    """The digit group a saved model was trained with: pretokenizer.json in its directory, None when there is none."""
    return read_pretokenizer(model_dir)[1]


def check_digit_group(n) -> int:
    """A digit group as the library's option `digit_group` (0: none).  ValueError for anything but None or an integer from 1
    to 255; bool is not an integer here."""
    if n is None:
        return 0
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= 255:
        raise ValueError(f"digit_group must be None or an integer from 1 to 255, got {n!r}")
    return int(n)


@dataclass
class BBPETrainerConfig:
    """Configuration of a BBPE trainer (fields and defaults of reference trainer.py:31-38).

    Attributes:
        vocab_size: target vocabulary size, special tokens included.
        min_frequency: a pair is merged only while its count is at least this.
        max_workers: worker threads for file-chunk pre-tokenisation.
        chunk_size_bytes: logical chunk size when splitting large files.
        seed: unused (kept for compatibility, as in the reference).
        special_tokens: strings that get vocabulary ids right after the 256 bytes.
        max_token_length: longest token a merge may create, in BYTES (not in the reference; `max_token_length` of other BPE
            trainers, where one character of a byte-level alphabet is one byte).  None: no limit; an integer >= 2: at every
            step the best pair is taken among the pairs with len(left) + len(right) <= max_token_length, and training stops
            when none of those is left or the best of them is below min_frequency.  Special tokens are vocabulary entries,
            not merges, and may be longer; the merges of a model that train_from continues are replayed as they are.  The
            limit is NOT stored by save / save_lossless: a train_from that should keep it needs it in its own config.
        digit_group: None: the GPT-2 pattern as it is (a digit run of any length is one pre-token); an integer G from 1 to
            255: \\p{N}+ of the pattern becomes \\p{N}{1,G}, so a digit run is cut after every G characters, counted from its
            first digit (3: the digit rule of the GPT-4 / Llama-3 family, 1: single digits) and no learned token holds more
            than G digits.  Part of the model: train and train_from set BBPEModel.digit_group, save / save_lossless store it
            (pretokenizer.json) and BBPETokenizer reads it.  With a group no special token may begin with a \\p{N}
            character (ValueError): it could match at a group boundary, where the device rule never looks.
        pretokenizer: "gpt2" (the reference's pattern) or "cl100k": the split of GPT-4, Llama-3 and Qwen2 -- contractions in
            either case, one character that is no letter, digit, CR or LF in front of a letter run, digits in groups of
            digit_group (None: 3) without a space in front, newlines kept with the punctuation or the whitespace before
            them.  Part of the model like digit_group (BBPEModel.pretokenizer, pretokenizer.json, BBPETokenizer).  With
            "cl100k" no special token may begin with a \\s or a \\p{N} character (ValueError).  "o200k_base": the split of
            GPT-4o, the o-series and gpt-oss -- words cut where the case changes (HTTPServer, foo|Bar), the contraction kept
            with its word, "/" kept behind the newlines that follow punctuation; digit_group and the first character of a
            special as with "cl100k", and no special token may contain another one or end with the beginning of one, itself
            included (ValueError): their occurrences must not overlap.
        normalizer: None, or "nfc": every chunk _chunk_ranges cuts is replaced by unicodedata.normalize("NFC", chunk) before
            the special tokens and the split pattern see it (on the device: yabpe_normalize in front of yabpe_pretokenize);
            chunks are normalised independently.  What Qwen2's tokenizer does in front of the cl100k split.  Part of the
            model like the pattern (BBPEModel.normalizer, "normalizer" in pretokenizer.json, BBPETokenizer).  Specials are
            matched in the normalised text: a special token that is not NFC itself is a ValueError, and "<|endoftext|>"
            followed by U+0338 normalises to "<|endoftext|" + U+226F and is then no special.  A run of more than 16,384
            code points that normalise together (a base with its combining marks) is a ValueError that names the file.
        errors: "strict" (the reference: an invalid byte is a ValueError that names the file and the position), or "replace" /
            "ignore" as bytes.decode and open() take them: every chunk _chunk_ranges cuts is replaced by
            chunk.decode("utf-8", errors).encode() before the normaliser, the special tokens and the split pattern see it (on
            the device: yabpe_utf8_repair in front of yabpe_normalize / yabpe_pretokenize).  Chunks are repaired
            independently: a sequence cut off by a chunk's end is ill-formed there.  A property of how the files are read,
            NOT of the model: not stored by save / save_lossless, not carried by BBPEModel, not compared by train_from.
            BBPETrainer.utf8_replaced holds the number of subparts replaced or dropped by the last call.
        lowercase: False, or True: every chunk _chunk_ranges cuts is replaced by chunk.lower() (str.lower() of CPython: the full
            Unicode mapping with the final-sigma rule, no locale) after the repair of invalid UTF-8 and before the normaliser,
            the special tokens and the split pattern see it (on the device: yabpe_lowercase between yabpe_utf8_repair and
            yabpe_normalize); with normalizer = "nfc" a chunk becomes NFC(chunk.lower()).  Chunks are lowered independently:
            the final-sigma rule never looks across a chunk cut.  The front end of uncased models.  Part of the model like
            the normaliser (BBPEModel.lowercase, "lowercase" in pretokenizer.json, BBPETokenizer).  Specials are matched in
            the lowered text: a special token that is not lower case itself is a ValueError -- the default special_tokens
            are upper case, so lower-case ones must be passed.  Must be a bool.
    """

    vocab_size: int = 32000
    min_frequency: int = 2
    max_workers: int = 8
    chunk_size_bytes: int = 8 * 1024 * 1024
    seed: int = 42
    special_tokens: Sequence[str] = field(default_factory=lambda: ["[PAD]", "[UNK]", "[BOS]", "[EOS]"])
    max_token_length: int | None = None
    digit_group: int | None = None
    pretokenizer: str = "gpt2"
    normalizer: str | None = None
    errors: str = "strict"
    lowercase: bool = False


U16_TOKENS = 65_534  # tokens the u16 merge loop holds (ids 0 .. 65,533)
ID32_TOKENS = (1 << 24) - 2  # ... and the u32 one (ids 0 .. 2^24 - 3: the decode table's bound)


def id_bits_mode() -> str:
    """YABPE_ID_BITS: "auto" (the default: the u16 path while ids are left, then the u32 path), "16" (the u16 path only: a
    job that needs more ids ends in its capacity error) or "32" (the whole job on the u32 path)."""
    mode = os.environ.get("YABPE_ID_BITS", "auto").strip().lower() or "auto"
    if mode not in ("16", "32", "auto"):
        raise ValueError(f"YABPE_ID_BITS is {mode!r}: 16, 32 or auto")
    return mode


def stage1_merges(n_tokens: int, budget: int) -> int:
    """Merges to ask of the u16 path: as many as ids are left (a merge that reuses an id takes none, so the caller asks again
    while this is positive), at most the budget."""
    return max(0, min(int(budget), U16_TOKENS - int(n_tokens)))


def check_sharded_budget(vocab_size: int) -> None:
    """The multi-GPU drivers run the u16 merge loop only."""
    if int(vocab_size) > U16_TOKENS:
        raise ValueError(f"vocab_size = {vocab_size}: training on several GPUs holds at most {U16_TOKENS:,} tokens (u16 ids); "
                         "the u32 merge loop (id_bits = 32) is single-device")


def max_token_bytes(config: BBPETrainerConfig) -> int:
    """config.max_token_length as the library's option `max_token_bytes` (0: no limit).  ValueError for anything but None or
    an integer >= 2 (two single bytes must be able to merge); bool is not an integer here."""
    n = getattr(config, "max_token_length", None)
    if n is None:
        return 0
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 2:
        raise ValueError(f"max_token_length must be None or an integer >= 2 (bytes), got {n!r}")
    return int(n)


def pretokenizer(config: BBPETrainerConfig) -> tuple[int, int]:
    """config.pretokenizer and config.digit_group as the library's options (`split_pattern`, `digit_group`; 0: none), checked
    together with the special tokens: THE validation of the pre-tokeniser's settings."""
    pattern = check_pretokenizer(getattr(config, "pretokenizer", "gpt2"))
    group = check_digit_group(getattr(config, "digit_group", None))
    if pattern and not group:
        group = CL100K_DIGIT_GROUP
    if group:
        for tok in config.special_tokens:
            if regex.match(r"\p{N}", tok):
                raise ValueError(f"special token {tok!r} begins with a digit (\\p{{N}}): not allowed with digit_group = {group}")
    if pattern:
        for tok in config.special_tokens:
            if regex.match(r"\s", tok):
                raise ValueError(f"special token {tok!r} begins with whitespace (\\s): not allowed with pretokenizer = {PRETOKENIZER_NAMES[pattern]!r}")
    if pattern == 3:
        check_disjoint_specials(config.special_tokens)
    check_normalized_specials(config.special_tokens, getattr(config, "normalizer", None))
    check_lowercase_specials(config.special_tokens, getattr(config, "lowercase", False))
    return pattern, group


def check_disjoint_specials(tokens: Sequence[str]) -> None:
    """The o200k_base pattern takes a special wherever its scanner stands at a token boundary, so occurrences must never
    overlap: ValueError for a special that contains another one, or whose proper suffix begins a special (itself included).
    Equal specials are one special."""
    for a in tokens:
        for b in tokens:
            if a != b and b in a:
                raise ValueError(f"special token {a!r} contains special token {b!r}: not allowed with pretokenizer = 'o200k_base'")
            for k in range(1, min(len(a) - 1, len(b)) + 1):
                if a[len(a) - k:] == b[:k]:
                    raise ValueError(f"the end of special token {a!r} begins special token {b!r} ({b[:k]!r}): not allowed with pretokenizer = 'o200k_base'")


def digit_group(config: BBPETrainerConfig) -> int:
    """The digit group of pretokenizer(config): 0 for none; with "cl100k" or "o200k_base" never 0 (None means 3)."""
    return pretokenizer(config)[1]


class BBPEModel:
    """Result container (reference trainer.py:41-52): copies of vocab, merges, special tokens; digit_group (not in the
    reference): the digit group of the pre-tokenisation the model was trained with, None for the GPT-2 pattern; pretokenizer:
    "gpt2", or "cl100k" / "o200k_base" (digit_group is then never None); normalizer: None or "nfc"; lowercase: whether the text
    was lowered in front of the normaliser."""

    def __init__(self, vocab: Mapping[bytes, int], merges: Sequence[tuple[bytes, bytes]],
                 special_tokens: Sequence[str], digit_group: int | None = None, pretokenizer: str = "gpt2",
                 normalizer: str | None = None, lowercase: bool = False) -> None:
        self.vocab: dict[bytes, int] = dict(vocab)
        self.merges: list[tuple[bytes, bytes]] = list(merges)
        self.special_tokens: list[str] = list(special_tokens)
        self.pretokenizer: str = PRETOKENIZER_NAMES[check_pretokenizer(pretokenizer)]
        self.digit_group: int | None = check_digit_group(digit_group) or (CL100K_DIGIT_GROUP if self.pretokenizer != "gpt2" else None)
        self.normalizer: str | None = NORMALIZERS[check_normalizer(normalizer)]
        self.lowercase: bool = check_lowercase(lowercase)

    @classmethod
    def from_file_lossless(cls, model_dir: str | Path) -> "BBPEModel":
        """Loads what BBPETrainer.save_lossless wrote (vocab.hex.json, merges.hex, special_tokens.json): every token and
        merge exactly as trained -- the form BBPETrainer.train_from can continue from."""
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


def _utf8_cut(window: bytes, pos: int) -> int:
    """Largest cut <= pos inside `window` that is not in the middle of a UTF-8 sequence
    (continuation bytes are 10xxxxxx); mirrors find_utf8_boundary of reference trainer.py:139-144."""
    if pos >= len(window):
        return len(window)
    while pos > 0 and (window[pos] & 0xC0) == 0x80:
        pos -= 1
    return pos


def chunk_ranges(size: int, step: int, read) -> list[tuple[int, int]]:
    """The reference's chunk cuts (get_chunks, trainer.py:172-198) for `size` bytes that `read(offset, n) -> bytes` gives
    access to (a file, or text that lives on the device): a cut every `step` bytes, moved back to a UTF-8 boundary."""
    if size == 0:
        return []
    if size <= step:
        return [(0, size)]
    ranges: list[tuple[int, int]] = []
    start = 0
    while start < size:
        stop = min(start + step, size)
        if stop < size:  # back off to a UTF-8 boundary using a 5-byte window (trainer.py:183-190)
            w0 = max(0, stop - 4)
            window = read(w0, stop + 1 - w0)
            stop = w0 + _utf8_cut(window, stop - w0)
        if stop > start:
            ranges.append((start, stop))
            start = stop
        else:
            start += 1  # no progress possible: the reference skips one byte (trainer.py:196-197)
    return ranges


def group_chunks(sizes: Sequence[int], batch_bytes: int) -> list[tuple[int, int]]:
    """Consecutive chunks grouped into batches: [(first, end)] index ranges that cover range(len(sizes)) in order, each with
    at least one chunk and at most `batch_bytes` bytes -- except that a chunk larger than that is a batch by itself."""
    if batch_bytes <= 0:
        raise ValueError("batch_bytes must be positive")
    batches: list[tuple[int, int]] = []
    first, held = 0, 0
    for i, n in enumerate(sizes):
        if i > first and held + n > batch_bytes:
            batches.append((first, i))
            first, held = i, 0
        held += n
    if len(sizes) > first:
        batches.append((first, len(sizes)))
    return batches


def device_options(config: BBPETrainerConfig) -> dict[str, int]:
    """THE place a config field becomes an option of the library (yabpe_set_option): the non-zero ones among max_token_bytes,
    digit_group and split_pattern, validated.  The maximum token length is read at the load of the words, the digit group
    and the split pattern by every pre-tokenisation or encode call, so they go in right after the context is made."""
    limit = max_token_bytes(config)
    pattern, group = pretokenizer(config)
    check_errors(getattr(config, "errors", "strict"))
    return {k: v for k, v in (("max_token_bytes", limit), ("digit_group", group), ("split_pattern", pattern)) if v}


def check_files(paths: Sequence[Path]) -> None:
    for path in paths:
        if not path.exists():
            raise FileNotFoundError(f"File not found: {path}")


def read_chunks(chunks: Sequence[tuple[Path, int, int]]) -> tuple[np.ndarray, list[int]]:
    """The chunks (file, start, stop) read into one u8 buffer, back to back, and each chunk's start in it."""
    buf = np.empty(sum(stop - start for _p, start, stop in chunks), dtype=np.uint8)
    starts: list[int] = []
    pos = 0
    for path, start, stop in chunks:
        starts.append(pos)
        with open(path, "rb") as f:
            f.seek(start)
            if f.readinto(memoryview(buf[pos:pos + stop - start])) != stop - start:
                raise OSError(f"File {path} changed while it was read")
        pos += stop - start
    return buf, starts


def utf8_error(chunks: Sequence[tuple[Path, int, int]], starts: Sequence[int], e) -> ValueError:
    """The reference's message for e (a _native.Utf8Error with its position in read_chunks(chunks)' buffer): the file and the
    position in that file."""
    k = max(i for i, s0 in enumerate(starts) if s0 <= e.position)
    path, start, _stop = chunks[k]
    return ValueError(f"File {path} contains invalid UTF-8 at position {start + e.position - starts[k]}.")


def _segment_reason(e) -> str:
    """The library's words for a _native.SegmentTooLong without its position in the buffer the normaliser read: that buffer is
    the whole corpus, one batch or one rank's chunks, and the message must be the same on every route."""
    return regex.sub(r"^the segment that starts at byte \d+ holds", "it holds", str(e))


def segment_error(chunks: Sequence[tuple[Path, int, int]], starts: Sequence[int], e) -> ValueError:
    """The same for a _native.SegmentTooLong of the normaliser: the file and the position where the run starts (`starts`: the
    chunks' starts in the text the normaliser read)."""
    k = max(i for i, s0 in enumerate(starts) if s0 <= e.position)
    path, start, _stop = chunks[k]
    return ValueError(f"File {path} holds a run of code points that normalise together over the normaliser's cap at position "
                      f"{start + e.position - int(starts[k])}: {_segment_reason(e)}")


def repaired_segment_error(chunks: Sequence[tuple[Path, int, int]], starts: Sequence[int], e) -> ValueError:
    """The same after errors="replace" / "ignore": e's position is one in the REPAIRED text (`starts`: the chunks' starts in it),
    which no longer maps to a file position -- the file, the chunk's byte range and the position inside the repaired chunk."""
    k = max(i for i, s0 in enumerate(starts) if s0 <= e.position)
    path, start, stop = chunks[k]
    return ValueError(f"File {path} holds a run of code points that normalise together over the normaliser's cap in the chunk of bytes "
                      f"{start} to {stop}, at position {e.position - int(starts[k])} of that chunk after its invalid UTF-8 was repaired: {_segment_reason(e)}")


class BBPETrainer:
    """Byte-level BPE trainer with the reference's API; the merge loop runs on the GPU."""

    def __init__(self, config: BBPETrainerConfig | None = None) -> None:
        self.config: BBPETrainerConfig = config or BBPETrainerConfig()
        self._vocab: dict[bytes, int] = {}
        self._merges: list[tuple[bytes, bytes]] = []
        self.last_stats: dict | None = None  # yabpe_stats of the last merge loop (not in the reference)
        self.utf8_replaced: int = 0  # subparts of invalid UTF-8 replaced or dropped by the last train / train_from (0 under "strict")

    def _context(self):
        """A device context for this trainer's configuration."""
        from . import _native  # fails loudly when libyabpe.so / a GPU is missing

        ctx = _native.Context()
        try:
            for name, value in device_options(self.config).items():
                ctx.set_option(name, value)
        except BaseException:
            ctx.close()
            raise
        return ctx

    def _model(self, vocab, merges) -> BBPEModel:
        pattern, group = pretokenizer(self.config)
        return BBPEModel(vocab=vocab, merges=merges, special_tokens=list(self.config.special_tokens), digit_group=group or None,
                         pretokenizer=PRETOKENIZER_NAMES[pattern], normalizer=getattr(self.config, "normalizer", None),
                         lowercase=getattr(self.config, "lowercase", False))

    # ------------------------------------------------------------------ train / save (trainer.py:63-117)
    def train(self, files: Sequence[str | Path], batch_bytes: int | None = None) -> BBPEModel:
        """`batch_bytes` (None: the environment variable YABPE_BATCH_BYTES; unset: everything at once): the files go through
        the device pre-tokeniser in batches of whole chunks of at most that many bytes and their pre-tokens are pooled on
        the device batch by batch -- for corpora larger than host or device memory.  The model is the same.
        An empty corpus gives the base vocabulary only (trainer.py:81-85); so does a zero budget, after the text was
        pre-tokenised (an invalid byte is still reported)."""
        device_options(self.config)  # (a bad limit, pre-tokeniser or digit group, or a special they do not allow, fails before any file is read or any device call is made)
        if not files:
            raise ValueError("At least one file must be provided")
        paths = [Path(f) if isinstance(f, str) else f for f in files]
        return self._train(paths, batch_bytes, self._base_tokens(), None, [], self._init_base_vocab())

    def train_from(self, model, files: Sequence[str | Path], batch_bytes: int | None = None) -> BBPEModel:
        """Continues training from `model` (a BBPEModel, or anything with .vocab, .merges and .special_tokens) on `files`:
        more merges on the same corpus, or new merges learned from a new one.  Every existing id is kept; the result is
        model.merges + the new merges and the extended vocab, exactly what train() gives when the corpus is the one the
        model was trained on.  The iteration budget is max(0, vocab_size - len(base) - len(model.merges)) (a merge that
        reused an id cost an iteration too, trainer.py:238).  An empty corpus or a zero budget returns the model unchanged.
        Pre-tokenisation is train()'s (special tokens are ordinary words), on the device under the same size / environment
        rule; the words are pooled (the flat layout does not apply).  `batch_bytes`: as train() takes it.
        config.max_token_length constrains only the merges learned here: the model's own merges are replayed whatever their
        length (the limit is not part of a saved model)."""
        device_options(self.config)  # (as in train)
        if not files:
            raise ValueError("At least one file must be provided")
        paths = [Path(f) if isinstance(f, str) else f for f in files]
        pattern, group = pretokenizer(self.config)
        if getattr(model, "pretokenizer", "gpt2") != PRETOKENIZER_NAMES[pattern]:
            raise ValueError(f"cannot continue from this model: it was trained with pretokenizer = {getattr(model, 'pretokenizer', 'gpt2')!r}, "
                             f"the trainer's is {PRETOKENIZER_NAMES[pattern]!r} (its merges would be replayed over words it never saw)")
        if getattr(model, "digit_group", None) != (group or None):
            raise ValueError(f"cannot continue from this model: it was trained with digit_group = {getattr(model, 'digit_group', None)!r}, "
                             f"the trainer's is {group or None!r} (its merges would be replayed over words it never saw)")
        if getattr(model, "normalizer", None) != getattr(self.config, "normalizer", None):
            raise ValueError(f"cannot continue from this model: it was trained with normalizer = {getattr(model, 'normalizer', None)!r}, "
                             f"the trainer's is {getattr(self.config, 'normalizer', None)!r} (its merges would be replayed over words it never saw)")
        if getattr(model, "lowercase", False) != getattr(self.config, "lowercase", False):
            raise ValueError(f"cannot continue from this model: it was trained with lowercase = {getattr(model, 'lowercase', False)!r}, "
                             f"the trainer's is {getattr(self.config, 'lowercase', False)!r} (its merges would be replayed over words it never saw)")
        toks, triples = self._resumable(model)
        old_merges = [(bytes(l), bytes(r)) for l, r in model.merges]
        check_files(paths)
        if self._budget(old_merges) == 0:  # nothing to learn: no file is read, whatever batch_bytes says
            self._vocab, self._merges, self.utf8_replaced = dict(model.vocab), old_merges, 0
            return self._model(self._vocab, self._merges)
        return self._train(paths, batch_bytes, toks, triples, old_merges, dict(model.vocab))

    def _budget(self, old_merges: Sequence = ()) -> int:
        """Iterations of the merge loop that the vocabulary size leaves (trainer.py:238)"""
        return max(0, self.config.vocab_size - len(self._base_tokens()) - len(old_merges))

    def _train(self, paths: Sequence[Path], batch_bytes: int | None, toks: list[bytes], triples, old_merges: list, unchanged: dict) -> BBPEModel:
        """train and train_from: `toks` the tokens in id order and `triples` the merges that made them (_resumable; None: a
        fresh model over the base tokens), `old_merges` those merges as bytes, `unchanged` the vocabulary to return when the
        corpus has no words.  The ONE place the route is chosen -- pre-tokeniser on the host, on the device
        (YABPE_PRETOKENIZE=gpu, or auto and 1 MiB of files or more), or on the device batch by batch through the word pool
        -- and the words are handed to _run in one of its two forms.  Same results on every route.  YABPE_LAYOUT=flat (every
        occurrence resident, no pooling) applies to a fresh model only: a continued one always pools."""
        flat = triples is None and os.environ.get("YABPE_LAYOUT", "dedup") == "flat"
        mode = os.environ.get("YABPE_PRETOKENIZE", "auto")
        self.utf8_replaced = 0
        batch = self._batch_bytes(batch_bytes)
        if batch is not None and flat:
            raise ValueError("batch_bytes needs the pooled layout: YABPE_LAYOUT=flat keeps every occurrence resident")
        check_files(paths)
        num_merges = self._budget(old_merges)
        vocab, new_merges = unchanged, []
        if batch is not None or mode == "gpu" or (mode == "auto" and sum(p.stat().st_size for p in paths) >= (1 << 20)):
            chunks = [(path, start, stop) for path in paths for start, stop in self._chunk_ranges(path)]
            if chunks:
                with self._context() as ctx:
                    words = self._device_words(ctx, chunks, batch, dedup=not flat)
                    if words[2] and num_merges:
                        vocab, new_merges = self._run(ctx, toks, words, triples, num_merges)
        else:
            pretokens = self._pretokenize(paths)
            if flat:
                words, freq = [t.encode("utf-8") for t in pretokens], None
            else:  # word-frequency pooling (trainer.py:221-225) on the host: the pre-tokens are Python strings here anyway
                pooled = Counter(pretokens)
                words, freq = [t.encode("utf-8") for t in pooled], np.fromiter(pooled.values(), dtype=np.uint64, count=len(pooled))
            if words and num_merges:
                with self._context() as ctx:
                    vocab, new_merges = self._run(ctx, toks, self._host_words(words, freq), triples, num_merges)
        self._vocab, self._merges = vocab, old_merges + new_merges
        return self._model(self._vocab, self._merges)

    @staticmethod
    def _batch_bytes(batch_bytes: int | None) -> int | None:
        if batch_bytes is None:
            env = os.environ.get("YABPE_BATCH_BYTES", "")
            if not env:
                return None
            batch_bytes = int(env)
        if int(batch_bytes) <= 0:
            raise ValueError("batch_bytes must be positive")
        if os.environ.get("YABPE_PRETOKENIZE", "auto") == "host":
            raise ValueError("batch_bytes needs the device pre-tokeniser (YABPE_PRETOKENIZE=host is set)")
        return int(batch_bytes)

    def _device_words(self, ctx, chunks: Sequence[tuple[Path, int, int]], batch_bytes: int | None, dedup: bool):
        """The chunks' pre-tokens as device words for _run: file bytes -> device_text_front, chunk by chunk -> yabpe_pretokenize
        -> word offsets in HBM (equal pre-tokens are pooled by the load when `dedup`).  With `batch_bytes` the chunks are
        read batch by batch (one batch on the host at a time) and each batch's pre-tokens added to ctx's word pool
        (yabpe_pool_add); the words are then the pool's, with its counts and nothing left to pool.  Pre-tokens never cross a
        chunk cut, so the pooled multiset is the same."""
        from . import _native

        form = check_normalizer(getattr(self.config, "normalizer", None))
        repair = check_errors(getattr(self.config, "errors", "strict"))
        lower = check_lowercase(getattr(self.config, "lowercase", False))

        def pretokenize(part):
            buf, starts = read_chunks(part)
            try:
                text, n_bytes, cur = device_text_front(ctx, buf, None, starts, repair=repair, lower=lower, form=form)
                if repair:
                    self.utf8_replaced += int(ctx.utf8_repair_stats()["n_subparts"])
                return ctx.pretokenize(text, n_bytes=n_bytes, chunk_starts=cur, special_tokens=list(self.config.special_tokens))
            except _native.Utf8Error as e:  # (positions in buf)
                raise utf8_error(part, starts, e) from e
            except _native.SegmentTooLong as e:
                # (a position in the text the normaliser read.  Lowered text: the chunk is the right one, the position inside it
                # counts the lowered bytes -- the file's, give or take what the 25 code points that change length did in front
                # of it)
                raise (repaired_segment_error if e.repaired else segment_error)(part, e.read_starts, e) from e

        if batch_bytes is None:
            return (*pretokenize(chunks), 0, dedup)
        for first, end in group_chunks([stop - start for _p, start, stop in chunks], batch_bytes):
            ctx.pool_add_ptr(*pretokenize(chunks[first:end]))
            ctx.pretokenize_free()
            if form:
                ctx.normalize_free()
            if lower:
                ctx.lowercase_free()
            if repair:
                ctx.utf8_repair_free()
        dev_bytes, dev_off, dev_freq, n_unique, _n_bytes = ctx.pool_get()
        return dev_bytes, dev_off, n_unique, dev_freq, False

    def _load(self, ctx, toks: list[bytes], words, triples, pooled: bool = False) -> None:
        """set_vocab + the load of `words` on ctx: host arrays (flat, off, freq) or device words (bytes address, offsets
        address, n, counts address or 0, dedup); with `triples` the resumed load.  pooled: equal words are pooled even where
        the words come without counts and without `dedup` (the u32 path's resumed load needs it)."""
        ctx.set_vocab(toks)
        if len(words) == 3:
            dedup = pooled and words[2] is None
            if triples is None:
                ctx.load_words(*words, dedup=dedup)
            else:
                ctx.load_words_resumed(*words, triples, dedup=dedup)
        else:
            dev_bytes, dev_off, n_words, dev_freq, dedup = words
            dedup = dedup or (pooled and not dev_freq)
            if triples is None:
                ctx.load_words_ptr(dev_bytes, dev_off, n_words, freq_ptr=dev_freq, dedup=dedup)
            else:
                ctx.load_words_resumed_ptr(dev_bytes, dev_off, n_words, triples, freq_ptr=dev_freq, dedup=dedup)

    def _run(self, ctx, toks: list[bytes], words, triples, num_merges: int):
        """The merge loop on ctx, from `toks` (with `triples`: the merges that made them, replayed by the load) over `words`:
        host arrays (flat, off, freq) or device words (bytes address, offsets address, n, counts address or 0, dedup) -- with
        counts they are the context's pool, which is cleared once the last load has copied what it needs.  -> (vocab, merges)
        The ONE place the id width is chosen (YABPE_ID_BITS, id_bits_mode): a budget that fits in 65,534 ids runs as it always
        did.  A larger one runs on the u16 path while ids are left (stage 1: stage1_merges per yabpe_train call, again after
        merges that reused an id; a call that returns fewer merges than asked hit a stop rule and ends the job), then the same
        words are loaded into a second context with id_bits = 32 through the resumed load, which replays every merge so far,
        and the u32 path runs the rest (stage 2).  last_stats says what each stage did."""
        mode = id_bits_mode()
        min_frequency = max(0, int(self.config.min_frequency))  # (<= 0: merge to exhaustion, as the reference does)
        is_pool = len(words) == 5 and bool(words[3])
        if mode == "16" or (mode == "auto" and len(toks) + num_merges <= U16_TOKENS):
            self._load(ctx, toks, words, triples)
            if is_pool:
                ctx.pool_clear()
            left, right, merged, _count = ctx.train(num_merges, min_frequency)
            self.last_stats = ctx.stats()
            return self._decode_merges(toks, left, right, merged)
        base = list(toks)
        done = [np.asarray(x, dtype=np.uint32) for x in (triples if triples is not None else ((), (), ()))]
        n_tokens, n_done, stages, stopped = len(toks), 0, 0, False
        if mode == "auto" and stage1_merges(n_tokens, num_merges) > 0:
            self._load(ctx, base, words, triples)
            while not stopped and stage1_merges(n_tokens, num_merges - n_done) > 0:
                ask = stage1_merges(n_tokens, num_merges - n_done)
                left, right, merged, _count = ctx.train(ask, min_frequency)
                done = [np.concatenate([d, np.asarray(x, dtype=np.uint32)]) for d, x in zip(done, (left, right, merged))]
                n_tokens += len({int(m) for m in merged.tolist() if m >= n_tokens})  # (fresh ids; a reused id takes none)
                n_done += len(left)
                stages += 1
                stopped = len(left) < ask
        stats16 = ctx.stats() if stages else None
        stats = {"id16_merges": n_done, "id16_stages": stages, "id32_merges": 0, "id32_replayed_merges": 0, "id32_load_ms": 0.0,
                 "id16_train_ms": stats16["train_ms"] if stats16 else 0.0}
        if not stopped and n_done < num_merges:
            # stage 2: every token so far, the words again (pooled), all merges replayed by rank
            all_toks = self._decode_tokens(base, done, len(triples[0]) if triples is not None else 0)
            replay = tuple(done) if len(done[0]) else None
            ctx32 = ctx if not stages else self._context()
            try:
                ctx32.set_option("id_bits", 32)
                self._load(ctx32, all_toks, words, replay, pooled=True)
                if is_pool:
                    ctx.pool_clear()
                rs = ctx32.resume_stats()
                left, right, merged, _count = ctx32.train(num_merges - n_done, min_frequency)
                done = [np.concatenate([d, np.asarray(x, dtype=np.uint32)]) for d, x in zip(done, (left, right, merged))]
                stats.update(ctx32.stats())
                stats.update(id32_merges=len(left), id32_replayed_merges=0 if replay is None else len(replay[0]),
                             id32_load_ms=rs["segment_ms"] + rs["build_ms"])
            finally:
                if ctx32 is not ctx:
                    ctx32.close()
        else:
            if is_pool:
                ctx.pool_clear()
            stats = {**stats16, **stats}
        self.last_stats = stats
        skip = len(triples[0]) if triples is not None else 0
        return self._decode_merges_from(base, done, skip)

    @staticmethod
    def _decode_tokens(base: Sequence[bytes], triples, n_old: int) -> list[bytes]:
        """The tokens in id order after `triples` ((left, right, merged) arrays; the first n_old made `base` itself)"""
        toks = list(base)
        for l, r, m in zip(triples[0][n_old:].tolist(), triples[1][n_old:].tolist(), triples[2][n_old:].tolist()):
            if m == len(toks):
                toks.append(toks[l] + toks[r])
        return toks

    @staticmethod
    def _decode_merges_from(base: Sequence[bytes], triples, n_old: int):
        """(vocab, the merges after the first n_old) of `triples` over `base` (the tokens the first n_old merges made)"""
        from ._native import decode_merges

        return decode_merges(base, triples[0][n_old:], triples[1][n_old:], triples[2][n_old:])

    # ------------------------------------------------------------------ continuing from a trained model
    def _resumable(self, model) -> tuple[list[bytes], tuple]:
        """Checks that `model` is what this trainer's configuration would have produced -- replaying its merges over
        _base_tokens() as _decode_merges does gives model.vocab exactly, and the special tokens are the configured ones --
        and returns (tokens in id order, the merges as (left, right, merged) id arrays).  ValueError otherwise."""
        from ._native import merge_triples

        vocab, merges = dict(model.vocab), list(model.merges)
        if list(model.special_tokens) != list(self.config.special_tokens):
            raise ValueError(f"cannot continue from this model: its special tokens {list(model.special_tokens)!r} are not the "
                             f"trainer's {list(self.config.special_tokens)!r}")
        if sorted(vocab.values()) != list(range(len(vocab))):
            raise ValueError("cannot continue from this model: its token ids are not dense (0 .. len(vocab) - 1, each once)")
        hint = ("; a model reloaded in the reference's text format (from_file) has lost merges and tokens -- save it with "
                "save_lossless and reload it with from_file_lossless")
        try:
            toks, triples = merge_triples(self._base_tokens(), merges)
        except ValueError as e:
            raise ValueError(f"cannot continue from this model: {e}{hint}") from None
        if {t: i for i, t in enumerate(toks)} != vocab:
            raise ValueError("cannot continue from this model: replaying its merges over the trainer's base vocabulary does not "
                             f"reproduce its vocab ({len(toks)} tokens replayed, {len(vocab)} in the model){hint}")
        return toks, triples

    @staticmethod
    def _decode_merges(base: Sequence[bytes], left, right, merged):
        from ._native import decode_merges

        return decode_merges(base, left, right, merged)

    def save(self, output_dir: str | Path) -> None:
        """vocab.json / merges.txt / special_tokens.json in the reference's format (trainer.py:94-117); with a digit group
        also pretokenizer.json ({"digit_group": G}), with another pattern {"pattern": "cl100k" or "o200k_base", "digit_group": G}."""
        if not self._vocab:
            raise ValueError("Model has not been trained yet. Call train() first.")
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "vocab.json", "w", encoding="utf-8") as f:
            json.dump({tok.decode("latin-1"): idx for tok, idx in self._vocab.items()}, f, ensure_ascii=False, indent=2)
        with open(out / "merges.txt", "w", encoding="utf-8") as f:
            for left, right in self._merges:
                f.write(f"{left.decode('latin-1')} {right.decode('latin-1')}\n")
        with open(out / "special_tokens.json", "w", encoding="utf-8") as f:
            json.dump(list(self.config.special_tokens), f, ensure_ascii=False, indent=2)
        self._save_pretokenizer(out)

    def _save_pretokenizer(self, out: Path) -> None:
        """pretokenizer.json, only when the model was trained with a digit group, another pattern than GPT-2's, a normaliser or
        lowercase (without them the directory holds exactly the files it always held; a file left there by an earlier save
        is removed).  "normalizer" is written only when one is set, "lowercase" only when it is."""
        pattern, group = pretokenizer(self.config)
        d = {"pattern": PRETOKENIZER_NAMES[pattern], "digit_group": group} if pattern else {"digit_group": group} if group else {}
        if getattr(self.config, "normalizer", None):
            d["normalizer"] = self.config.normalizer
        if check_lowercase(getattr(self.config, "lowercase", False)):
            d["lowercase"] = True
        if d:
            with open(out / PRETOKENIZER_FILE, "w", encoding="utf-8") as f:
                json.dump(d, f)
        elif (out / PRETOKENIZER_FILE).exists():
            (out / PRETOKENIZER_FILE).unlink()

    def save_lossless(self, output_dir: str | Path) -> None:
        """The same model in a format that survives a reload byte for byte: `vocab.hex.json` ({token hex: id}),
        `merges.hex` (one `left_hex right_hex` line per merge, the serialisation of the golden files) and
        special_tokens.json.  The reference's own format (save()) loses every merge whose LEFT token contains a space --
        its loader splits each line at the first space (tokenizer.py:137) -- and every token with a line break; it is kept
        as it is for compatibility, this one is offered next to it (BBPETokenizer.from_file_lossless)."""
        if not self._vocab:
            raise ValueError("Model has not been trained yet. Call train() first.")
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "vocab.hex.json", "w", encoding="ascii") as f:
            json.dump({tok.hex(): idx for tok, idx in self._vocab.items()}, f, indent=0)
        with open(out / "merges.hex", "w", encoding="ascii") as f:
            for left, right in self._merges:
                f.write(f"{left.hex()} {right.hex()}\n")
        with open(out / "special_tokens.json", "w", encoding="utf-8") as f:
            json.dump(list(self.config.special_tokens), f, ensure_ascii=False, indent=2)
        self._save_pretokenizer(out)

    # ------------------------------------------------------------------ base vocab (trainer.py:119-134)
    def _base_tokens(self) -> list[bytes]:
        toks = [bytes([b]) for b in range(256)]
        seen = set(toks)
        for s in self.config.special_tokens:
            tb = s.encode("utf-8")
            if tb not in seen:  # a special whose bytes already exist gets no id (trainer.py:130)
                seen.add(tb)
                toks.append(tb)
        return toks

    def _init_base_vocab(self) -> dict[bytes, int]:
        return {t: i for i, t in enumerate(self._base_tokens())}

    # ------------------------------------------------------------------ pre-tokenisation (trainer.py:136-214)
    def _chunk_ranges(self, path: Path) -> list[tuple[int, int]]:
        size = path.stat().st_size
        with open(path, "rb") as f:
            def read(off: int, n: int) -> bytes:
                f.seek(off)
                return f.read(n)

            return chunk_ranges(size, self.config.chunk_size_bytes, read)

    def _split_pattern(self) -> "regex.Pattern[str]":
        pattern, group = pretokenizer(self.config)
        pat = split_pattern(group, PRETOKENIZER_NAMES[pattern])
        if self.config.special_tokens:  # specials first, in config order, kept as words (trainer.py:165-167)
            pat = "|".join(regex.escape(t) for t in self.config.special_tokens) + "|" + pat
        return regex.compile(pat)

    def _pretokenize(self, files: Sequence[Path]) -> list[str]:
        """All non-empty pre-tokens as strings, in file / chunk order."""
        pattern = self._split_pattern()
        errors = ERRORS[check_errors(getattr(self.config, "errors", "strict"))]
        replaced: list[int] = []  # per chunk (list.append is atomic)

        def run(path: Path, start: int, stop: int) -> list[str]:
            with open(path, "rb") as f:
                f.seek(start)
                raw = f.read(stop - start)
            try:
                if errors == "strict":
                    text = raw.decode("utf-8")
                else:
                    text, n = decode_counting(raw, errors)
                    replaced.append(n)
            except UnicodeDecodeError as e:
                raise ValueError(f"File {path} contains invalid UTF-8 at position {start + e.start}.") from e
            text = lowercase_text(text, getattr(self.config, "lowercase", False))
            return [t for t in pattern.findall(normalize_text(text, getattr(self.config, "normalizer", None))) if t]

        check_files(files)
        out: list[str] = []
        with ThreadPoolExecutor(max_workers=self.config.max_workers) as pool:
            jobs = []
            for path in files:
                for start, stop in self._chunk_ranges(path):
                    jobs.append(pool.submit(run, path, start, stop))
            for job in jobs:  # submission order => deterministic output order (trainer.py:209)
                out.extend(job.result())
        self.utf8_replaced = sum(replaced)
        return out

    def _preprocess_corpus(self, files: Sequence[Path]) -> list[list[int]]:
        """Pre-tokens as lists of byte values, as the reference returns them (trainer.py:136-214)."""
        return [list(t.encode("utf-8")) for t in self._pretokenize(files)]

    # ------------------------------------------------------------------ merge loop (trainer.py:216-302)
    def _merge_loop(self, sequences: list[list[int]]) -> tuple[dict[bytes, int], list[tuple[bytes, bytes]]]:
        """Runs the BPE merge loop on the GPU.  `sequences`: one list of byte values (0..255) per pre-token."""
        words = [bytes(s) for s in sequences]
        return self._merge_loop_words(words, None)

    @staticmethod
    def _host_words(words: Sequence[bytes], freq: np.ndarray | None):
        """Words on the host as _run takes them: (their bytes back to back, len(words) + 1 offsets, freq)"""
        off = np.zeros(len(words) + 1, dtype=np.uint64)
        np.cumsum(np.fromiter((len(w) for w in words), dtype=np.uint64, count=len(words)), out=off[1:])
        return np.frombuffer(b"".join(words), dtype=np.uint8), off, freq

    def _merge_loop_words(self, words: Sequence[bytes], freq: np.ndarray | None):
        max_token_bytes(self.config)
        base = self._base_tokens()
        if not words or self._budget() == 0:
            return {t: i for i, t in enumerate(base)}, []
        with self._context() as ctx:
            return self._run(ctx, base, self._host_words(words, freq), None, self._budget())
