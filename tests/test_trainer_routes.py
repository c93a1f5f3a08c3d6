"""CPU: which library calls BBPETrainer.train / train_from and train_text_sharded make on each of their routes (host, device,
batched), in which order and with which arguments.  `_native.Context` is replaced by a stand-in that records every call, so
no library and no GPU is needed: what is pinned here is the Python host layer -- config -> options, chunk reading, the load
that is chosen, the budget rules, the place an invalid byte is reported at.  (The GPU tests pin that the real library gives
the right model for those calls.)"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

from yet_another_bpe import _native
from yet_another_bpe.distributed import train_text_sharded
from yet_another_bpe.tokenizer import BBPETokenizer
from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

SP = ["<s>"]
BASE = [bytes([b]) for b in range(256)] + [b"<s>"]
DEV_TEXT, DEV_OFF, POOL_BYTES, POOL_OFF, POOL_FREQ = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
N_WORDS, N_UNIQUE = 7, 5
STATS = {"merges_done": 2}
OLD = [(b"a", b"b"), (b"ab", b"c")]  # the merges of the model train_from continues: ids 257, 258
TOKS = BASE + [b"ab", b"abc"]
# what the stand-in's train() returns: over BASE two fresh ids (257, 258), over TOKS two merges whose bytes exist already
FIXED = (np.array([97, 257], np.uint32), np.array([98, 99], np.uint32), np.array([257, 258], np.uint32), np.array([9, 8], np.uint64))


class Recorder:
    """Stand-in for _native.Context: the methods the host drivers use, with the real signatures and defaults; every call goes
    into Recorder.log with its arguments (arrays as bytes / lists)."""
    log: list = []
    n_words = N_WORDS
    bad_utf8 = None  # (index of the pretokenize call that fails, position it reports)

    def __init__(self, device=None):
        self.log.append(("open",))
        self._pretok_calls = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.log.append(("close",))

    def set_option(self, name, value):
        self.log.append(("set_option", name, value))

    def set_vocab(self, tokens):
        self.log.append(("set_vocab", list(tokens)))

    def pretokenize(self, text, n_bytes=None, chunk_starts=None, special_tokens=()):
        self.log.append(("pretokenize", bytes(text), [int(s) for s in chunk_starts], list(special_tokens)))
        self._pretok_calls += 1
        if self.bad_utf8 and self.bad_utf8[0] == self._pretok_calls - 1:
            raise _native.Utf8Error(self.bad_utf8[1])
        return DEV_TEXT, DEV_OFF, self.n_words

    def pretokenize_free(self):
        self.log.append(("pretokenize_free",))

    def pool_add_ptr(self, bytes_ptr, off_ptr, n_words, freq_ptr=0):
        self.log.append(("pool_add_ptr", bytes_ptr, off_ptr, n_words, freq_ptr))

    def pool_get(self):
        self.log.append(("pool_get",))
        n = N_UNIQUE if self.n_words else 0
        return POOL_BYTES, POOL_OFF, POOL_FREQ, n, 40 if n else 0

    def pool_clear(self):
        self.log.append(("pool_clear",))

    @staticmethod
    def _arrays(flat, off, freq):
        return bytes(np.asarray(flat, np.uint8)), [int(x) for x in off], None if freq is None else [int(x) for x in freq]

    @staticmethod
    def _triples(triples):
        return tuple([int(x) for x in a] for a in triples)

    def load_words(self, flat, off, freq=None, dedup=False):
        self.log.append(("load_words", *self._arrays(flat, off, freq), dedup))

    def load_words_ptr(self, bytes_ptr, off_ptr, n_words, freq_ptr=0, dedup=False):
        self.log.append(("load_words_ptr", bytes_ptr, off_ptr, n_words, freq_ptr, dedup))

    def load_words_resumed(self, flat, off, freq, triples, dedup=False):
        self.log.append(("load_words_resumed", *self._arrays(flat, off, freq), self._triples(triples), dedup))

    def load_words_resumed_ptr(self, bytes_ptr, off_ptr, n_words, triples, freq_ptr=0, dedup=True):
        self.log.append(("load_words_resumed_ptr", bytes_ptr, off_ptr, n_words, self._triples(triples), freq_ptr, dedup))

    def train(self, num_merges, min_frequency):
        self.log.append(("train", num_merges, min_frequency))
        return FIXED

    def stats(self):
        self.log.append(("stats",))
        return dict(STATS)

    def encode_set_model(self, vocab, merges, specials_ordered, unk_id):
        self.log.append(("encode_set_model",))


@pytest.fixture
def rec(monkeypatch):
    for name in ("YABPE_PRETOKENIZE", "YABPE_BATCH_BYTES", "YABPE_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in (("log", []), ("n_words", N_WORDS), ("bad_utf8", None)):
        monkeypatch.setattr(Recorder, name, value)
    monkeypatch.setattr(_native, "Context", Recorder)
    return Recorder


A_TEXT = (b"one two three, it's 12345 and 678 again.  " * 4)[:150]
B_TEXT = b"x" * 99 + "é".encode() + ("naïve café 42 世界\n\n  tab\there " * 8).encode()[:159]
CHUNK = 100
A_CHUNKS = [(0, 100), (100, 150)]
B_CHUNKS = [(0, 99), (99, 199), (199, 260)]  # the cut at 100 is inside the two-byte sequence at 99 and moves back


@pytest.fixture
def files(tmp_path):
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes(A_TEXT)
    b.write_bytes(B_TEXT)
    B_TEXT.decode("utf-8")
    assert len(B_TEXT) == 260 and (B_TEXT[100] & 0xC0) == 0x80
    return [a, b]


PIECES = [A_TEXT[s:e] for s, e in A_CHUNKS] + [B_TEXT[s:e] for s, e in B_CHUNKS]
JOINED = b"".join(PIECES)
JOINED_STARTS = [0, 100, 150, 249, 349]

DEFAULT = {}
FULL = {"max_token_length": 5, "digit_group": 2, "pretokenizer": "cl100k"}
FULL_OPTIONS = [("set_option", "max_token_bytes", 5), ("set_option", "digit_group", 2), ("set_option", "split_pattern", 1)]


def config(extra, **kw):
    return BBPETrainerConfig(**{"vocab_size": 267, "min_frequency": -3, "special_tokens": SP, "chunk_size_bytes": CHUNK, **extra, **kw})


def old_model(extra):
    return BBPEModel({t: i for i, t in enumerate(TOKS)}, OLD, SP, digit_group=extra.get("digit_group"), pretokenizer=extra.get("pretokenizer", "gpt2"))


def run(entry, trainer, files, **kw):
    """entry "train": a fresh model (budget 267 - 257 = 10); "train_from": two merges more in front (budget 8)"""
    if entry == "train":
        return trainer.train(files, **kw)
    return trainer.train_from(old_model({k: getattr(trainer.config, k) for k in ("digit_group", "pretokenizer")}), files, **kw)


def options(extra):
    return FULL_OPTIONS if extra else []


def host_words(trainer, files, pooled):
    """The host path's load: (flat, off, freq) of the pre-tokens, pooled in first-seen order or every occurrence"""
    pretokens = trainer._pretokenize(files)
    count = Counter(pretokens)
    words = [t.encode("utf-8") for t in (count if pooled else pretokens)]
    return b"".join(words), np.cumsum([0] + [len(w) for w in words]).tolist(), list(count.values()) if pooled else None


TRIPLES = ([97, 257], [98, 99], [257, 258])
ENTRY = {  # entry point -> (tokens of set_vocab, budget, merges and vocab of the result after FIXED)
    "train": (BASE, 10, OLD, {t: i for i, t in enumerate(TOKS)}),
    "train_from": (TOKS, 8, OLD + OLD, {t: i for i, t in enumerate(TOKS)}),
}


def tail(entry):
    return [("train", ENTRY[entry][1], 0), ("stats",), ("close",)]  # (min_frequency -3 reaches the library as 0)


def check_result(entry, trainer, model, extra):
    assert model.merges == ENTRY[entry][2] and model.vocab == ENTRY[entry][3]
    assert trainer._merges == model.merges and trainer._vocab == model.vocab
    assert model.special_tokens == SP and model.pretokenizer == extra.get("pretokenizer", "gpt2")
    assert model.digit_group == extra.get("digit_group")
    assert trainer.last_stats == STATS


def test_chunks_of_the_corpus(files):
    t = BBPETrainer(config(DEFAULT))
    assert [t._chunk_ranges(f) for f in files] == [A_CHUNKS, B_CHUNKS]


@pytest.mark.parametrize("extra", [DEFAULT, FULL], ids=["default", "full"])
@pytest.mark.parametrize("layout", ["dedup", "flat"])
@pytest.mark.parametrize("entry", ["train", "train_from"])
def test_host_route(rec, files, monkeypatch, entry, layout, extra):
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    monkeypatch.setenv("YABPE_LAYOUT", layout)
    t = BBPETrainer(config(extra))
    model = run(entry, t, files)
    pooled = layout == "dedup" or entry == "train_from"  # train_from pools whatever the layout
    load = ("load_words", *host_words(t, files, pooled), False) if entry == "train" else \
        ("load_words_resumed", *host_words(t, files, pooled), TRIPLES, False)
    assert (load[3] is None) == (not pooled)
    assert rec.log == [("open",), *options(extra), ("set_vocab", ENTRY[entry][0]), load, *tail(entry)]
    check_result(entry, t, model, extra)


@pytest.mark.parametrize("extra", [DEFAULT, FULL], ids=["default", "full"])
@pytest.mark.parametrize("layout", ["dedup", "flat"])
@pytest.mark.parametrize("entry", ["train", "train_from"])
def test_device_route(rec, files, monkeypatch, entry, layout, extra):
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    monkeypatch.setenv("YABPE_LAYOUT", layout)
    t = BBPETrainer(config(extra))
    model = run(entry, t, files)
    dedup = layout == "dedup" or entry == "train_from"
    load = ("load_words_ptr", DEV_TEXT, DEV_OFF, N_WORDS, 0, dedup) if entry == "train" else \
        ("load_words_resumed_ptr", DEV_TEXT, DEV_OFF, N_WORDS, TRIPLES, 0, True)
    assert rec.log == [("open",), *options(extra), ("pretokenize", JOINED, JOINED_STARTS, SP), ("set_vocab", ENTRY[entry][0]), load,
                       *tail(entry)]
    check_result(entry, t, model, extra)


def batched_log(entry, extra, batches):
    log = [("open",), *options(extra)]
    for text, starts in batches:
        log += [("pretokenize", text, starts, SP), ("pool_add_ptr", DEV_TEXT, DEV_OFF, N_WORDS, 0), ("pretokenize_free",)]
    load = ("load_words_ptr", POOL_BYTES, POOL_OFF, N_UNIQUE, POOL_FREQ, False) if entry == "train" else \
        ("load_words_resumed_ptr", POOL_BYTES, POOL_OFF, N_UNIQUE, TRIPLES, POOL_FREQ, False)
    return log + [("pool_get",), ("set_vocab", ENTRY[entry][0]), load, ("pool_clear",), *tail(entry)]


@pytest.mark.parametrize("extra", [DEFAULT, FULL], ids=["default", "full"])
@pytest.mark.parametrize("entry", ["train", "train_from"])
def test_batched_route(rec, files, monkeypatch, entry, extra):
    t = BBPETrainer(config(extra))
    model = run(entry, t, files, batch_bytes=CHUNK)  # every chunk a batch of its own
    assert rec.log == batched_log(entry, extra, [(p, [0]) for p in PIECES])
    check_result(entry, t, model, extra)
    # chunks of two files in one batch; the environment variable does what the argument does
    rec.log.clear()
    monkeypatch.setenv("YABPE_BATCH_BYTES", "250")
    run(entry, BBPETrainer(config(extra)), files)
    assert rec.log == batched_log(entry, extra, [(JOINED[:249], [0, 100, 150]), (JOINED[249:], [0, 100])])


def test_batched_route_and_the_flat_layout(rec, files, monkeypatch):
    monkeypatch.setenv("YABPE_LAYOUT", "flat")
    with pytest.raises(ValueError, match="flat"):
        BBPETrainer(config(DEFAULT)).train(files, batch_bytes=CHUNK)
    assert rec.log == []
    run("train_from", BBPETrainer(config(DEFAULT)), files, batch_bytes=CHUNK)  # pooled regardless
    assert rec.log == batched_log("train_from", DEFAULT, [(p, [0]) for p in PIECES])


# CHANGED with the shared tail of the sharded drivers: min_frequency -3 reaches the library as 0, as it does from train (it
# went through unclamped before: ("train", 10, -3)).  The only expectation of this file that the refactor changed.
SHARDED_TRAIN = ("train", 10, 0)


def test_sharded_route(rec, files):
    for extra in (DEFAULT, FULL):
        rec.log.clear()
        model = train_text_sharded(lambda: Recorder(), files, config(extra), 0, 1, options={"verify": 1})
        assert rec.log == [("open",), ("set_option", "verify", 1), *options(extra), ("set_vocab", BASE),
                           ("pretokenize", JOINED, JOINED_STARTS, SP), ("load_words_ptr", DEV_TEXT, DEV_OFF, N_WORDS, 0, True),
                           SHARDED_TRAIN,
                           ("close",)]
        assert model.merges == OLD and model.vocab == ENTRY["train"][3] and model.special_tokens == SP
        assert model.pretokenizer == extra.get("pretokenizer", "gpt2") and model.digit_group == extra.get("digit_group")
    # no words on this rank: the empty load in the peers' layout
    rec.log.clear()
    rec.n_words = 0
    model = train_text_sharded(lambda: Recorder(), files, config(DEFAULT), 0, 1)
    assert rec.log[3:] == [("load_words", b"", [0], None, True), SHARDED_TRAIN, ("close",)]


@pytest.mark.parametrize("mode", ["host", "gpu", "batched"])
def test_zero_budget(rec, files, monkeypatch, mode):
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host" if mode == "host" else "gpu")
    kw = {"batch_bytes": 250} if mode == "batched" else {}
    # train: pre-tokenises all the same (an invalid byte would be reported), then the base model
    t = BBPETrainer(config(DEFAULT, vocab_size=257))
    model = t.train(files, **kw)
    pretok = {"host": [], "gpu": [("open",), ("pretokenize", JOINED, JOINED_STARTS, SP), ("close",)],
              "batched": batched_log("train", DEFAULT, [(JOINED[:249], [0, 100, 150]), (JOINED[249:], [0, 100])])[:8] + [("close",)]}
    assert rec.log == pretok[mode]
    assert model.merges == [] == t._merges and model.vocab == {tok: i for i, tok in enumerate(BASE)} == t._vocab and t.last_stats is None
    (files[1].parent / "bad.txt").write_bytes(b"ok \xff")
    with pytest.raises(ValueError, match=r"bad\.txt contains invalid UTF-8 at position 3\."):
        rec.bad_utf8 = (0, 3)
        BBPETrainer(config(DEFAULT, vocab_size=257)).train([files[1].parent / "bad.txt"], **kw)
    # train_from: the model unchanged, no context opened
    rec.log.clear()
    t = BBPETrainer(config(DEFAULT, vocab_size=259))
    model = run("train_from", t, files, **kw)
    assert rec.log == []
    assert model.merges == OLD == t._merges and model.vocab == {tok: i for i, tok in enumerate(TOKS)} == t._vocab and t.last_stats is None


@pytest.mark.parametrize("mode", ["host", "gpu", "batched"])
@pytest.mark.parametrize("entry", ["train", "train_from"])
def test_no_words(rec, files, tmp_path, monkeypatch, entry, mode):
    """Nothing to train on -- files without a byte, or a pre-tokeniser that returns no word: the base vocabulary from train,
    the model unchanged from train_from; no train call, last_stats untouched."""
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host" if mode == "host" else "gpu")
    kw = {"batch_bytes": 250} if mode == "batched" else {}
    toks = BASE if entry == "train" else TOKS
    (tmp_path / "empty.txt").write_bytes(b"")
    cases = [[tmp_path / "empty.txt"]] + ([files] if mode != "host" else [])
    rec.n_words = 0
    for corpus in cases:
        rec.log.clear()
        t = BBPETrainer(config(DEFAULT))
        model = run(entry, t, corpus, **kw)
        assert model.merges == (OLD if entry == "train_from" else []) == t._merges
        assert model.vocab == {tok: i for i, tok in enumerate(toks)} == t._vocab and t.last_stats is None
        if corpus is not files:
            assert rec.log == []  # an empty corpus opens no context
        else:
            assert rec.log[0] == ("open",) and rec.log[-1] == ("close",) and rec.log[-2] == (("pool_get",) if mode == "batched" else
                                                                                           ("pretokenize", JOINED, JOINED_STARTS, SP))
            assert not {"set_vocab", "train", "stats", "pool_clear"} & {c[0] for c in rec.log}


def test_invalid_utf8_is_located_in_its_file(rec, files, monkeypatch):
    """The stand-in reports a byte inside the second file's second chunk (file position 99 + 20)."""
    msg = r"File .*b\.txt contains invalid UTF-8 at position 119\."
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    for entry in ("train", "train_from"):
        rec.bad_utf8 = (0, 249 + 20)  # in the joined buffer
        with pytest.raises(ValueError, match=msg) as e:
            run(entry, BBPETrainer(config(DEFAULT)), files)
        assert isinstance(e.value.__cause__, _native.Utf8Error)
        rec.bad_utf8 = (1, 20)  # the second batch begins with that chunk: a position relative to the batch
        with pytest.raises(ValueError, match=msg):
            run(entry, BBPETrainer(config(DEFAULT)), files, batch_bytes=250)
        assert rec.log[-1] == ("close",)
    rec.bad_utf8 = (0, 249 + 20)
    with pytest.raises(ValueError, match=msg):
        train_text_sharded(lambda: Recorder(), files, config(DEFAULT), 0, 1)
    rec.bad_utf8 = (1, 100 + 20)  # the chunk after it
    with pytest.raises(ValueError, match=r"b\.txt contains invalid UTF-8 at position 219\."):
        BBPETrainer(config(DEFAULT)).train(files, batch_bytes=250)


@pytest.mark.parametrize("mode", ["host", "gpu", "batched"])
def test_order_of_errors(rec, files, tmp_path, monkeypatch, mode):
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host" if mode == "host" else "gpu")
    kw = {"batch_bytes": 250} if mode == "batched" else {}
    corpus = [files[0], tmp_path / "missing.txt"]
    for entry in ("train", "train_from"):
        with pytest.raises(ValueError, match="max_token_length"):
            run(entry, BBPETrainer(config(DEFAULT, max_token_length=1)), corpus, **kw)
        with pytest.raises(FileNotFoundError, match="File not found: .*missing.txt"):
            run(entry, BBPETrainer(config(DEFAULT)), corpus, **kw)
    with pytest.raises(ValueError, match="max_token_length"):
        train_text_sharded(lambda: Recorder(), corpus, config(DEFAULT, max_token_length=1), 0, 1)
    with pytest.raises(FileNotFoundError, match="File not found: .*missing.txt"):
        train_text_sharded(lambda: Recorder(), corpus, config(DEFAULT), 0, 1)
    # the model's checks of train_from come before the file checks
    with pytest.raises(ValueError, match="digit_group"):
        BBPETrainer(config(DEFAULT, digit_group=3)).train_from(old_model(DEFAULT), corpus, **kw)
    with pytest.raises(ValueError, match="pretokenizer"):
        BBPETrainer(config(DEFAULT, pretokenizer="cl100k")).train_from(old_model(DEFAULT), corpus, **kw)
    assert rec.log == []  # no context was opened


def test_auto_rule(rec, tmp_path):
    """Without YABPE_PRETOKENIZE: the device pre-tokeniser from 1 MiB of files on"""
    small, big = tmp_path / "small.txt", tmp_path / "big.txt"
    small.write_bytes(b"a b " * 10)
    big.write_bytes(b"a b " * (1 << 18))
    cfg = config(DEFAULT, chunk_size_bytes=1 << 30)
    BBPETrainer(cfg).train([small])
    assert [c[0] for c in rec.log] == ["open", "set_vocab", "load_words", "train", "stats", "close"]
    rec.log.clear()
    BBPETrainer(cfg).train([big])
    assert [c[0] for c in rec.log] == ["open", "pretokenize", "set_vocab", "load_words_ptr", "train", "stats", "close"]
    rec.log.clear()
    BBPETrainer(cfg).train([small, big])
    assert rec.log[1][:3] == ("pretokenize", small.read_bytes() + big.read_bytes(), [0, 40])


def test_merge_loop_words(rec):
    t = BBPETrainer(config(FULL))
    vocab, merges = t._merge_loop([[97, 98], [99], [97, 98]])
    assert rec.log == [("open",), *FULL_OPTIONS, ("set_vocab", BASE), ("load_words", b"abcab", [0, 2, 3, 5], None, False), ("train", 10, 0),
                       ("stats",), ("close",)]
    assert merges == OLD and vocab == ENTRY["train"][3] and t.last_stats == STATS
    rec.log.clear()
    assert BBPETrainer(config(DEFAULT))._merge_loop([]) == ({tok: i for i, tok in enumerate(BASE)}, [])
    assert rec.log == []


def test_tokenizer_device_options(rec):
    """The encoder's context gets the options of its pre-tokeniser, the names the trainer uses"""
    for kw, expect in (({}, []), ({"digit_group": 2}, FULL_OPTIONS[1:2]), ({"pretokenizer": "cl100k"}, [("set_option", "digit_group", 3), FULL_OPTIONS[2]]),
                       ({"pretokenizer": "cl100k", "digit_group": 2}, FULL_OPTIONS[1:])):
        rec.log.clear()
        BBPETokenizer({t: i for i, t in enumerate(BASE)}, [], ["7up", " x"], **kw)._device()  # (no trainer's rule for specials applies)
        assert rec.log == [("open",), *expect, ("encode_set_model",)]


def test_load_words_marshalling(monkeypatch):
    """The four load methods of _native.Context: which function of the library each calls, with which pointers, count, flags
    and merges; the arrays it marshalled outlive the call (Context._keep)."""
    import ctypes

    calls = []

    class Lib:
        @staticmethod
        def yabpe_load_words(h, *args):
            calls.append(("yabpe_load_words", *args))
            return 0

        @staticmethod
        def yabpe_load_words_resumed(h, *args):
            calls.append(("yabpe_load_words_resumed", *args))
            return 0

    def at(ptr, dtype, n):
        ptr = getattr(ptr, "value", ptr)
        return None if ptr is None else np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * n).from_address(ptr)).tolist()

    monkeypatch.setattr(_native, "lib", lambda: Lib)
    ctx = object.__new__(_native.Context)
    ctx._h = ctypes.c_void_p()
    flat, off, freq = np.frombuffer(b"abcab", np.uint8), [0, 2, 3, 5], [4, 5, 6]  # (lists: converted and kept by the call)
    triples = ([97, 257], [98, 99], [257, 258])
    empty = tuple(np.zeros(0, np.uint32) for _ in range(3))
    ctx.load_words(flat, off)
    ctx.load_words(flat, off, freq, dedup=True)
    ctx.load_words(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, dedup=True)
    for (name, pf, po, pq, n, flags), (words, counts, flag) in zip(calls, [(5, None, 0), (5, freq, 1), (0, None, 1)]):
        assert (name, n, flags) == ("yabpe_load_words", 3 if words else 0, flag)
        assert (pf is None) == (not words) and at(pf, np.uint8, words) == (list(b"abcab") if words else None)
        assert at(po, np.uint64, n + 1) == off[:n + 1] and at(pq, np.uint64, n) == counts
    calls.clear()
    ctx.load_words_resumed(flat, off, freq, triples)
    ctx.load_words_resumed(flat, off, None, empty, dedup=True)
    (name, pf, po, pq, n, flags, pl, pr, pm, k), second = calls
    assert (name, n, flags, k) == ("yabpe_load_words_resumed", 3, 0, 2) and at(pf, np.uint8, 5) == list(b"abcab")
    assert at(po, np.uint64, 4) == off and at(pq, np.uint64, 3) == freq
    assert (at(pl, np.uint32, 2), at(pr, np.uint32, 2), at(pm, np.uint32, 2)) == triples
    assert second[3:] == (None, 3, 1, None, None, None, 0)
    calls.clear()
    ctx.load_words_ptr(0x1000, 0x2000, 7)
    ctx.load_words_ptr(0x1000, 0x2000, 7, freq_ptr=0x3000, dedup=True)
    ctx.load_words_resumed_ptr(0x1000, 0x2000, 7, triples)  # (dedup is the default of this one alone)
    ctx.load_words_resumed_ptr(0x1000, 0x2000, 7, empty, freq_ptr=0x3000, dedup=False)
    plain = [tuple(getattr(a, "value", a) for a in c[:6]) for c in calls]
    assert plain == [("yabpe_load_words", 0x1000, 0x2000, None, 7, 0), ("yabpe_load_words", 0x1000, 0x2000, 0x3000, 7, 1),
                     ("yabpe_load_words_resumed", 0x1000, 0x2000, None, 7, 1), ("yabpe_load_words_resumed", 0x1000, 0x2000, 0x3000, 7, 0)]
    assert [at(p, np.uint32, 2) for p in calls[2][6:9]] == list(triples) and calls[2][9] == 2
    assert calls[3][6:] == (None, None, None, 0)
