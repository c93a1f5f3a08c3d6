"""CPU: the one chain of text passes, trainer.device_text_front -- utf8_repair, lowercase, normalize, the starts read back after
each -- driven directly and through its three callers (BBPETrainer._device_words, distributed._pretokenize_my_chunks,
BBPETokenizer._device_text) for every subset of the three settings.  `_native.Context` is the recording stand-in of
tests/test_trainer_routes.py with the three passes added: every pass returns an address of its own and shifts the starts, so
that the log shows what each step was given."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from tests.test_trainer_routes import A_TEXT, B_TEXT, BASE, JOINED, JOINED_STARTS, SP, Recorder, config
from tests.test_trainer_routes import files  # noqa: F401 (fixture)
from yet_another_bpe import _native
from yet_another_bpe.distributed import train_text_sharded
from yet_another_bpe.tokenizer import BBPETokenizer
from yet_another_bpe.trainer import BBPETrainer

ORDER = ("utf8_repair", "lowercase", "normalize")
TEXT_AT = {"utf8_repair": 0x10000, "lowercase": 0x20000, "normalize": 0x30000}    # the text a pass hands out
STARTS_AT = {"utf8_repair": 0x11000, "lowercase": 0x21000, "normalize": 0x31000}  # ... and its part offsets
N_OUT = {"utf8_repair": 901, "lowercase": 902, "normalize": 903}
SHIFT = {"utf8_repair": 1, "lowercase": 2, "normalize": 3}  # part k starts SHIFT * k later in the pass's text
SUBSETS = [frozenset(s) for r in range(4) for s in itertools.combinations(ORDER, r)]
N_SUBPARTS = 3
RUN = ("the segment that starts at byte {} holds more than 16384 code points to normalise together (a base and its combining marks): "
       "over the cap of 16384")


def key(text):
    """a text argument in the log: the address, or the host array's bytes"""
    return text if isinstance(text, int) else bytes(text)


class FrontRecorder(Recorder):
    empties = None   # the pass that leaves no byte
    too_long = None  # the position at which normalize finds a run over the cap

    def __init__(self, device=None):
        super().__init__(device)
        self.mem = {}

    def _pass(self, name, text, n_bytes, part_starts, *more):
        self.log.append((name, key(text), n_bytes, [int(s) for s in part_starts], *more))
        self.mem[STARTS_AT[name]] = [int(s) + SHIFT[name] * k for k, s in enumerate(part_starts)]
        return TEXT_AT[name], STARTS_AT[name], 0 if self.empties == name else N_OUT[name]

    def utf8_repair(self, text, n_bytes=None, part_starts=None, mode=_native.UTF8_MODES["replace"]):
        return self._pass("utf8_repair", text, n_bytes, part_starts, mode)

    def lowercase(self, text, n_bytes=None, part_starts=None):
        return self._pass("lowercase", text, n_bytes, part_starts)

    def normalize(self, text, n_bytes=None, part_starts=None, form=_native.NORM_NFC):
        if self.too_long is not None:
            self.log.append(("normalize", key(text), n_bytes, [int(s) for s in part_starts], form))
            raise _native.SegmentTooLong(self.too_long, RUN.format(self.too_long))
        return self._pass("normalize", text, n_bytes, part_starts, form)

    def d2h(self, ptr, n_bytes, dtype=np.uint8):
        self.log.append(("d2h", ptr, n_bytes))
        out = np.array(self.mem[ptr], dtype=dtype)
        assert out.nbytes == n_bytes
        return out

    def utf8_repair_stats(self):
        self.log.append(("utf8_repair_stats",))
        return {"n_subparts": N_SUBPARTS}

    def utf8_repair_free(self):
        self.log.append(("utf8_repair_free",))

    def lowercase_free(self):
        self.log.append(("lowercase_free",))

    def normalize_free(self):
        self.log.append(("normalize_free",))

    def pretokenize(self, text, n_bytes=None, chunk_starts=None, special_tokens=()):
        self.log.append(("pretokenize", key(text), n_bytes, [int(s) for s in chunk_starts], list(special_tokens)))
        return 0x1000, 0x2000, self.n_words

    def encode_to_host(self, text, n_bytes=None, doc_starts=None):
        self.log.append(("encode_to_host", key(text), n_bytes, [int(s) for s in doc_starts]))
        return np.zeros(0, np.uint32), np.zeros(len(doc_starts) + 1, np.uint64)


@pytest.fixture
def rec(monkeypatch):
    for name in ("YABPE_BATCH_BYTES", "YABPE_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    for name, value in (("log", []), ("n_words", 7), ("bad_utf8", None), ("empties", None), ("too_long", None)):
        monkeypatch.setattr(FrontRecorder, name, value)
    monkeypatch.setattr(_native, "Context", FrontRecorder)
    return FrontRecorder


def chain(text: bytes, starts, on, empties=None, mode=1):
    """What the chain must do with a host text: -> (the calls of the passes and the reads of their starts, in order, and what the
    consumer is given as (text, n_bytes, starts))"""
    calls, n_bytes, cur = [], None, [int(s) for s in starts]
    for name in ORDER:
        if name not in on:
            continue
        more = {"utf8_repair": (mode,), "lowercase": (), "normalize": (1,)}[name]
        calls += [(name, text, n_bytes, cur, *more), ("d2h", STARTS_AT[name], 8 * len(cur))]
        text, n_bytes, cur = TEXT_AT[name], 0 if name == empties else N_OUT[name], [s + SHIFT[name] * k for k, s in enumerate(cur)]
        if n_bytes == 0:  # nothing left: the later passes do not run, the consumer gets an empty host text
            text, n_bytes = b"", None
            break
    return calls, (text, n_bytes, cur)


def settings(on, mode="replace"):
    return {"errors": mode if "utf8_repair" in on else "strict", "lowercase": "lowercase" in on, "normalizer": "nfc" if "normalize" in on else None}


def passes(log):
    """the log without the calls that are not the chain's or its consumer's"""
    keep = set(ORDER) | {"d2h", "utf8_repair_stats", "pretokenize", "encode_to_host", "pool_add_ptr"} | {n + "_free" for n in ORDER + ("pretokenize",)}
    return [c for c in log if c[0] in keep]


CASES = [(on, empties) for on in SUBSETS for empties in (None, *[n for n in ORDER if n in on])]
IDS = ["+".join(n for n in ORDER if n in on) + (f"-{empties}_empties" if empties else "") or "none" for on, empties in CASES]


@pytest.mark.parametrize("on,empties", CASES, ids=IDS)
def test_chain_directly(rec, on, empties):
    from yet_another_bpe.trainer import device_text_front

    rec.empties = empties
    ctx = FrontRecorder()
    rec.log.clear()
    buf, starts = np.frombuffer(JOINED, np.uint8), JOINED_STARTS
    text, n_bytes, out = device_text_front(ctx, buf, None, starts, repair=2 if "utf8_repair" in on else 0, lower="lowercase" in on,
                                           form=1 if "normalize" in on else 0)
    calls, given = chain(JOINED, starts, on, empties, mode=2)
    assert rec.log == calls
    assert (key(text), n_bytes, [int(s) for s in out]) == given
    if given[1] is None and on:
        assert empties and isinstance(text, np.ndarray) and text.dtype == np.uint8 and text.size == 0
    if not on:
        assert text is buf and out is starts
    # a device text goes in as it came: the address and its length
    rec.empties = None
    rec.log.clear()
    device_text_front(ctx, 0x7000, 77, [0, 5], repair=1, lower=False, form=1)
    assert rec.log == [("utf8_repair", 0x7000, 77, [0, 5], 1), ("d2h", STARTS_AT["utf8_repair"], 16),
                       ("normalize", TEXT_AT["utf8_repair"], N_OUT["utf8_repair"], [0, 6], 1), ("d2h", STARTS_AT["normalize"], 16)]


def test_repair_runs_on_an_empty_text_and_the_others_do_not_follow(rec):
    from yet_another_bpe.trainer import device_text_front

    rec.empties = "utf8_repair"  # (what the driver's empty path returns: 0 bytes)
    ctx = FrontRecorder()
    rec.log.clear()
    text, n_bytes, out = device_text_front(ctx, np.zeros(0, np.uint8), None, [0, 0], repair=1, lower=True, form=1)
    assert rec.log == [("utf8_repair", b"", None, [0, 0], 1), ("d2h", STARTS_AT["utf8_repair"], 16)]
    assert (key(text), n_bytes, [int(s) for s in out]) == (b"", None, [0, 1])


@pytest.mark.parametrize("on,empties", CASES, ids=IDS)
def test_chain_through_the_trainer_and_the_sharded_driver(rec, files, on, empties):  # noqa: F811
    rec.empties = empties
    calls, given = chain(JOINED, JOINED_STARTS, on, empties)
    stats = [("utf8_repair_stats",)] if "utf8_repair" in on else []
    t = BBPETrainer(config(settings(on)))
    t.train(files)
    assert passes(rec.log) == [*calls, *stats, ("pretokenize", *given, SP)]
    assert t.utf8_replaced == (N_SUBPARTS if "utf8_repair" in on else 0)
    rec.log.clear()
    train_text_sharded(lambda: FrontRecorder(), files, config(settings(on)), 0, 1)
    assert passes(rec.log) == [*calls, ("pretokenize", *given, SP)]


@pytest.mark.parametrize("on,empties", CASES, ids=IDS)
def test_chain_through_the_tokenizer(rec, on, empties):
    rec.empties = empties
    s = settings(on, "ignore")
    tok = BBPETokenizer({t: i for i, t in enumerate(BASE)}, [], ["<s>"], normalizer=s["normalizer"], lowercase=s["lowercase"])
    docs = ["one two", "", "three"]
    tok.encode_array(docs, errors=s["errors"])
    calls, given = chain(b"one twothree", [0, 7, 7], on, empties, mode=2)
    assert passes(rec.log) == [*calls, ("encode_to_host", *given)]


def test_batched_route_frees_every_pass_per_batch(rec, files):  # noqa: F811
    t = BBPETrainer(config(settings(set(ORDER))))
    t.train(files, batch_bytes=250)
    expect = []
    for text, starts in ((JOINED[:249], [0, 100, 150]), (JOINED[249:], [0, 100])):
        calls, given = chain(text, starts, set(ORDER))
        expect += [*calls, ("utf8_repair_stats",), ("pretokenize", *given, SP), ("pool_add_ptr", 0x1000, 0x2000, 7, 0),
                   ("pretokenize_free",), ("normalize_free",), ("lowercase_free",), ("utf8_repair_free",)]
    assert passes(rec.log) == expect
    assert t.utf8_replaced == 2 * N_SUBPARTS
    # only the passes that ran are freed
    rec.log.clear()
    BBPETrainer(config(settings({"lowercase"}))).train(files, batch_bytes=250)
    assert [c[0] for c in passes(rec.log)][-3:] == ["pool_add_ptr", "pretokenize_free", "lowercase_free"]


# The messages of the parent commit (the three copies of the chain) for these two cases, with the file's path put in: position
# 270 of the text the normaliser read lies in the fourth chunk, bytes 99 to 199 of b.txt, which starts at 258 in the repaired and
# lowered text (249 + 3 * (1 + 2)) and at 255 in the lowered one (249 + 3 * 2).
REPAIRED_MESSAGE = ("File {} holds a run of code points that normalise together over the normaliser's cap in the chunk of bytes 99 to 199, at "
                    "position 12 of that chunk after its invalid UTF-8 was repaired: it holds more than 16384 code points to normalise together "
                    "(a base and its combining marks): over the cap of 16384")
STRICT_MESSAGE = ("File {} holds a run of code points that normalise together over the normaliser's cap at position 114: it holds more "
                  "than 16384 code points to normalise together (a base and its combining marks): over the cap of 16384")


@pytest.mark.parametrize("repair", [True, False], ids=["repaired", "strict"])
def test_a_run_over_the_cap_carries_the_starts_the_normaliser_read(rec, files, repair):  # noqa: F811
    from yet_another_bpe.trainer import device_text_front

    on = set(ORDER) if repair else {"lowercase", "normalize"}
    read = [s + (3 if repair else 2) * k for k, s in enumerate(JOINED_STARTS)]
    rec.too_long = 270
    with pytest.raises(_native.SegmentTooLong) as e:
        device_text_front(FrontRecorder(), np.frombuffer(JOINED, np.uint8), None, JOINED_STARTS, repair=int(repair), lower=True, form=1)
    assert rec.log[-1][0] == "normalize" and rec.log[-1][3] == read
    assert e.value.read_starts == read and e.value.repaired is repair and e.value.position == 270
    assert all(type(s0) is int for s0 in e.value.read_starts)
    message = (REPAIRED_MESSAGE if repair else STRICT_MESSAGE).format(files[1])
    for batch in (None, 1000):
        with pytest.raises(ValueError) as e:
            BBPETrainer(config(settings(on))).train(files, batch_bytes=batch)
        assert str(e.value) == message and isinstance(e.value.__cause__, _native.SegmentTooLong)
        assert rec.log[-1] == ("close",)
    with pytest.raises(ValueError) as e:
        train_text_sharded(lambda: FrontRecorder(), files, config(settings(on)), 0, 1)
    assert str(e.value) == message


def test_the_files_are_the_routes_files():
    assert len(A_TEXT) == 150 and len(B_TEXT) == 260 and JOINED_STARTS[3] == 249
