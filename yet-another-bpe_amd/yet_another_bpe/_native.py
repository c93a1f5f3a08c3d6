"""ctypes binding of libyabpe.so (C ABI: include/yabpe.h) -- the only way the Python host reaches the GPU.

No fallback of any kind: if the library is not built, or no MI355X is visible, this raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int64, c_uint8, c_uint32, c_uint64, c_void_p
from pathlib import Path

import numpy as np

_CSRC = Path(__file__).resolve().parent.parent / "csrc"
LIB_PATH = Path(os.environ.get("YABPE_LIB", _CSRC / "libyabpe.so"))


class YabpeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"yabpe error {code}: {msg}")
        self.code = code


class Utf8Error(ValueError):
    """yabpe_pretokenize found malformed UTF-8; .position = UnicodeDecodeError.start inside the buffer."""

    def __init__(self, position: int):
        super().__init__(f"invalid UTF-8 at byte {position}")
        self.position = position


class SegmentTooLong(ValueError):
    """yabpe_normalize met a run of code points that normalise together (a base and its combining marks) over the cap;
    .position = the byte where that segment starts inside the buffer."""

    def __init__(self, position: int, msg: str):
        super().__init__(msg)
        self.position = position


E_CAPACITY = -4
E_UTF8 = -7
NORM_NFC = 1  # yabpe_normalize: form
UTF8_MODES = {"replace": 1, "ignore": 2}  # yabpe_utf8_repair: mode (YABPE_UTF8_*)


class Stats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in (
        "n_words", "n_words_input", "n_long_words", "tokens_initial", "tokens_now", "merges_done", "n_tiles",
        "live_slots", "table_capacity", "table_entries", "retiles", "table_rebuilds")] + [
        ("load_ms", c_double), ("train_ms", c_double), ("apply_ms_sampled", c_double)] + [(n, c_uint64) for n in (
            "apply_launches_sampled", "apply_algo_bytes_sampled", "apply_actual_bytes_sampled", "algo_bytes_total")] + [
        ("scan_ms_sampled", c_double)] + [(n, c_uint64) for n in (
            "scan_launches_sampled", "scan_algo_bytes_sampled", "scan_actual_bytes_sampled", "scan_skip_launches", "scan_skip_tiles_read", "cand_rebuilds", "cand_rescans", "fused_launches")] + [
        ("dense_ms_sampled", c_double)] + [(n, c_uint64) for n in ("dense_launches_sampled", "dense_algo_bytes_sampled", "dense_actual_bytes_sampled")] + [
        ("sparse_ms", c_double), ("sparse_merges", c_uint64), ("tail_ms", c_double), ("tail_merges", c_uint64)] + [
        (n, c_uint64) for n in ("exchanges", "exchange_bytes", "exchange_cap_records", "exchange_growths", "exchange_max_records", "sparse_launches", "tail_launches")] + [("exchange_ms_sampled", c_double), ("exchanges_sampled", c_uint64), ("exchange_p2p", c_uint64),
        ("dense_launches", c_uint64), ("dense_merges", c_uint64), ("scan_skip_pieces_taken", c_uint64),
        ("pool_growths", c_uint64)]


class EncodeStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_bytes", "n_docs", "n_pretokens", "n_unique", "n_unique_long", "n_specials", "n_ids")] + [
        (n, c_double) for n in ("split_ms", "pretok_ms", "pool_ms", "words_ms", "emit_ms", "total_ms")]


class DecodeStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_ids", "n_docs", "n_unknown", "n_gathered", "n_bytes", "n_replacements", "n_docs_repaired")] + [
        (n, c_double) for n in ("lengths_ms", "gather_ms", "check_ms", "repair_ms", "total_ms")]


class LayoutStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_ids", "n_docs", "n_rows", "row_len", "n_truncated_docs", "n_ids_dropped", "n_pad_slots")] + [
        (n, c_double) for n in ("lengths_ms", "write_ms", "total_ms")]


class Mask(ctypes.Structure):
    """yabpe_mask_t"""
    _fields_ = [(n, c_uint64) for n in ("seed", "first_doc", "select_threshold", "mask_threshold", "random_threshold")] + [
        (n, c_uint32) for n in ("mask_id", "n_random", "ignore", "flags")]


class MaskStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_ids", "n_docs", "n_protected", "n_selected", "n_masked", "n_random", "n_kept")] + [
        (n, c_double) for n in ("mask_ms", "total_ms")]


class Span(ctypes.Structure):
    """yabpe_span_t"""
    _fields_ = [(n, c_uint64) for n in ("seed", "first_doc", "open_threshold")] + [("len_threshold", c_uint64 * 31), ("max_len", c_uint32),
                                                                                   ("n_sentinels", c_uint32), ("sentinels", c_void_p),
                                                                                   ("max_doc_ids", c_uint64), ("flags", c_uint32)]


class SpanStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_ids", "n_docs", "n_protected", "n_noise", "n_runs", "n_runs_over", "n_cut", "n_in", "n_tgt")] + [
        (n, c_double) for n in ("flags_ms", "index_ms", "place_ms", "write_ms", "kernel_ms", "total_ms")]


class Fim(ctypes.Structure):
    """yabpe_fim_t"""
    _fields_ = [(n, c_uint64) for n in ("seed", "first_doc", "fim_threshold", "spm_threshold")] + [
        (n, c_uint32) for n in ("pre_id", "suf_id", "mid_id", "eot_id", "ignore")] + [("max_len", c_uint64), ("flags", c_uint32)]


class FimStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_docs", "n_psm", "n_spm", "n_truncated_docs", "n_ids_dropped", "n_out")] + [
        (n, c_double) for n in ("cuts_ms", "plan_ms", "write_ms", "total_ms")]


class Layout(ctypes.Structure):
    """yabpe_layout_t"""
    _fields_ = [(n, c_uint32) for n in ("row_len", "pad_id", "bos_id", "eos_id", "flags")]


class Windows(ctypes.Structure):
    """yabpe_windows_t"""
    _fields_ = [(n, c_void_p) for n in ("rows", "row_doc", "row_start", "row_len", "spans")] + [("n_rows", c_uint64)]


class Pairs(ctypes.Structure):
    """yabpe_pairs_t"""
    _fields_ = [(n, c_uint32) for n in ("sep_id", "n_sep", "mode", "stride")]


class PairRows(ctypes.Structure):
    """yabpe_pair_rows_t"""
    _fields_ = [(n, c_void_p) for n in ("rows", "types", "row_pair", "row_start", "first_len", "second_len", "spans")] + [("n_rows", c_uint64)]


class FitRows(ctypes.Structure):
    """yabpe_fit_rows_t"""
    _fields_ = [(n, c_void_p) for n in ("ids", "doc", "pos", "used")] + [("n_rows", c_uint64)]


class ResumeStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_unique", "n_long", "tokens")] + [(n, c_double) for n in ("segment_ms", "build_ms")]


class PoolStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_calls", "n_words_added", "n_empty_dropped", "n_unique", "n_bytes", "slot_capacity",
                                        "arena_capacity", "slot_growths", "arena_growths")] + [
        (n, c_double) for n in ("pool_ms", "probe_ms", "append_ms", "total_ms")]


class NormalizeStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_bytes_in", "n_bytes_out", "n_parts", "n_suspects", "n_dirty", "n_dirty_long", "n_copied")] + [
        (n, c_double) for n in ("class_ms", "find_ms", "segments_ms", "write_ms", "total_ms")]


class Utf8Stats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_bytes_in", "n_bytes_out", "n_parts", "n_subparts")] + [("first_bad_pos", c_int64)] + [
        (n, c_double) for n in ("check_ms", "write_ms", "total_ms")]


class LowercaseStats(ctypes.Structure):
    _fields_ = [(n, c_uint64) for n in ("n_bytes_in", "n_bytes_out", "n_parts", "n_changed", "n_resized", "n_sigma", "n_final_sigma", "path",
                                        "n_copied")] + [(n, c_double) for n in ("check_ms", "scan_ms", "write_ms", "total_ms")]


class Latency(ctypes.Structure):
    _fields_ = [(n, c_double) for n in ("launch_gap_us", "load_trip_us", "coherent_trip_us", "atomic_trip_us")]


_lib = None
# int fn(void *user, const void *send_dev, void *recv_dev, uint64_t nbytes)  (include/yabpe.h: yabpe_allgather_fn)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_uint64)

# every symbol include/yabpe.h declares (tests/test_abi.py checks the library exports all of them)
SYMBOLS = [
    "yabpe_abi_version", "yabpe_device_count", "yabpe_create", "yabpe_destroy", "yabpe_last_error", "yabpe_set_option",
    "yabpe_set_vocab", "yabpe_load_words", "yabpe_train", "yabpe_n_tokens", "yabpe_token_bytes", "yabpe_stats",
    "yabpe_iter_log", "yabpe_event_log", "yabpe_latency_probe", "yabpe_verify_table", "yabpe_stream_checksum", "yabpe_stream_dump", "yabpe_synth_generate", "yabpe_synth_generate_lex", "yabpe_synth_free",
    "yabpe_memcpy_d2h", "yabpe_memcpy_h2d", "yabpe_pretokenize", "yabpe_pretokenize_free",
    "yabpe_comm_unique_id", "yabpe_comm_init", "yabpe_comm_init_custom", "yabpe_comm_enable_p2p",
    "yabpe_encode_set_model", "yabpe_encode", "yabpe_encode_spans", "yabpe_encode_dropout", "yabpe_encode_words", "yabpe_encode_free", "yabpe_encode_stats", "yabpe_encode_checksum",
    "yabpe_decode_set_model", "yabpe_decode", "yabpe_decode_free", "yabpe_decode_stats",
    "yabpe_load_words_resumed", "yabpe_resume_stats",
    "yabpe_layout_pad", "yabpe_layout_pack", "yabpe_layout_windows", "yabpe_layout_pairs", "yabpe_layout_fit", "yabpe_layout_free", "yabpe_layout_stats",
    "yabpe_mask", "yabpe_mask_free", "yabpe_mask_stats",
    "yabpe_span_corrupt", "yabpe_span_free", "yabpe_span_stats",
    "yabpe_fim_cuts", "yabpe_fim", "yabpe_fim_free", "yabpe_fim_stats",
    "yabpe_pool_add", "yabpe_pool_get", "yabpe_pool_clear", "yabpe_pool_stats",
    "yabpe_normalize", "yabpe_normalize_free", "yabpe_normalize_stats",
    "yabpe_utf8_repair", "yabpe_utf8_repair_free", "yabpe_utf8_repair_stats",
    "yabpe_lowercase", "yabpe_lowercase_free", "yabpe_lowercase_stats",
]


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C {_CSRC}` (hipcc --offload-arch=gfx950). "
                "The BPE hot path has no CPU fallback.")
        L = ctypes.CDLL(str(LIB_PATH))
        L.yabpe_abi_version.restype = c_int
        L.yabpe_device_count.restype = c_int
        L.yabpe_create.argtypes = [POINTER(c_void_p), c_int]
        L.yabpe_destroy.argtypes = [c_void_p]
        L.yabpe_destroy.restype = None
        L.yabpe_last_error.argtypes = [c_void_p]
        L.yabpe_last_error.restype = c_char_p
        L.yabpe_set_option.argtypes = [c_void_p, c_char_p, c_int64]
        L.yabpe_set_vocab.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
        L.yabpe_load_words.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32]
        L.yabpe_load_words_resumed.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32]
        L.yabpe_resume_stats.argtypes = [c_void_p, POINTER(ResumeStats)]
        L.yabpe_train.argtypes = [c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_uint32)]
        L.yabpe_n_tokens.argtypes = [c_void_p, POINTER(c_uint32)]
        L.yabpe_token_bytes.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, POINTER(c_uint32)]
        L.yabpe_stats.argtypes = [c_void_p, POINTER(Stats)]
        L.yabpe_iter_log.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]
        L.yabpe_event_log.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]
        L.yabpe_verify_table.argtypes = [c_void_p, POINTER(c_uint64)]
        L.yabpe_stream_checksum.argtypes = [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]
        L.yabpe_stream_dump.argtypes = [c_void_p, POINTER(c_uint32), POINTER(c_uint32), c_void_p, c_void_p, c_void_p, c_void_p]
        L.yabpe_synth_generate.argtypes = [c_void_p, c_uint64, c_uint32, c_uint64, c_void_p, c_uint32, c_int,
                                           POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64), POINTER(c_uint64)]
        L.yabpe_synth_generate_lex.argtypes = [c_void_p, c_uint64, c_uint32, c_uint64, c_void_p, c_void_p,
                                               POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64), POINTER(c_uint64)]
        L.yabpe_synth_free.argtypes = [c_void_p]
        L.yabpe_pretokenize.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32,
                                        POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_pretokenize_free.argtypes = [c_void_p]
        L.yabpe_memcpy_d2h.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64]
        L.yabpe_memcpy_h2d.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64]
        L.yabpe_comm_unique_id.argtypes = [c_void_p]
        L.yabpe_comm_init.argtypes = [c_void_p, c_int, c_int, c_void_p]
        L.yabpe_comm_init_custom.argtypes = [c_void_p, c_int, c_int, ALLGATHER_FN, c_void_p]
        L.yabpe_comm_enable_p2p.argtypes = [c_void_p]
        L.yabpe_encode_set_model.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32,
                                             c_void_p, c_void_p, c_uint32, c_uint32]
        L.yabpe_encode.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                   POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_encode_spans.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                         POINTER(c_void_p), POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_encode_dropout.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_uint64, POINTER(c_void_p),
                                           POINTER(c_void_p), POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_encode_words.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                         POINTER(c_void_p), POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_encode_free.argtypes = [c_void_p]
        L.yabpe_encode_stats.argtypes = [c_void_p, POINTER(EncodeStats)]
        L.yabpe_encode_checksum.argtypes = [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]
        L.yabpe_decode_set_model.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
        L.yabpe_decode.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64)]
        L.yabpe_decode_free.argtypes = [c_void_p]
        L.yabpe_decode_stats.argtypes = [c_void_p, POINTER(DecodeStats)]
        L.yabpe_layout_pad.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(Layout), POINTER(c_void_p), POINTER(c_void_p),
                                       POINTER(c_uint32)]
        L.yabpe_layout_pack.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(Layout), POINTER(c_void_p), POINTER(c_void_p),
                                        POINTER(c_void_p), POINTER(c_uint64)]
        L.yabpe_layout_windows.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(Layout), c_uint32, POINTER(Windows)]
        L.yabpe_layout_pairs.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(Layout), POINTER(Pairs), POINTER(PairRows)]
        L.yabpe_layout_fit.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(Layout), POINTER(FitRows)]
        L.yabpe_layout_free.argtypes = [c_void_p]
        L.yabpe_layout_stats.argtypes = [c_void_p, POINTER(LayoutStats)]
        L.yabpe_mask.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(Mask), POINTER(c_void_p), POINTER(c_void_p)]
        L.yabpe_mask_free.argtypes = [c_void_p]
        L.yabpe_mask_stats.argtypes = [c_void_p, POINTER(MaskStats)]
        L.yabpe_span_corrupt.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(Span), POINTER(c_void_p), POINTER(c_void_p),
                                         POINTER(c_uint64), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64)]
        L.yabpe_span_free.argtypes = [c_void_p]
        L.yabpe_span_stats.argtypes = [c_void_p, POINTER(SpanStats)]
        L.yabpe_fim_cuts.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(Fim), POINTER(c_void_p), POINTER(c_void_p)]
        L.yabpe_fim.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(Fim), POINTER(c_void_p), POINTER(c_void_p),
                                POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64)]
        L.yabpe_fim_free.argtypes = [c_void_p]
        L.yabpe_fim_stats.argtypes = [c_void_p, POINTER(FimStats)]
        L.yabpe_pool_add.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]
        L.yabpe_pool_get.argtypes = [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint64), POINTER(c_uint64)]
        L.yabpe_pool_clear.argtypes = [c_void_p]
        L.yabpe_pool_stats.argtypes = [c_void_p, POINTER(PoolStats)]
        L.yabpe_normalize.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                      POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_normalize_free.argtypes = [c_void_p]
        L.yabpe_normalize_stats.argtypes = [c_void_p, POINTER(NormalizeStats)]
        L.yabpe_utf8_repair.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                        POINTER(c_uint64)]
        L.yabpe_utf8_repair_free.argtypes = [c_void_p]
        L.yabpe_utf8_repair_stats.argtypes = [c_void_p, POINTER(Utf8Stats)]
        L.yabpe_lowercase.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_void_p),
                                      POINTER(c_uint64), POINTER(ctypes.c_int64)]
        L.yabpe_lowercase_free.argtypes = [c_void_p]
        L.yabpe_lowercase_stats.argtypes = [c_void_p, POINTER(LowercaseStats)]
        if L.yabpe_abi_version() != 2:
            raise ImportError("libyabpe.so ABI version mismatch")
        _lib = L
    return _lib


LOAD_DEDUP = 0x1
SPANS_CHARS = 0x1  # yabpe_encode_spans: code points instead of bytes
LAYOUT_BOS, LAYOUT_EOS, LAYOUT_TRUNC_LEFT, LAYOUT_PAD_LEFT, LAYOUT_DROP_LAST = 0x01, 0x02, 0x04, 0x08, 0x10  # yabpe_layout_t.flags
LAYOUT_NO_DOC = 0xFFFFFFFF  # `doc` of a packed slot past the end of the stream
WORD_SPECIAL = 0x80000000  # yabpe_encode_words: bit 31 of a words entry (YABPE_WORD_SPECIAL)
MASK_WHOLE_WORD = 0x1  # yabpe_mask_t.flags
MASK_IGNORE = 0xFFFFFF9C  # yabpe_mask_t.ignore: -100 as i32, the label a loss skips
SPAN_WHOLE_WORD, SPAN_FINAL_SENTINEL = 0x1, 0x2  # yabpe_span_t.flags
SPAN_MAX_LEN = 32  # YABPE_SPAN_MAX_LEN
FIM_EOT, FIM_LOSS_MIDDLE, FIM_PIECES = 0x1, 0x2, 0x4  # yabpe_fim_t.flags
PAIRS_MODES = {"longest_first": 0, "only_first": 1, "only_second": 2, "windows": 3}  # yabpe_pairs_t.mode (YABPE_PAIRS_*)


def _text_arg(text, n_bytes):
    """A text argument -- bytes / u8 array (the library stages it) or a device address (then n_bytes is required) -> (the array
    that must outlive the call or None, pointer, length)"""
    if isinstance(text, int):
        return None, c_void_p(text), int(n_bytes)
    keep = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    return keep, c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)


def _starts_arg(starts) -> np.ndarray:
    """Ascending chunk / part / document starts as the u64 table a driver takes (None or empty: one, at 0)"""
    return np.ascontiguousarray(starts if starts is not None and len(starts) else [0], dtype=np.uint64)


def _stats_dict(s: ctypes.Structure) -> dict:
    return {f: getattr(s, f) for f, _ in s._fields_}


class Context:
    """One GPU context == one merge-loop run (or several yabpe_train continuations)."""

    def __init__(self, device: int | None = None):
        L = lib()
        if device is None:
            device = int(os.environ.get("YABPE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self._h = c_void_p()
        rc = L.yabpe_create(byref(self._h), device)
        if rc != 0:
            raise YabpeError(rc, L.yabpe_last_error(None).decode())
        self.device = device
        for k, v in os.environ.items():  # YABPE_OPT_check_interval=16 etc.
            if k.startswith("YABPE_OPT_"):
                self.set_option(k[len("YABPE_OPT_"):], int(v))

    # -- lifetime
    def close(self) -> None:
        if self._h:
            lib().yabpe_destroy(self._h)
            self._h = c_void_p()

    def __enter__(self) -> "Context":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        if rc != 0:
            raise YabpeError(rc, lib().yabpe_last_error(self._h).decode())

    # -- API
    def set_option(self, name: str, value: int) -> None:
        self._chk(lib().yabpe_set_option(self._h, name.encode(), int(value)))

    def set_vocab(self, tokens: list[bytes]) -> None:
        blob = np.frombuffer(b"".join(tokens), dtype=np.uint8)
        off = np.zeros(len(tokens) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(t) for t in tokens])
        self._base = list(tokens)
        self._chk(lib().yabpe_set_vocab(self._h, blob.ctypes.data, off.ctypes.data, len(tokens)))

    def _load(self, flat, off, n_words: int | None, freq, dedup: bool, triples=None) -> None:
        """yabpe_load_words; with `triples` ((left, right, merged) u32 arrays) yabpe_load_words_resumed.  flat, off, freq: host
        arrays (u8 bytes, n + 1 u64 offsets, n u64 counts or None) when n_words is None, else addresses (freq 0: no counts).
        The arrays handed to the library stay in self._keep, so they outlive the call."""
        if n_words is None:
            flat, off = np.ascontiguousarray(flat, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
            freq = None if freq is None else np.ascontiguousarray(freq, dtype=np.uint64)
            n_words = len(off) - 1
            assert freq is None or len(freq) == n_words
            words = (flat.ctypes.data if flat.size else None, off.ctypes.data, None if freq is None else freq.ctypes.data)
        else:
            words = (c_void_p(flat), c_void_p(off), c_void_p(freq) if freq else None)
        l, r, m = (np.ascontiguousarray(x, dtype=np.uint32) for x in (triples if triples is not None else ((), (), ())))
        self._keep = (flat, off, freq, l, r, m)
        if triples is None:
            self._chk(lib().yabpe_load_words(self._h, *words, n_words, LOAD_DEDUP if dedup else 0))
        else:
            self._chk(lib().yabpe_load_words_resumed(self._h, *words, n_words, LOAD_DEDUP if dedup else 0,
                                                     *(x.ctypes.data if len(l) else None for x in (l, r, m)), len(l)))

    def load_words(self, flat, off, freq=None, dedup: bool = False) -> None:
        """flat: u8 bytes, off: u64 offsets (n+1), freq: optional u64 counts: numpy arrays on the host."""
        self._load(flat, off, None, freq, dedup)

    def load_words_ptr(self, bytes_ptr: int, off_ptr: int, n_words: int, freq_ptr: int = 0, dedup: bool = False) -> None:
        """Device (or host) addresses, e.g. from synth_generate() or torch tensors' data_ptr()."""
        self._load(bytes_ptr, off_ptr, n_words, freq_ptr, dedup)

    # -- continuing from a trained model: `triples` = (left, right, merged) u32 arrays (merge_triples), after set_vocab with
    # all of the model's tokens
    def load_words_resumed(self, flat, off, freq, triples, dedup: bool = False) -> None:
        self._load(flat, off, None, freq, dedup, triples)

    def load_words_resumed_ptr(self, bytes_ptr: int, off_ptr: int, n_words: int, triples, freq_ptr: int = 0, dedup: bool = True) -> None:
        """Device (or host) addresses for the words, e.g. the results of pretokenize()."""
        self._load(bytes_ptr, off_ptr, n_words, freq_ptr, dedup, triples)

    def resume_stats(self) -> dict:
        s = ResumeStats()
        self._chk(lib().yabpe_resume_stats(self._h, byref(s)))
        return _stats_dict(s)

    def train(self, num_merges: int, min_frequency: int):
        left = np.zeros(max(num_merges, 1), dtype=np.uint32)
        right = np.zeros_like(left)
        merged = np.zeros_like(left)
        count = np.zeros(max(num_merges, 1), dtype=np.uint64)
        n = c_uint32(0)
        self._chk(lib().yabpe_train(self._h, num_merges, min_frequency, left.ctypes.data, right.ctypes.data,
                                    merged.ctypes.data, count.ctypes.data, byref(n)))
        k = n.value
        return left[:k], right[:k], merged[:k], count[:k]

    def n_tokens(self) -> int:
        n = c_uint32(0)
        self._chk(lib().yabpe_n_tokens(self._h, byref(n)))
        return n.value

    def token_bytes(self, tid: int) -> bytes:
        ln = c_uint32(0)
        self._chk(lib().yabpe_token_bytes(self._h, tid, None, 0, byref(ln)))
        buf = (c_uint8 * max(ln.value, 1))()
        self._chk(lib().yabpe_token_bytes(self._h, tid, buf, ln.value, byref(ln)))
        return bytes(buf[:ln.value])

    def stats(self) -> dict:
        s = Stats()
        self._chk(lib().yabpe_stats(self._h, byref(s)))
        return _stats_dict(s)

    def iter_log(self):
        n = c_uint32(0)
        self._chk(lib().yabpe_iter_log(self._h, None, None, 0, byref(n)))
        sites = np.zeros(max(n.value, 1), dtype=np.uint64)
        live = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._chk(lib().yabpe_iter_log(self._h, sites.ctypes.data, live.ctypes.data, n.value, byref(n)))
        return sites[:n.value], live[:n.value]

    def event_log(self):
        n = c_uint32(0)
        self._chk(lib().yabpe_event_log(self._h, None, None, None, 0, byref(n)))
        it = np.zeros(max(n.value, 1), dtype=np.uint32)
        us = np.zeros(max(n.value, 1), dtype=np.float32)
        scan = np.zeros(max(n.value, 1), dtype=np.float32)
        self._chk(lib().yabpe_event_log(self._h, it.ctypes.data, us.ctypes.data, scan.ctypes.data, n.value, byref(n)))
        return it[:n.value], us[:n.value], scan[:n.value]

    def latency_probe(self) -> dict:
        """Measured latency pieces of one sparse merge on this device (include/yabpe.h yabpe_latency_t), microseconds."""
        s = Latency()
        self._chk(lib().yabpe_latency_probe(self._h, byref(s)))
        return _stats_dict(s)

    def verify_table(self) -> int:
        m = c_uint64(0)
        self._chk(lib().yabpe_verify_table(self._h, byref(m)))
        return m.value

    def stream_checksum(self) -> tuple[int, int, int]:
        a, b, c = c_uint64(0), c_uint64(0), c_uint64(0)
        self._chk(lib().yabpe_stream_checksum(self._h, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    def stream_dump(self) -> dict:
        """The resident tile stream as it lies in memory: n_tiles, tiles (n_tiles x 1024 u16), tile_len, tile_wbase (None in
        the flat layout) and sig (512 x n_tiles u64, None while the skip index is not valid)."""
        n, fl = c_uint32(0), c_uint32(0)
        self._chk(lib().yabpe_stream_dump(self._h, byref(n), byref(fl), None, None, None, None))
        nt = n.value
        tiles = np.zeros((nt, 1024), dtype=np.uint16)
        tlen = np.zeros(nt, dtype=np.uint32)
        wbase = np.zeros(nt, dtype=np.uint32) if fl.value & 1 else None
        sig = np.zeros((512, nt), dtype=np.uint64) if fl.value & 2 else None
        if nt:
            self._chk(lib().yabpe_stream_dump(self._h, byref(n), byref(fl), tiles.ctypes.data, tlen.ctypes.data,
                                              None if wbase is None else wbase.ctypes.data, None if sig is None else sig.ctypes.data))
        return {"n_tiles": nt, "tiles": tiles, "tile_len": tlen, "tile_wbase": wbase, "sig": sig}

    def synth_generate(self, target_bytes: int, n_types: int, seed: int, alphabet: bytes, space_prefix: bool):
        """-> (dev_bytes_ptr, dev_off_ptr, n_words, n_bytes); buffers live until close()/synth_free()."""
        al = np.frombuffer(alphabet, dtype=np.uint8)
        pb, po, nw, nb = c_void_p(), c_void_p(), c_uint64(0), c_uint64(0)
        self._chk(lib().yabpe_synth_generate(self._h, target_bytes, n_types, seed, al.ctypes.data, len(al),
                                             1 if space_prefix else 0, byref(pb), byref(po), byref(nw), byref(nb)))
        return pb.value, po.value, nw.value, nb.value

    def synth_generate_lex(self, target_bytes: int, seed: int, lex_bytes: np.ndarray, lex_off: np.ndarray):
        """Synthetic text from a lexicon (synth.text_lexicon): -> (dev_bytes_ptr, dev_piece_off_ptr, n_pieces, n_bytes)."""
        lb = np.ascontiguousarray(lex_bytes, dtype=np.uint8)
        lo = np.ascontiguousarray(lex_off, dtype=np.uint64)
        pb, po, nw, nb = c_void_p(), c_void_p(), c_uint64(0), c_uint64(0)
        self._chk(lib().yabpe_synth_generate_lex(self._h, c_uint64(target_bytes), c_uint32(len(lo) - 1), c_uint64(seed), c_void_p(lb.ctypes.data),
                                                 c_void_p(lo.ctypes.data), byref(pb), byref(po), byref(nw), byref(nb)))
        return pb.value, po.value, nw.value, nb.value

    def synth_free(self) -> None:
        self._chk(lib().yabpe_synth_free(self._h))

    def pretokenize(self, text, n_bytes: int | None = None, chunk_starts=None, special_tokens=()):
        """GPT-2 pre-tokenisation on the device (reference trainer.py:136-214; with the option "digit_group" = G the digit
        runs are cut into groups of G, with the option "split_pattern" = 1 the cl100k pattern is used, with 3 the o200k_base pattern, include/yabpe.h).  `text`: bytes / u8 array (staged) or a
        device address (then n_bytes is required).  chunk_starts: ascending chunk starts, first one 0.
        -> (dev_text_ptr, dev_word_off_ptr, n_words); raises Utf8Error(position) on malformed UTF-8."""
        _keep, ptr, n = _text_arg(text, n_bytes)
        ch = _starts_arg(chunk_starts)
        sb = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in special_tokens]
        spb = np.frombuffer(b"".join(sb) or b"\0", dtype=np.uint8)
        spo = np.zeros(len(sb) + 1, dtype=np.uint32)
        if sb:
            spo[1:] = np.cumsum([len(x) for x in sb])
        dt, do, nw, bad = c_void_p(), c_void_p(), c_uint64(0), ctypes.c_int64(-1)
        rc = lib().yabpe_pretokenize(self._h, ptr, n, ch.ctypes.data, len(ch), spb.ctypes.data, spo.ctypes.data, len(sb),
                                     byref(dt), byref(do), byref(nw), byref(bad))
        if rc == E_UTF8:
            raise Utf8Error(bad.value)
        self._chk(rc)
        return dt.value or 0, do.value, nw.value

    def pretokenize_free(self) -> None:
        self._chk(lib().yabpe_pretokenize_free(self._h))

    # -- the text passes in front of pretokenize() / encode(): text in, text and part offsets out
    def _pass_to_host(self, dt: int, do: int, nb: int, n_parts: int):
        """A pass's device results -> (text u8[nb], part_off u64[n_parts + 1]) copied to the host."""
        return (self.d2h(dt, nb) if nb else np.zeros(0, np.uint8)), self.d2h(do, 8 * (n_parts + 1), np.uint64)

    # -- Unicode normalisation in front of pretokenize() / encode() (include/yabpe.h: yabpe_normalize)
    def normalize(self, text, n_bytes: int | None = None, part_starts=None, form: int = NORM_NFC):
        """NFC of every part of `text` on the device.  `text`: bytes / u8 array (staged) or a device address (then n_bytes is
        required).  part_starts: ascending part starts, the first one 0 (None: one part); parts are normalised independently.
        -> (dev_text_ptr, dev_part_off_ptr u64[n_parts + 1], n_bytes_out); the buffers live until the next normalize,
        normalize_free() or close().  A text that is NFC already comes back as it is (a device address: the same address).
        Raises Utf8Error(position) on malformed UTF-8 and SegmentTooLong(position) over the cap, positions in the input."""
        _keep, ptr, n = _text_arg(text, n_bytes)
        st = _starts_arg(part_starts)
        dt, do, nb, bad = c_void_p(), c_void_p(), c_uint64(0), ctypes.c_int64(-1)
        rc = lib().yabpe_normalize(self._h, ptr, n, st.ctypes.data, len(st), int(form), byref(dt), byref(do), byref(nb), byref(bad))
        if rc == E_UTF8:
            raise Utf8Error(bad.value)
        if rc == E_CAPACITY and bad.value >= 0:
            raise SegmentTooLong(bad.value, lib().yabpe_last_error(self._h).decode())
        self._chk(rc)
        return dt.value or 0, do.value, nb.value

    def normalize_to_host(self, text, n_bytes: int | None = None, part_starts=None, form: int = NORM_NFC):
        """-> (text u8[n_bytes_out], part_off u64[n_parts + 1]) copied to the host."""
        return self._pass_to_host(*self.normalize(text, n_bytes, part_starts, form), len(_starts_arg(part_starts)))

    def normalize_free(self) -> None:
        self._chk(lib().yabpe_normalize_free(self._h))

    def normalize_stats(self) -> dict:
        s = NormalizeStats()
        self._chk(lib().yabpe_normalize_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- errors="replace" / "ignore" in front of normalize() / pretokenize() / encode() (include/yabpe.h: yabpe_utf8_repair)
    def utf8_repair(self, text, n_bytes: int | None = None, part_starts=None, mode: int = UTF8_MODES["replace"]):
        """part.decode("utf-8", errors).encode() of every part of `text` on the device.  `text`: bytes / u8 array (staged) or a
        device address (then n_bytes is required).  part_starts: ascending part starts, the first one 0 (None: one part); a
        sequence cut off by a part's end is ill-formed there.  mode: UTF8_MODES["replace"] or ["ignore"].
        -> (dev_text_ptr, dev_part_off_ptr u64[n_parts + 1], n_bytes_out); the buffers live until the next utf8_repair,
        utf8_repair_free() or close().  A text that is valid comes back as it is (a device address: the same address)."""
        _keep, ptr, n = _text_arg(text, n_bytes)
        st = _starts_arg(part_starts)
        dt, do, nb = c_void_p(), c_void_p(), c_uint64(0)
        self._chk(lib().yabpe_utf8_repair(self._h, ptr, n, st.ctypes.data, len(st), int(mode), byref(dt), byref(do), byref(nb)))
        return dt.value or 0, do.value, nb.value

    def utf8_repair_to_host(self, text, n_bytes: int | None = None, part_starts=None, mode: int = UTF8_MODES["replace"]):
        """-> (text u8[n_bytes_out], part_off u64[n_parts + 1]) copied to the host."""
        return self._pass_to_host(*self.utf8_repair(text, n_bytes, part_starts, mode), len(_starts_arg(part_starts)))

    def utf8_repair_free(self) -> None:
        self._chk(lib().yabpe_utf8_repair_free(self._h))

    def utf8_repair_stats(self) -> dict:
        s = Utf8Stats()
        self._chk(lib().yabpe_utf8_repair_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- str.lower() between utf8_repair() and normalize() (include/yabpe.h: yabpe_lowercase)
    def lowercase(self, text, n_bytes: int | None = None, part_starts=None):
        """part.lower() of every part of `text` on the device.  `text`: bytes / u8 array (staged) or a device address (then
        n_bytes is required).  part_starts: ascending part starts, the first one 0 (None: one part); parts are lowered
        independently (the final-sigma rule does not look across a part boundary).
        -> (dev_text_ptr, dev_part_off_ptr u64[n_parts + 1], n_bytes_out); the buffers live until the next lowercase,
        lowercase_free() or close().  A text that is lower case already comes back as it is (a 16-byte aligned device
        address: the same address).  Raises Utf8Error(position) on malformed UTF-8, the position in the input."""
        _keep, ptr, n = _text_arg(text, n_bytes)
        st = _starts_arg(part_starts)
        dt, do, nb, bad = c_void_p(), c_void_p(), c_uint64(0), ctypes.c_int64(-1)
        rc = lib().yabpe_lowercase(self._h, ptr, n, st.ctypes.data, len(st), byref(dt), byref(do), byref(nb), byref(bad))
        if rc == E_UTF8:
            raise Utf8Error(bad.value)
        self._chk(rc)
        return dt.value or 0, do.value, nb.value

    def lowercase_to_host(self, text, n_bytes: int | None = None, part_starts=None):
        """-> (text u8[n_bytes_out], part_off u64[n_parts + 1]) copied to the host."""
        return self._pass_to_host(*self.lowercase(text, n_bytes, part_starts), len(_starts_arg(part_starts)))

    def lowercase_free(self) -> None:
        self._chk(lib().yabpe_lowercase_free(self._h))

    def lowercase_stats(self) -> dict:
        s = LowercaseStats()
        self._chk(lib().yabpe_lowercase_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- encoding with a trained model (BBPETokenizer.encode on the device)
    def encode_set_model(self, vocab: dict, merges, specials_ordered, unk_id: int) -> None:
        """vocab {bytes: id}, merges [(bytes, bytes)] in order, specials in the tokenizer's order (longest first)."""
        a = encode_model_arrays(vocab, merges, specials_ordered)
        self._enc_model = a  # (the library copies; kept only for the duration of the call)
        self._chk(lib().yabpe_encode_set_model(self._h, a["vb"].ctypes.data, a["vo"].ctypes.data, a["vi"].ctypes.data, len(a["vi"]),
                                               a["mb"].ctypes.data, a["mo"].ctypes.data, len(a["mo"]) // 2, a["sb"].ctypes.data,
                                               a["so"].ctypes.data, len(a["so"]) - 1, int(unk_id)))

    def _encode_call(self, text, n_bytes, doc_starts, flags, dropout=None, words=False):
        """yabpe_encode (flags None), yabpe_encode_spans, yabpe_encode_dropout (dropout = (threshold, seed)) or yabpe_encode_words
        (words) -> (dev ids, dev doc_off, dev spans / dev words or None, n_ids)"""
        _keep, ptr, n = _text_arg(text, n_bytes)
        docs = _starts_arg(doc_starts)
        di, dd, ds, ni, bad = c_void_p(), c_void_p(), c_void_p(), c_uint64(0), ctypes.c_int64(-1)
        if words:
            rc = lib().yabpe_encode_words(self._h, ptr, n, docs.ctypes.data, len(docs), byref(di), byref(dd), byref(ds), byref(ni), byref(bad))
        elif dropout is not None:
            rc = lib().yabpe_encode_dropout(self._h, ptr, n, docs.ctypes.data, len(docs), int(dropout[0]), int(dropout[1]), byref(di), byref(dd),
                                            byref(ni), byref(bad))
        elif flags is None:
            rc = lib().yabpe_encode(self._h, ptr, n, docs.ctypes.data, len(docs), byref(di), byref(dd), byref(ni), byref(bad))
        else:
            rc = lib().yabpe_encode_spans(self._h, ptr, n, docs.ctypes.data, len(docs), int(flags), byref(di), byref(dd), byref(ds), byref(ni),
                                          byref(bad))
        if rc == E_UTF8:
            raise Utf8Error(bad.value)
        self._chk(rc)
        return di.value or 0, dd.value, ds.value, ni.value

    def encode(self, text, n_bytes: int | None = None, doc_starts=None):
        """text: bytes / u8 array (staged) or a device address (n_bytes required); doc_starts: ascending document starts, the
        first one 0.  -> (dev_ids_ptr u32, dev_doc_off_ptr u64[n_docs + 1], n_ids); the buffers live until the next encode,
        encode_free() or close().  Raises Utf8Error(position) on malformed UTF-8."""
        di, dd, _ds, ni = self._encode_call(text, n_bytes, doc_starts, None)
        return di, dd, ni

    def encode_to_host(self, text, n_bytes: int | None = None, doc_starts=None):
        """-> (ids u32[n_ids], doc_off u64[n_docs + 1]) copied to the host."""
        n_docs = len(doc_starts) if doc_starts is not None and len(doc_starts) else 1
        di, dd, ni = self.encode(text, n_bytes, doc_starts)
        ids = self.d2h(di, 4 * ni, np.uint32) if ni else np.zeros(0, np.uint32)
        return ids, self.d2h(dd, 8 * (n_docs + 1), np.uint64)

    def encode_spans(self, text, n_bytes: int | None = None, doc_starts=None, chars: bool = False):
        """encode() plus every id's span in its document (yabpe_encode_spans; chars: code points instead of bytes).
        -> (dev_ids_ptr u32, dev_doc_off_ptr u64[n_docs + 1], dev_spans_ptr u64[2 n_ids] as (start, end) pairs, n_ids)."""
        return self._encode_call(text, n_bytes, doc_starts, SPANS_CHARS if chars else 0)

    def encode_spans_to_host(self, text, n_bytes: int | None = None, doc_starts=None, chars: bool = False):
        """-> (ids u32[n_ids], doc_off u64[n_docs + 1], spans u64[n_ids, 2]) copied to the host."""
        n_docs = len(doc_starts) if doc_starts is not None and len(doc_starts) else 1
        di, dd, ds, ni = self.encode_spans(text, n_bytes, doc_starts, chars)
        ids = self.d2h(di, 4 * ni, np.uint32) if ni else np.zeros(0, np.uint32)
        spans = self.d2h(ds, 16 * ni, np.uint64).reshape(-1, 2) if ni else np.zeros((0, 2), np.uint64)
        return ids, self.d2h(dd, 8 * (n_docs + 1), np.uint64), spans

    def encode_dropout(self, text, threshold: int, seed: int = 0, n_bytes: int | None = None, doc_starts=None):
        """encode() with BPE-dropout (yabpe_encode_dropout): threshold = min(2^32, int(p * 2^32)), seed in [0, 2^64).
        -> (dev_ids_ptr u32, dev_doc_off_ptr u64[n_docs + 1], n_ids), owned and released as encode()'s."""
        di, dd, _ds, ni = self._encode_call(text, n_bytes, doc_starts, None, dropout=(threshold, seed))
        return di, dd, ni

    def encode_dropout_to_host(self, text, threshold: int, seed: int = 0, n_bytes: int | None = None, doc_starts=None):
        """-> (ids u32[n_ids], doc_off u64[n_docs + 1]) copied to the host."""
        n_docs = len(doc_starts) if doc_starts is not None and len(doc_starts) else 1
        di, dd, ni = self.encode_dropout(text, threshold, seed, n_bytes, doc_starts)
        ids = self.d2h(di, 4 * ni, np.uint32) if ni else np.zeros(0, np.uint32)
        return ids, self.d2h(dd, 8 * (n_docs + 1), np.uint64)

    def encode_words(self, text, n_bytes: int | None = None, doc_starts=None):
        """encode() plus the piece of its document every id was made from (yabpe_encode_words).
        -> (dev_ids_ptr u32, dev_doc_off_ptr u64[n_docs + 1], dev_words_ptr u32[n_ids]: the piece index, WORD_SPECIAL set for a
        special occurrence, n_ids), owned and released as encode()'s."""
        return self._encode_call(text, n_bytes, doc_starts, None, words=True)

    def encode_words_to_host(self, text, n_bytes: int | None = None, doc_starts=None):
        """-> (ids u32[n_ids], doc_off u64[n_docs + 1], words u32[n_ids] without the flag bit, special bool[n_ids]) copied to
        the host."""
        n_docs = len(doc_starts) if doc_starts is not None and len(doc_starts) else 1
        di, dd, dw, ni = self.encode_words(text, n_bytes, doc_starts)
        ids = self.d2h(di, 4 * ni, np.uint32) if ni else np.zeros(0, np.uint32)
        words = self.d2h(dw, 4 * ni, np.uint32) if ni else np.zeros(0, np.uint32)
        return ids, self.d2h(dd, 8 * (n_docs + 1), np.uint64), words & np.uint32(WORD_SPECIAL - 1), (words >> 31).astype(bool)

    def encode_free(self) -> None:
        self._chk(lib().yabpe_encode_free(self._h))

    def encode_stats(self) -> dict:
        s = EncodeStats()
        self._chk(lib().yabpe_encode_stats(self._h, byref(s)))
        return _stats_dict(s)

    def encode_checksum(self) -> tuple[int, int, int]:
        a, b, c = c_uint64(0), c_uint64(0), c_uint64(0)
        self._chk(lib().yabpe_encode_checksum(self._h, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    # -- decoding with a trained model (BBPETokenizer.decode on the device)
    def decode_set_model(self, vocab: dict) -> None:
        """vocab {bytes: id}: the table id -> bytes (when two strings share an id, the last one in dict order wins)."""
        a = decode_model_arrays(vocab)
        self._chk(lib().yabpe_decode_set_model(self._h, a["vb"].ctypes.data, a["vo"].ctypes.data, a["vi"].ctypes.data, len(a["vi"])))

    def decode(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None):
        """ids: u32 array (staged) or a device address (n_ids required); doc_starts: ascending document starts into the ids,
        the first one 0, as an array or a device address (n_docs required); None: one document.
        -> (dev_text_ptr u8, dev_text_off_ptr u64[n_docs + 1], n_bytes); the buffers live until the next decode, decode_free()
        or close()."""
        keep = None
        if isinstance(ids, int):
            ptr, n = c_void_p(ids), int(n_ids)
        else:
            keep = np.ascontiguousarray(ids, dtype=np.uint32)
            ptr, n = c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)
        if isinstance(doc_starts, int):
            dptr, nd = c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        dt, do, nb = c_void_p(), c_void_p(), c_uint64(0)
        self._chk(lib().yabpe_decode(self._h, ptr, n, dptr, nd, byref(dt), byref(do), byref(nb)))
        return dt.value or 0, do.value, nb.value

    def decode_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None):
        """-> (text u8[n_bytes], text_off u64[n_docs + 1]) copied to the host."""
        if n_docs is None:
            n_docs = len(doc_starts) if doc_starts is not None and not isinstance(doc_starts, int) and len(doc_starts) else 1
        dt, do, nb = self.decode(ids, n_ids, doc_starts, n_docs)
        text = self.d2h(dt, nb) if nb else np.zeros(0, np.uint8)
        return text, self.d2h(do, 8 * (n_docs + 1), np.uint64)

    def decode_free(self) -> None:
        self._chk(lib().yabpe_decode_free(self._h))

    def decode_stats(self) -> dict:
        s = DecodeStats()
        self._chk(lib().yabpe_decode_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- fixed-shape batches (BBPETokenizer.encode_batch_padded / encode_batch_packed / encode_batch_windows on the device)
    @staticmethod
    def _layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id, flags):
        """ids / doc_starts as decode() takes them -> (keep-alive arrays, ids pointer, n_ids, starts pointer, n_docs, Layout)"""
        keep = docs = None
        if isinstance(ids, int):
            ptr, n = c_void_p(ids), int(n_ids)
        else:
            keep = np.ascontiguousarray(ids, dtype=np.uint32)
            ptr, n = c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)
        if isinstance(doc_starts, int):
            dptr, nd = c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        flags = int(flags) | (LAYOUT_BOS if bos_id is not None else 0) | (LAYOUT_EOS if eos_id is not None else 0)
        return (keep, docs), ptr, n, dptr, nd, Layout(int(row_len), int(pad_id), int(bos_id or 0), int(eos_id or 0), flags)

    @staticmethod
    def _spans_arg(spans, n_ids):
        """spans: None, a device address, or a u64 array [n_ids, 2] -> (keep-alive array, spans pointer)"""
        if spans is None or isinstance(spans, int):
            return None, c_void_p(spans or 0)
        keep_spans = np.ascontiguousarray(spans, dtype=np.uint64)
        if keep_spans.size != 2 * n_ids:
            raise ValueError(f"spans must hold one (start, end) per id: {keep_spans.size} values for {n_ids} ids")
        if not keep_spans.size:
            keep_spans = np.zeros(2, np.uint64)  # (no ids: never read, but not NULL -- the call still returns spans)
        return keep_spans, c_void_p(keep_spans.ctypes.data)

    def _rows_to_host(self, dev_ptr, n_rows, *shape, dtype=np.uint32):
        """a flat device result -> its host copy [n_rows, *shape] (no elements: nothing to copy, the pointer may be 0)"""
        n = int(n_rows * np.prod(shape, dtype=np.int64))
        flat = self.d2h(dev_ptr, n * np.dtype(dtype).itemsize, dtype) if n else np.zeros(0, dtype)
        return flat.reshape(n_rows, *shape)

    def layout_pad(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, row_len: int = 0, pad_id: int = 0,
                   bos_id: int | None = None, eos_id: int | None = None, trunc_left: bool = False, pad_left: bool = False, flags: int = 0):
        """One padded row per document (yabpe_layout_pad).  ids: u32 array (staged) or a device address (n_ids required);
        doc_starts: ascending document starts into the ids, the first one 0, as an array or a device address (n_docs
        required); None: one document -- encode()'s device results go straight in.  row_len 0: the longest sequence.
        flags: further YABPE_LAYOUT_* bits as they are.
        -> (dev_rows_ptr u32[n_docs * row_len], dev_len_ptr u32[n_docs], row_len); the buffers live until the next layout
        call, layout_free() or close()."""
        _keep, ptr, n, dptr, nd, lay = self._layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id,
                                                         flags | (LAYOUT_TRUNC_LEFT if trunc_left else 0) | (LAYOUT_PAD_LEFT if pad_left else 0))
        dr, dl, rl = c_void_p(), c_void_p(), c_uint32(0)
        self._chk(lib().yabpe_layout_pad(self._h, ptr, n, dptr, nd, byref(lay), byref(dr), byref(dl), byref(rl)))
        return dr.value or 0, dl.value or 0, rl.value

    def layout_pad_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, **kw):
        """-> (rows u32[n_docs, row_len], lengths u32[n_docs]) copied to the host."""
        if n_docs is None:
            n_docs = len(doc_starts) if doc_starts is not None and not isinstance(doc_starts, int) and len(doc_starts) else 1
        dr, dl, rl = self.layout_pad(ids, n_ids, doc_starts, n_docs, **kw)
        return self._rows_to_host(dr, n_docs, rl), self._rows_to_host(dl, n_docs)

    def layout_pack(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, row_len: int = 0, pad_id: int = 0,
                    bos_id: int | None = None, eos_id: int | None = None, drop_last: bool = False, flags: int = 0):
        """The documents end to end in rows of row_len (yabpe_layout_pack); arguments as layout_pad takes them.
        -> (dev_ids_ptr, dev_doc_ptr, dev_pos_ptr: u32[n_rows * row_len] each, n_rows); the buffers live until the next
        layout call, layout_free() or close()."""
        _keep, ptr, n, dptr, nd, lay = self._layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id,
                                                         flags | (LAYOUT_DROP_LAST if drop_last else 0))
        di, dd, dp, nr = c_void_p(), c_void_p(), c_void_p(), c_uint64(0)
        self._chk(lib().yabpe_layout_pack(self._h, ptr, n, dptr, nd, byref(lay), byref(di), byref(dd), byref(dp), byref(nr)))
        return di.value or 0, dd.value or 0, dp.value or 0, nr.value

    def layout_pack_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, **kw):
        """-> (ids, doc, pos), each u32[n_rows, row_len], copied to the host."""
        di, dd, dp, nr = self.layout_pack(ids, n_ids, doc_starts, n_docs, **kw)
        rl = int(kw.get("row_len", 0))
        return tuple(self._rows_to_host(p, nr, rl) for p in (di, dd, dp))

    def layout_windows(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, spans=None, row_len: int = 0,
                       stride: int = 0, pad_id: int = 0, bos_id: int | None = None, eos_id: int | None = None, pad_left: bool = False,
                       flags: int = 0):
        """Rows of row_len with consecutive rows of a document sharing `stride` ids (yabpe_layout_windows); ids, doc_starts and
        the ids of the layout as layout_pad takes them.  spans: None, or what encode_spans returns next to the ids -- a u64
        array [n_ids, 2] (staged) or a device address.
        -> (dev_rows_ptr u32[n_rows * row_len], dev_row_doc_ptr, dev_row_start_ptr, dev_lengths_ptr: u32[n_rows] each,
        dev_spans_ptr u64[n_rows * row_len * 2] or 0 without spans, n_rows); the buffers live until the next layout call,
        layout_free() or close()."""
        _keep, ptr, n, dptr, nd, lay = self._layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id,
                                                         flags | (LAYOUT_PAD_LEFT if pad_left else 0))
        _keep_spans, sptr = self._spans_arg(spans, n)
        w = Windows()
        self._chk(lib().yabpe_layout_windows(self._h, ptr, n, dptr, nd, sptr, byref(lay), int(stride), byref(w)))
        return w.rows or 0, w.row_doc or 0, w.row_start or 0, w.row_len or 0, w.spans or 0, w.n_rows

    def layout_windows_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, spans=None, **kw):
        """-> (rows u32[n_rows, row_len], row_doc, row_start, lengths: u32[n_rows] each) copied to the host, with spans also
        the slots' spans u64[n_rows, row_len, 2]."""
        dr, dd, ds, dl, dsp, nr = self.layout_windows(ids, n_ids, doc_starts, n_docs, spans, **kw)
        rl = int(kw.get("row_len", 0))
        out = (self._rows_to_host(dr, nr, rl),) + tuple(self._rows_to_host(p, nr) for p in (dd, ds, dl))
        return out + (self._rows_to_host(dsp, nr, rl, 2, dtype=np.uint64),) if spans is not None else out

    def layout_pairs(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, spans=None, row_len: int = 0,
                     mode="longest_first", stride: int = 0, sep_id: int | None = None, n_sep: int = 1, pad_id: int = 0,
                     bos_id: int | None = None, eos_id: int | None = None, pad_left: bool = False, flags: int = 0):
        """Documents 2p and 2p + 1 as the two sides of pair p in rows of row_len (yabpe_layout_pairs); ids, doc_starts, spans
        and the ids of the layout as layout_windows takes them (an empty doc_starts array: no pairs).  mode: a name of
        PAIRS_MODES or a YABPE_PAIRS_* value; sep_id None: no separator, else n_sep copies of it between the sides.
        -> (dev_rows_ptr u32[n_rows * row_len], dev_types_ptr u8[n_rows * row_len], dev_row_pair_ptr, dev_row_start_ptr,
        dev_first_len_ptr, dev_second_len_ptr: u32[n_rows] each, dev_spans_ptr u64[n_rows * row_len * 2] or 0 without spans,
        n_rows); the buffers live until the next layout call, layout_free() or close()."""
        _keep, ptr, n, dptr, nd, lay = self._layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id,
                                                         flags | (LAYOUT_PAD_LEFT if pad_left else 0))
        if doc_starts is not None and not isinstance(doc_starts, int) and len(doc_starts) == 0:
            nd = 0
        _keep_spans, sptr = self._spans_arg(spans, n)
        pairs = Pairs(int(sep_id or 0), int(n_sep) if sep_id is not None else 0, PAIRS_MODES[mode] if isinstance(mode, str) else int(mode),
                      int(stride))
        w = PairRows()
        self._chk(lib().yabpe_layout_pairs(self._h, ptr, n, dptr, nd, sptr, byref(lay), byref(pairs), byref(w)))
        return (w.rows or 0, w.types or 0, w.row_pair or 0, w.row_start or 0, w.first_len or 0, w.second_len or 0, w.spans or 0, w.n_rows)

    def layout_pairs_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, spans=None, **kw):
        """-> (rows u32[n_rows, row_len], types u8[n_rows, row_len], row_pair, row_start, first_len, second_len: u32[n_rows]
        each) copied to the host, with spans also the slots' spans u64[n_rows, row_len, 2]."""
        dr, dt, *per_row, dsp, nr = self.layout_pairs(ids, n_ids, doc_starts, n_docs, spans, **kw)
        rl = int(kw.get("row_len", 0))
        out = (self._rows_to_host(dr, nr, rl), self._rows_to_host(dt, nr, rl, dtype=np.uint8)) + tuple(self._rows_to_host(p, nr) for p in per_row)
        return out + (self._rows_to_host(dsp, nr, rl, 2, dtype=np.uint64),) if spans is not None else out

    def layout_fit(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, row_len: int = 0, pad_id: int = 0,
                   bos_id: int | None = None, eos_id: int | None = None, flags: int = 0):
        """Whole documents in rows of row_len, packed by best-fit decreasing (yabpe_layout_fit); ids, doc_starts and the ids of
        the layout as layout_pad takes them (an empty doc_starts array: no documents).
        -> (dev_ids_ptr, dev_doc_ptr, dev_pos_ptr: u32[n_rows * row_len] each, dev_used_ptr u32[n_rows], n_rows); the buffers
        live until the next layout call, layout_free() or close()."""
        _keep, ptr, n, dptr, nd, lay = self._layout_args(ids, n_ids, doc_starts, n_docs, row_len, pad_id, bos_id, eos_id, flags)
        if doc_starts is not None and not isinstance(doc_starts, int) and len(doc_starts) == 0:
            nd = 0
        w = FitRows()
        self._chk(lib().yabpe_layout_fit(self._h, ptr, n, dptr, nd, byref(lay), byref(w)))
        return w.ids or 0, w.doc or 0, w.pos or 0, w.used or 0, w.n_rows

    def layout_fit_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, **kw):
        """-> (ids, doc, pos: u32[n_rows, row_len] each, used u32[n_rows]) copied to the host."""
        di, dd, dp, du, nr = self.layout_fit(ids, n_ids, doc_starts, n_docs, **kw)
        rl = int(kw.get("row_len", 0))
        return tuple(self._rows_to_host(p, nr, rl) for p in (di, dd, dp)) + (self._rows_to_host(du, nr),)

    def layout_free(self) -> None:
        self._chk(lib().yabpe_layout_free(self._h))

    def layout_stats(self) -> dict:
        s = LayoutStats()
        self._chk(lib().yabpe_layout_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- masked-language-model batches (BBPETokenizer.mask_tokens on the device)
    def mask(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, words=None, *, seed: int = 0, first_doc: int = 0,
             select: int = 0, mask: int = 0, random: int = 0, mask_id: int = 0, n_random: int = 0, ignore: int = MASK_IGNORE,
             whole_word: bool = False, flags: int = 0):
        """One masking draw over ragged ids (yabpe_mask).  ids / doc_starts as layout_pad takes them; words: None, a u32 array
        (staged) or a device address -- what encode_words returns, flag bit included.  select, mask, random: the thresholds
        Ts, Tm, Tr = min(2^32, int(x * 2^32)).  flags: further YABPE_MASK_* bits as they are.
        -> (dev_ids_ptr u32[n_ids], dev_labels_ptr u32[n_ids]); the buffers live until the next mask, mask_free() or close()."""
        keep = docs = keep_words = None
        if isinstance(ids, int):
            ptr, n = c_void_p(ids), int(n_ids)
        else:
            keep = np.ascontiguousarray(ids, dtype=np.uint32)
            ptr, n = c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)
        if isinstance(doc_starts, int):
            dptr, nd = c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        if words is None or isinstance(words, int):
            wptr = c_void_p(words or 0)
        else:
            keep_words = np.ascontiguousarray(words, dtype=np.uint32)
            if keep_words.size != n:
                raise ValueError(f"words must hold one entry per id: {keep_words.size} for {n} ids")
            if not keep_words.size:
                keep_words = np.zeros(1, np.uint32)  # (no ids: never read, but not NULL -- the words are given)
            wptr = c_void_p(keep_words.ctypes.data)
        m = Mask(int(seed), int(first_doc), int(select), int(mask), int(random), int(mask_id), int(n_random), int(ignore),
                 int(flags) | (MASK_WHOLE_WORD if whole_word else 0))
        di, dl = c_void_p(), c_void_p()
        self._chk(lib().yabpe_mask(self._h, ptr, n, dptr, nd, wptr, byref(m), byref(di), byref(dl)))
        return di.value or 0, dl.value or 0

    def mask_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, words=None, **kw):
        """-> (inputs u32[n_ids], labels i32[n_ids]) copied to the host."""
        n = int(n_ids) if isinstance(ids, int) else int(np.size(ids))
        di, dl = self.mask(ids, n_ids, doc_starts, n_docs, words, **kw)
        if not n:
            return np.zeros(0, np.uint32), np.zeros(0, np.int32)
        return self.d2h(di, 4 * n, np.uint32), self.d2h(dl, 4 * n, np.uint32).view(np.int32)

    def mask_free(self) -> None:
        self._chk(lib().yabpe_mask_free(self._h))

    def mask_stats(self) -> dict:
        s = MaskStats()
        self._chk(lib().yabpe_mask_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- span-corruption batches (BBPETokenizer.corrupt_spans on the device)
    def span_corrupt(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, words=None, *, sentinels, seed: int = 0,
                     first_doc: int = 0, open: int = 0, lens=(), max_len: int | None = None, max_doc_ids: int = 0, whole_word: bool = False,
                     final_sentinel: bool = False, flags: int = 0):
        """One span-corruption draw over ragged ids (yabpe_span_corrupt).  ids / doc_starts / words as mask takes them.  open,
        lens: the thresholds To and C[0 .. max_len - 2] (BBPETokenizer.span_thresholds); max_len None: len(lens) + 1.
        sentinels: the u32 table.  flags: further YABPE_SPAN_* bits as they are.
        -> (dev_in_ptr u32[n_in], dev_in_off_ptr u64[n_docs + 1], n_in, dev_tgt_ptr u32[n_tgt], dev_tgt_off_ptr u64[n_docs + 1], n_tgt,
        n_docs); the buffers live until the next span_corrupt, span_free() or close()."""
        keep = docs = keep_words = None
        if isinstance(ids, int):
            ptr, n = c_void_p(ids), int(n_ids)
        else:
            keep = np.ascontiguousarray(ids, dtype=np.uint32)
            ptr, n = c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)
        if isinstance(doc_starts, int):
            dptr, nd = c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        if words is None or isinstance(words, int):
            wptr = c_void_p(words or 0)
        else:
            keep_words = np.ascontiguousarray(words, dtype=np.uint32)
            if keep_words.size != n:
                raise ValueError(f"words must hold one entry per id: {keep_words.size} for {n} ids")
            if not keep_words.size:
                keep_words = np.zeros(1, np.uint32)  # (no ids: never read, but not NULL -- the words are given)
            wptr = c_void_p(keep_words.ctypes.data)
        lens = [int(x) for x in lens]
        if len(lens) > SPAN_MAX_LEN - 1:
            raise ValueError(f"at most {SPAN_MAX_LEN - 1} length thresholds, not {len(lens)}")
        sent = np.ascontiguousarray(sentinels, dtype=np.uint32).ravel()
        sp = Span(int(seed), int(first_doc), int(open), (c_uint64 * 31)(*lens), len(lens) + 1 if max_len is None else int(max_len), int(sent.size),
                  c_void_p(sent.ctypes.data if sent.size else 0), int(max_doc_ids),
                  int(flags) | (SPAN_WHOLE_WORD if whole_word else 0) | (SPAN_FINAL_SENTINEL if final_sentinel else 0))
        di, dio, dt, dto, ni, nt = c_void_p(), c_void_p(), c_void_p(), c_void_p(), c_uint64(), c_uint64()
        self._chk(lib().yabpe_span_corrupt(self._h, ptr, n, dptr, nd, wptr, byref(sp), byref(di), byref(dio), byref(ni), byref(dt), byref(dto),
                                           byref(nt)))
        return di.value or 0, dio.value or 0, int(ni.value), dt.value or 0, dto.value or 0, int(nt.value), nd

    def span_corrupt_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, words=None, **kw):
        """-> (inputs u32[n_in], in_off u64[n_docs + 1], targets u32[n_tgt], tgt_off u64[n_docs + 1]) copied to the host."""
        di, dio, ni, dt, dto, nt, nd = self.span_corrupt(ids, n_ids, doc_starts, n_docs, words, **kw)
        rag = lambda p, n: self.d2h(p, 4 * n, np.uint32) if n else np.zeros(0, np.uint32)  # noqa: E731
        return rag(di, ni), self.d2h(dio, 8 * (nd + 1), np.uint64), rag(dt, nt), self.d2h(dto, 8 * (nd + 1), np.uint64)

    def span_free(self) -> None:
        self._chk(lib().yabpe_span_free(self._h))

    def span_stats(self) -> dict:
        s = SpanStats()
        self._chk(lib().yabpe_span_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- fill-in-the-middle batches (BBPETokenizer.fim_tokens / fim_cuts on the device)
    @staticmethod
    def _fim_arg(seed=0, first_doc=0, fim=0, spm=0, pre_id=0, suf_id=0, mid_id=0, eot_id=None, ignore=MASK_IGNORE, max_len=0,
                 loss_middle=False, pieces=False, flags=0) -> Fim:
        return Fim(int(seed), int(first_doc), int(fim), int(spm), int(pre_id), int(suf_id), int(mid_id), int(eot_id or 0), int(ignore), int(max_len),
                   int(flags) | (0 if eot_id is None else FIM_EOT) | (FIM_LOSS_MIDDLE if loss_middle else 0) | (FIM_PIECES if pieces else 0))

    def fim_cuts(self, text, n_bytes: int | None = None, doc_starts=None, n_docs: int | None = None, **kw):
        """The character-level cuts of every document (yabpe_fim_cuts).  text as encode takes it; doc_starts: a u64 table
        (staged) or a device address with n_docs.  kw: seed, first_doc, fim, spm (the thresholds Tf, Ts), flags.
        -> (dev_piece_off_ptr u64[3 * n_docs], dev_cuts_ptr u64[3 * n_docs], n_docs); the buffers live until the next
        fim_cuts, fim_free() or close()."""
        _keep, ptr, n = _text_arg(text, n_bytes)
        if isinstance(doc_starts, int):
            docs, dptr, nd = None, c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        f = self._fim_arg(**kw)
        po, cu = c_void_p(), c_void_p()
        self._chk(lib().yabpe_fim_cuts(self._h, ptr, n, dptr, nd, byref(f), byref(po), byref(cu)))
        return po.value or 0, cu.value or 0, nd

    def fim_cuts_to_host(self, text, n_bytes: int | None = None, doc_starts=None, n_docs: int | None = None, **kw):
        """-> (piece_off u64[n_docs, 3], cuts u64[n_docs, 3]) copied to the host."""
        po, cu, nd = self.fim_cuts(text, n_bytes, doc_starts, n_docs, **kw)
        return self.d2h(po, 24 * nd, np.uint64).reshape(nd, 3), self.d2h(cu, 24 * nd, np.uint64).reshape(nd, 3)

    def fim(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, cuts=None, **kw):
        """One fill-in-the-middle rearrangement of ragged ids (yabpe_fim).  ids / doc_starts as mask takes them (doc_starts 0
        with n_docs: a NULL table); cuts: None, a u64 array (staged) or a device address -- what fim_cuts returns, with
        pieces=True.  kw: seed, first_doc, fim, spm, pre_id, suf_id, mid_id, eot_id (None: no eot), ignore, max_len,
        loss_middle, pieces, flags (further YABPE_FIM_* bits as they are).
        -> (dev_ids_ptr u32[n_out], dev_labels_ptr u32[n_out], dev_off_ptr u64[n_out_docs + 1], dev_info_ptr u32[n_out_docs, 4],
        n_out, n_out_docs); the buffers live until the next fim, fim_free() or close()."""
        keep = docs = keep_cuts = None
        if isinstance(ids, int):
            ptr, n = c_void_p(ids), int(n_ids)
        else:
            keep = np.ascontiguousarray(ids, dtype=np.uint32)
            ptr, n = c_void_p(keep.ctypes.data if keep.size else 0), int(keep.size)
        if isinstance(doc_starts, int):
            dptr, nd = c_void_p(doc_starts), int(n_docs)
        else:
            docs = _starts_arg(doc_starts)
            dptr, nd = c_void_p(docs.ctypes.data), len(docs)
        if cuts is None or isinstance(cuts, int):
            cptr = c_void_p(cuts or 0)
        else:
            keep_cuts = np.ascontiguousarray(cuts, dtype=np.uint64).ravel()
            cptr = c_void_p(keep_cuts.ctypes.data)
        f = self._fim_arg(**kw)
        di, dl, do, dn, no = c_void_p(), c_void_p(), c_void_p(), c_void_p(), c_uint64()
        self._chk(lib().yabpe_fim(self._h, ptr, n, dptr, nd, cptr, byref(f), byref(di), byref(dl), byref(do), byref(dn), byref(no)))
        return di.value or 0, dl.value or 0, do.value or 0, dn.value or 0, int(no.value), nd // 3 if f.flags & FIM_PIECES else nd

    def fim_to_host(self, ids, n_ids: int | None = None, doc_starts=None, n_docs: int | None = None, cuts=None, **kw):
        """-> (ids u32[n_out], labels i32[n_out], off u64[n_out_docs + 1], info u32[n_out_docs, 4]) copied to the host."""
        di, dl, do, dn, no, nd = self.fim(ids, n_ids, doc_starts, n_docs, cuts, **kw)
        rag = lambda p: self.d2h(p, 4 * no, np.uint32) if no else np.zeros(0, np.uint32)  # noqa: E731
        info = self.d2h(dn, 16 * nd, np.uint32).reshape(nd, 4) if nd else np.zeros((0, 4), np.uint32)
        return rag(di), rag(dl).view(np.int32), self.d2h(do, 8 * (nd + 1), np.uint64), info

    def fim_free(self) -> None:
        self._chk(lib().yabpe_fim_free(self._h))

    def fim_stats(self) -> dict:
        s = FimStats()
        self._chk(lib().yabpe_fim_stats(self._h, byref(s)))
        return _stats_dict(s)

    # -- the persistent word pool (corpora larger than device memory: words go in call by call, the merge loop loads the pool)
    def pool_add(self, flat, off, freq=None) -> None:
        """Adds the words' counts to the context's pool.  flat: u8 bytes, off: u64 offsets (n + 1), freq: optional u64
        counts (None: every word counts once) -- host arrays, as load_words takes them."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(off) - 1, 0)
        fq = None
        if freq is not None:
            fq = np.ascontiguousarray(freq, dtype=np.uint64)
            assert len(fq) == n
        self._chk(lib().yabpe_pool_add(self._h, flat.ctypes.data if flat.size else None, off.ctypes.data if off.size else None,
                                       fq.ctypes.data if fq is not None and fq.size else None, n))

    def pool_add_ptr(self, bytes_ptr: int, off_ptr: int, n_words: int, freq_ptr: int = 0) -> None:
        """Device (or host) addresses, e.g. the results of pretokenize()."""
        self._chk(lib().yabpe_pool_add(self._h, c_void_p(bytes_ptr) if bytes_ptr else None, c_void_p(off_ptr) if off_ptr else None,
                                       c_void_p(freq_ptr) if freq_ptr else None, n_words))

    def pool_get(self):
        """-> (dev_bytes_ptr, dev_off_ptr u64[n_unique + 1], dev_freq_ptr u64[n_unique], n_unique, n_bytes): what
        load_words_ptr(bytes, off, n_unique, freq) takes; valid until the next pool_add, pool_clear() or close().  The pool
        may be cleared as soon as the load has returned."""
        pb, po, pf, nu, nb = c_void_p(), c_void_p(), c_void_p(), c_uint64(0), c_uint64(0)
        self._chk(lib().yabpe_pool_get(self._h, byref(pb), byref(po), byref(pf), byref(nu), byref(nb)))
        return pb.value or 0, po.value or 0, pf.value or 0, nu.value, nb.value

    def pool_items(self) -> dict:
        """The pool copied to the host as {word bytes: count} (tests and small pools)."""
        pb, po, pf, nu, nb = self.pool_get()
        if not nu:
            return {}
        off = self.d2h(po, 8 * (nu + 1), np.uint64).tolist()
        cnt = self.d2h(pf, 8 * nu, np.uint64).tolist()
        blob = self.d2h(pb, nb).tobytes()
        return {blob[a:b]: k for a, b, k in zip(off[:-1], off[1:], cnt)}

    def pool_clear(self) -> None:
        self._chk(lib().yabpe_pool_clear(self._h))

    def pool_stats(self) -> dict:
        s = PoolStats()
        self._chk(lib().yabpe_pool_stats(self._h, byref(s)))
        return _stats_dict(s)

    def h2d(self, dev_ptr: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr)
        self._chk(lib().yabpe_memcpy_h2d(self._h, c_void_p(dev_ptr), arr.ctypes.data, arr.nbytes))

    # -- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (c_uint8 * 128)()
        rc = lib().yabpe_comm_unique_id(buf)
        if rc != 0:
            raise YabpeError(rc, lib().yabpe_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, rank: int, n_ranks: int, unique_id: bytes) -> None:
        """RCCL transport (one process per GPU).  Call before load_words."""
        assert len(unique_id) == 128
        buf = (c_uint8 * 128).from_buffer_copy(unique_id)
        self._chk(lib().yabpe_comm_init(self._h, rank, n_ranks, buf))

    def comm_init_custom(self, rank: int, n_ranks: int, allgather) -> None:
        """Custom transport: allgather(send_dev_ptr, recv_dev_ptr, nbytes) -> 0 on success."""
        def _cb(_user, send, recv, nbytes):
            try:
                return int(allgather(send, recv, nbytes) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return -1
        self._ag_cb = ALLGATHER_FN(_cb)  # keep alive
        self._chk(lib().yabpe_comm_init_custom(self._h, rank, n_ranks, self._ag_cb, None))

    def comm_enable_p2p(self) -> None:
        """Peer-to-peer exchange (hipIpc-mapped receive buffers) instead of the all-gather; collective."""
        self._chk(lib().yabpe_comm_enable_p2p(self._h))

    def d2h(self, dev_ptr: int, nbytes: int, dtype=np.uint8) -> np.ndarray:
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._chk(lib().yabpe_memcpy_d2h(self._h, out.ctypes.data, c_void_p(dev_ptr), nbytes))
        return out


def encode_model_arrays(vocab: dict, merges, specials_ordered) -> dict:
    """The flat arrays of yabpe_encode_set_model: vocab bytes / u64 offsets / u32 ids, merges as 2 n + 1 u64 offsets
    (left, right, left, right ...), specials' bytes / u32 offsets."""
    def flat(items, dtype):
        blob = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8).copy()
        off = np.zeros(len(items) + 1, dtype=dtype)
        if items:
            off[1:] = np.cumsum([len(x) for x in items])
        return blob, off

    toks = list(vocab)
    vb, vo = flat(toks, np.uint64)
    vi = np.asarray([vocab[t] for t in toks] or [0], dtype=np.uint32)[:len(toks)]
    mb, mo = flat([x for pair in merges for x in pair], np.uint64)
    sb, so = flat([t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in specials_ordered], np.uint32)
    return {"vb": vb, "vo": vo, "vi": np.ascontiguousarray(vi), "mb": mb, "mo": mo, "sb": sb, "so": so}


def decode_model_arrays(vocab: dict) -> dict:
    """The flat arrays of yabpe_decode_set_model, in dict order: vocab bytes / u64 offsets / u32 ids.  An id outside
    [0, 2^32) raises YabpeError(E_CAPACITY) (the device table holds ids below 2^24)."""
    toks = list(vocab)
    for t in toks:
        if not 0 <= vocab[t] < 1 << 32:
            raise YabpeError(E_CAPACITY, f"token id {vocab[t]} of {t!r}: the decode table holds ids below 2^24")
    blob = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8).copy()
    off = np.zeros(len(toks) + 1, dtype=np.uint64)
    if toks:
        off[1:] = np.cumsum([len(t) for t in toks])
    vi = np.asarray([vocab[t] for t in toks] or [0], dtype=np.uint32)[:len(toks)]
    return {"vb": blob, "vo": off, "vi": np.ascontiguousarray(vi)}


def merge_triples(base_tokens, merges):
    """Replays `merges` [(bytes, bytes)] over the base token list as BBPETrainer._decode_merges does: -> (tokens in id order,
    (left, right, merged) u32 arrays).  l + r gets the next id unless those bytes are a token already (trainer.py:298-300).
    Raises ValueError when an operand is not a token at that point."""
    toks = list(base_tokens)
    ids = {t: i for i, t in enumerate(toks)}
    left = np.zeros(len(merges), dtype=np.uint32)
    right = np.zeros(len(merges), dtype=np.uint32)
    merged = np.zeros(len(merges), dtype=np.uint32)
    for k, (l, r) in enumerate(merges):
        l, r = bytes(l), bytes(r)
        for side in (l, r):
            if side not in ids:
                raise ValueError(f"merge {k} names {side!r}, which is not a token when that merge is replayed")
        m = ids.get(l + r)
        if m is None:
            m = ids[l + r] = len(toks)
            toks.append(l + r)
        left[k], right[k], merged[k] = ids[l], ids[r], m
    return toks, (left, right, merged)


def decode_merges(base_tokens, left, right, merged):
    """The inverse of merge_triples: (left, right, merged) id arrays over the base token list -> ({token: id}, [(bytes, bytes)])."""
    toks = list(base_tokens)
    merges: list[tuple[bytes, bytes]] = []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        merges.append((toks[l], toks[r]))
        if m == len(toks):  # a fresh id; otherwise the bytes already existed (trainer.py:298-300)
            toks.append(toks[l] + toks[r])
        else:
            assert toks[m] == toks[l] + toks[r], "merged id does not name left+right"
    return {t: i for i, t in enumerate(toks)}, merges


def train_words(words_flat, words_off, freq, base_tokens: list[bytes], num_merges: int, min_frequency: int,
                dedup: bool = False, options: dict | None = None, want_stats: bool = False):
    """Convenience used by tests/bench: returns (vocab, merges[, stats]) like _merge_loop."""
    with Context() as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        ctx.set_vocab(base_tokens)
        ctx.load_words(words_flat, words_off, freq, dedup=dedup)
        left, right, merged, count = ctx.train(num_merges, min_frequency)
        stats = ctx.stats() if want_stats else None
    vocab, merges = decode_merges(base_tokens, left, right, merged)
    return (vocab, merges, stats) if want_stats else (vocab, merges)
