"""Workers for the multi-rank tests of the text options (spawned by tests/dist_workers.spawn: gloo on 127.0.0.1, the ranks
share one GPU and exchange through the custom transport).  The configurations are tests/text_dist_helpers.py's."""
from __future__ import annotations


def gpu_text_options(rank, world, dist, path, names):
    """train_text_sharded over the file for each named configuration in turn (one spawn pays the start-up once; the first
    exception ends the worker).  -> {name: (merges as hex pairs, vocabulary size)}"""
    from tests import text_dist_helpers as th
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import train_text_sharded

    out = {}
    for name in names:
        model = train_text_sharded(lambda: _native.Context(0), [path], th.config(name), rank, world, transport="torch", options={"verify": 1})
        out[name] = ([(a.hex(), b.hex()) for a, b in model.merges], len(model.vocab))
    return out


def gpu_text_error(rank, world, dist, path, cfg_kwargs):
    """-> str(e) of the ValueError the driver raises on this rank, or None"""
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import train_text_sharded
    from yet_another_bpe.trainer import BBPETrainerConfig

    try:
        train_text_sharded(lambda: _native.Context(0), [path], BBPETrainerConfig(**cfg_kwargs), rank, world, transport="torch", options={"verify": 1})
    except ValueError as e:
        return str(e)
    return None


def gpu_device_text_options(rank, world, dist, path, name, chunk_size):
    """train_device_text_sharded over a device copy of the file's bytes (a torch tensor, alive for the call): every rank gets
    the address of the whole text and pre-tokenises its chunks from there.  -> (merges as hex pairs, pre-tokens here)"""
    from pathlib import Path

    import numpy as np
    import torch

    from tests import text_dist_helpers as th
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import train_device_text_sharded

    cfg = th.config(name, chunk_size_bytes=chunk_size)
    text = torch.from_numpy(np.frombuffer(Path(path).read_bytes(), np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    left, right, merged, _count, _stats, n_words = train_device_text_sharded(lambda: _native.Context(0), lambda ctx: (text.data_ptr(), text.numel()), cfg, rank, world,
                                                                              transport="torch", options={"verify": 1})
    del text
    toks = [bytes([b]) for b in range(256)] + [t.encode() for t in cfg.special_tokens]
    out = []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        out.append((toks[l].hex(), toks[r].hex()))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
    return out, int(n_words)
