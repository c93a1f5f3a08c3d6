"""Worker for tests/test_gpu_exchange.py: several training jobs on ONE multi-rank context (the exchange buffers, the
peer-to-peer areas, their flag words and sequence counter outlive a job), with explicit word ranges per rank where a job
names them.  Also the corpora of those jobs, shared with tests/test_exchange_inputs.py."""
from __future__ import annotations

from tests import dist_workers  # (the sys.path set-up and spawn live there)

SP = ["<|endoftext|>"]
REFUSAL = "enable the peer-to-peer exchange before yabpe_load_words"
STATS = ("n_words", "n_tiles", "n_long_words", "exchanges", "exchange_growths", "exchange_cap_records", "exchange_max_records",
         "exchange_p2p", "exchanges_sampled", "table_rebuilds")
LONG_WORDS = [b" " * 900, b"ab" * 700, b"xyz" * 50] * 3  # more than 63 tokens each: outside the tile stream
LONE_WORD = b"  "  # rank 3's only word: its pair is one that rank 0's long words hold too
SHORT_SLICE = (4000, 6000)  # the words of corpus.en that rank 2 holds
SHAPES_MERGES = 120


def shapes_corpus(layout: str, world: int = 4):
    """-> (words, freq or None, ranges): rank 0 holds only long words, rank 1 nothing, rank 2 only short words, rank 3 one
    two-byte word; at world 2: long words only | everything else.  layout "weighted": equal words pooled, with frequencies."""
    from tests import helpers

    short = helpers.corpus_en_words()[SHORT_SLICE[0]:SHORT_SLICE[1]]
    words, freq = LONG_WORDS + short + [LONE_WORD], None
    n_long = len(LONG_WORDS)
    if layout == "weighted":
        words, freq = helpers.pooled(words)  # (first occurrences in order: the long words stay in front, the lone word last)
        n_long = len(set(LONG_WORDS))
    else:
        assert layout == "flat", layout
    n = len(words)
    if world == 4:
        ranges = [(0, n_long), (n_long, n_long), (n_long, n - 1), (n - 1, n)]
    else:
        assert world == 2, world
        ranges = [(0, n_long), (n_long, n)]
    return words, freq, ranges


def job_corpus(name: str, world: int):
    """-> (words, freq or None) of a job's corpus, whole: every rank builds the same one."""
    from tests import helpers

    if name == "corpus_en":
        return helpers.corpus_en_words(), None
    if name == "corpus_en_reversed":
        return helpers.corpus_en_words()[::-1], None
    if name == "tie_stems":
        from tests import tie_helpers

        return tie_helpers.stems(), None
    if name.startswith("shapes_"):
        return shapes_corpus(name[len("shapes_"):], world)[:2]
    raise ValueError(name)


def jobs_on_one_context(rank, world, dist, transport, options, jobs):
    """jobs: [(corpus name, n_merges, ranges), ...], run in order on one context; ranges: the word range (w0, w1) of every rank,
    or None for plan_shards.  -> ([(merges as hex pairs, table verified, stats) per job], (code, text) of a comm_enable_p2p()
    after the last job: the context holds words, so it must refuse)."""
    from tests import helpers
    from yet_another_bpe import _native
    from yet_another_bpe.distributed import attach, plan_shards

    base = helpers.base_tokens(SP)
    out = []
    with _native.Context(0) as ctx:
        for k, v in {**options, "verify": 1}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(base)
        attach(ctx, rank, world, transport)
        for n, (name, n_merges, ranges) in enumerate(jobs):
            words, freq = job_corpus(name, world)
            flat, off = helpers.flatten(words)
            w0, w1 = (ranges or plan_shards(off, world))[rank]
            if n:
                ctx.set_vocab(base)  # (resets tokens and merge state; the communicator and its buffers stay)
            ctx.load_words(flat, off[w0:w1 + 1], None if freq is None else freq[w0:w1])
            left, right, merged, _count = ctx.train(n_merges, 1)
            st = ctx.stats()
            mism = ctx.verify_table()
            toks, merges = list(base), []
            for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
                merges.append((toks[l].hex(), toks[r].hex()))
                if m == len(toks):
                    toks.append(toks[l] + toks[r])
            out.append((merges, mism == 0, {k: int(st[k]) for k in STATS}))
        try:
            ctx.comm_enable_p2p()
            refusal = (0, "")
        except _native.YabpeError as e:
            refusal = (e.code, str(e))
    return out, refusal
