"""GPU (-m gpu): the branches of the multi-rank exchange that tests/test_gpu_distributed.py does not reach, with two and four
ranks on the one GPU of the test box (tests/exchange_workers.py: several jobs on ONE context per spawn).

- A job leaves the peer-to-peer exchange while it runs: the exchange buffers start at 4 records and are reallocated up to the
  capacity C the "torch" control reports; mapped areas of 4, 16 or 64 records (p2p_cap_records) are outgrown at the first,
  second or third reallocation (tests/test_exchange_inputs.py holds the bounds), and the job goes on through the transport.
  The stats tell that the switch happened: exchange_p2p flips 1 -> 0 exactly where the control's capacity predicts it,
  exchanges were event-timed before the switch (only the peer-to-peer path times them) and none in the job after it.
- A second job on the same context, under peer to peer (the sequence counter and the flag words of job 1 stay) and after a
  fallback (the context stays on the transport, the buffers stay grown).
- Ranks without tiles: long words only, no words at all, one tile -- flat and weighted, both transports.
- The overflow recoveries and the tie-heavy batched selection with four contributors.

Every expected merge list is the CPU oracle's on the whole corpus, every comparison is exact, every rank verifies its replica
of the pair table after every job.  Not covered: the p2p_timeout_ms exit (it needs a peer that never arrives)."""
from __future__ import annotations

import time

import pytest

from oracle import oracle
from tests import dist_workers, exchange_workers as xw, helpers

pytestmark = pytest.mark.gpu
OVERFLOW = {"delta_cap": 4, "check_interval": 5}
TIES = {"split": 1, "batch_max": 16, "cand_min_count": 1}
SHAPES = {"check_interval": 5}  # (an exchange stops carrying whole buffers of 16,384 records after 20 merges, not after 256)
TWO_JOBS = [("corpus_en", 300, None), ("corpus_en_reversed", 200, None)]
EXCHANGE_KEYS = ("exchanges", "exchange_growths", "exchange_cap_records", "exchange_max_records", "exchange_p2p", "table_rebuilds")
_EXPECTED = {}


def expected(name, n_merges):
    if (name, n_merges) not in _EXPECTED:
        words, freq = xw.job_corpus(name, 4)
        flat, off = helpers.flatten(words)
        _EXPECTED[name, n_merges] = oracle.train_flat(flat, off, 257 + n_merges, 1, xw.SP, freq=freq)[1]
    return _EXPECTED[name, n_merges]


def run(world, transport, options, jobs):
    """One spawn.  Checks what holds in every case: every rank returns the oracle's merges and a verified table after every
    job, the ranks agree on what the exchanges did, and the closing comm_enable_p2p() is refused.  -> [job][rank] stats."""
    t0 = time.perf_counter()
    outs = dist_workers.spawn(xw.jobs_on_one_context, world, transport, options, jobs, timeout=300)
    wall = time.perf_counter() - t0
    assert len(outs) == world
    stats = []
    for j, (name, n_merges, _ranges) in enumerate(jobs):
        exp = expected(name, n_merges)
        for rank, (results, _refusal) in enumerate(outs):
            merges, verified, st = results[j]
            assert [(bytes.fromhex(a), bytes.fromhex(b)) for a, b in merges] == exp, (name, rank, st)
            assert verified, (name, rank, st)
        stats.append([results[j][2] for results, _refusal in outs])
        for st in stats[-1]:
            assert {k: st[k] for k in EXCHANGE_KEYS} == {k: stats[-1][0][k] for k in EXCHANGE_KEYS}, stats[-1]
        s = stats[-1][0]
        print(f"[{transport} world {world} {options}] job {j + 1} {name}: exchanges {s['exchanges']} ({'odd' if s['exchanges'] % 2 else 'even'}), "
              f"growths {s['exchange_growths']}, cap {s['exchange_cap_records']}, max records {s['exchange_max_records']}, p2p {s['exchange_p2p']}, "
              f"sampled {[st['exchanges_sampled'] for st in stats[-1]]}, rebuilds {s['table_rebuilds']}")
    for rank, (_results, (code, text)) in enumerate(outs):
        assert code == -1 and xw.REFUSAL in text, (rank, code, text)
    print(f"[{transport} world {world} {options}] spawn of {len(jobs)} job(s): {wall:.1f} s")
    return stats


_CONTROL = {}


def control(world):
    """The first job through the transport alone: the capacity its exchange buffers end at, and how often they grew."""
    if world not in _CONTROL:
        (job,) = run(world, "torch", OVERFLOW, TWO_JOBS[:1])
        _CONTROL[world] = job[0]
    return _CONTROL[world]


@pytest.mark.parametrize("world", [2, 4])
def test_control_through_the_transport(world):
    st = control(world)
    assert st["exchange_p2p"] == 0 and st["exchanges_sampled"] == 0
    assert st["exchange_cap_records"] >= 256  # a rank sends more than 64 records at merge 29: 4 -> 16 -> 64 -> 256 at least
    assert st["exchange_growths"] >= 3 and st["table_rebuilds"] >= 3  # (every growth recounts)
    assert 64 < st["exchange_max_records"] <= st["exchange_cap_records"]


def check_two_jobs(world, area_records):
    cap = control(world)["exchange_cap_records"]
    job1, job2 = run(world, "torch+p2p", {**OVERFLOW, "p2p_cap_records": area_records}, TWO_JOBS)
    roomy = max(4, area_records) >= cap  # (p2p_setup: the areas hold max(delta_cap, p2p_cap_records) records)
    for st in job1:
        # the records per round are the same numbers under both transports: the buffers end at the same capacity
        assert st["exchange_cap_records"] == cap and st["exchange_growths"] == control(world)["exchange_growths"]
        assert st["exchange_p2p"] == (1 if roomy else 0)
        assert st["exchanges_sampled"] > 0  # peer-to-peer exchanges ran (before the switch): only they are event-timed
    for st in job2:
        assert st["exchange_cap_records"] == cap  # nothing shrank ...
        assert st["exchange_p2p"] == (1 if roomy else 0)  # ... and nothing went back to the areas
        assert (st["exchanges_sampled"] > 0) == roomy
        assert st["exchanges"] > 0


@pytest.mark.parametrize("area_records", [1, 16, 64, "roomy"])
def test_two_ranks_leave_the_peer_areas_at_each_reallocation(area_records):
    """Areas of 4 (option 1), 16 and 64 records are outgrown at the first, second and third reallocation; areas of the control's
    capacity never.  Job 2 runs on the same context: after a fallback it stays on the transport, in the roomy case it goes on
    peer to peer with job 1's sequence numbers in the flag words."""
    check_two_jobs(2, control(2)["exchange_cap_records"] if area_records == "roomy" else area_records)


@pytest.mark.parametrize("area_records", [16, "roomy"])
def test_four_ranks_leave_the_peer_areas(area_records):
    check_two_jobs(4, control(4)["exchange_cap_records"] if area_records == "roomy" else area_records)


def test_four_ranks_walk_the_same_window_peer_to_peer():
    """tests/tie_helpers.py's stems through the batched selection, four replicas, the exchange peer to peer."""
    assert 300 <= len(expected("tie_stems", 400)) <= 400
    (job,) = run(4, "torch+p2p", TIES, [("tie_stems", 400, None)])
    for st in job:
        assert st["n_words"] > 0 and st["exchange_p2p"] == 1 and st["exchanges_sampled"] > 0


@pytest.mark.parametrize("world,transport", [(4, "torch"), (4, "torch+p2p"), (2, "torch+p2p")])
def test_ranks_without_tiles(world, transport):
    """Rank 0 holds only long words (no tile, but records to send), at four ranks rank 1 holds nothing and rank 3 one tile;
    job 1 flat (dense histogram + the long-word exchange at the initial count), job 2 weighted (the generic table exchange).
    (When this test was written rank 0 came back with 8 and 3 empty tiles: the load sized the tile stream by the shard's bytes,
    long words included, so no rank with records to send was ever without tiles.  The load now drops tiles that hold no word.)"""
    p2p = 1 if transport.endswith("+p2p") else 0
    flat, weighted = (xw.shapes_corpus(layout, world)[2] for layout in ("flat", "weighted"))
    jobs = run(world, transport, SHAPES, [("shapes_flat", xw.SHAPES_MERGES, flat), ("shapes_weighted", xw.SHAPES_MERGES, weighted)])
    for job, n_long in zip(jobs, (9, 3)):  # (the weighted layout pools the nine long words into three)
        assert job[0]["n_tiles"] == 0 and job[0]["n_long_words"] == n_long and job[0]["n_words"] == n_long
        for st in job[1:]:
            assert st["n_long_words"] == 0
        if world == 4:
            assert job[1]["n_words"] == 0 and job[1]["n_tiles"] == 0
            assert job[2]["n_words"] > 500 and job[2]["n_tiles"] >= 1
            assert job[3]["n_words"] == 1 and job[3]["n_tiles"] == 1
        else:
            assert job[1]["n_words"] > 500 and job[1]["n_tiles"] >= 1
        for st in job:
            assert st["exchange_p2p"] == p2p and (st["exchanges_sampled"] > 0) == bool(p2p) and st["exchanges"] > 0


@pytest.mark.parametrize("layout", ["flat", "weighted"])
def test_one_rank_with_long_words_only(layout):
    """The same shape without a communicator: a context whose words are all long ones keeps no tile (until these tests the load
    left it the empty tiles counted for the words' bytes), selects on its own and applies with k_apply_long alone."""
    from yet_another_bpe import _native

    words, freq = xw.LONG_WORDS, None
    if layout == "weighted":
        words, freq = helpers.pooled(words)
    flat, off = helpers.flatten(words)
    exp = oracle.train_flat(flat, off, 257 + 40, 1, xw.SP, freq=freq)[1]
    assert 5 <= len(exp) < 40  # (the three words fold in halves, a few merges each; then no pair is left: the job runs dry)
    base = helpers.base_tokens(xw.SP)
    with _native.Context(0) as ctx:
        ctx.set_option("verify", 1)
        ctx.set_vocab(base)
        ctx.load_words(flat, off, freq)
        left, right, merged, _count = ctx.train(40, 1)
        st = ctx.stats()
        assert ctx.verify_table() == 0
    assert _native.decode_merges(base, left, right, merged)[1] == exp
    assert st["n_tiles"] == 0 and st["n_long_words"] == len(words) == st["n_words"]
