"""CPU: the plain-Python contract BBPETokenizer.fit_labelled on hand-made batches -- rows as encode_batch_fit's, the two label
forms, mask_first, the seam records, the right cut, and the refused arguments."""
from __future__ import annotations

import pytest

from tests import layout_helpers as lh

TOK = lh.GivenIds()
IGN, C = -100, 8
BATCHES = {  # sequence lengths: every edge of a row of 8, several sequences a row, empty ones, none at all
    "edges": [0, 1, 2, 7, 8, 11],
    "several-a-row": [3, 3, 2, 5, 1, 1, 4, 0, 2],
    "one": [5],
    "only-empty": [0, 0],
    "none": [],
}


def batch(lens):
    """ids 100 s + p, labels 1000 + the id but `ignore` at every third position"""
    ids = [[100 * s + p for p in range(n)] for s, n in enumerate(lens)]
    return ids, [[IGN if p % 3 == 1 else 1000 + t for p, t in enumerate(seq)] for seq in ids]


@pytest.mark.parametrize("name", list(BATCHES))
def test_rows_labels_and_seams(name):
    ids, labels = batch(BATCHES[name])
    al = TOK.fit_labelled(ids, labels, C, pad_id=9, labels="aligned", mask_first=False)
    assert (al["ids"], al["seq"], al["pos"], al["used"]) == TOK.encode_batch_fit(ids, C, pad_id=9)
    sh, first = (TOK.fit_labelled(ids, labels, C, pad_id=9, labels=form, mask_first=True) for form in ("shifted", "aligned"))
    assert TOK.fit_labelled(ids, labels, C, pad_id=9, mask_first=False) == sh  # shifted is the default, mask_first has no effect on it
    for r, (seq, pos) in enumerate(zip(al["seq"], al["pos"])):
        for c in range(C):
            end = c + 1 == C or seq[c + 1] != seq[c] or seq[c] == 0xFFFFFFFF  # the last slot of its sequence, or a pad
            assert sh["labels"][r][c] == (IGN if end else al["labels"][r][c + 1])
            assert first["labels"][r][c] == (IGN if pos[c] == 0 else al["labels"][r][c])
            if seq[c] != 0xFFFFFFFF:
                assert al["labels"][r][c] == labels[seq[c]][pos[c]]
        recs = al["placed"][al["row_first"][r]:al["row_first"][r + 1]]  # the records reproduce every slot's (seq, pos)
        slots = [(s, p) for s, col, n in recs for p in range(n)]
        assert [col for _s, col, _n in recs] == [sum(n for _s, _c, n in recs[:k]) for k in range(len(recs))]
        assert slots + [(0xFFFFFFFF, 0)] * (C - len(slots)) == list(zip(seq, pos)) and al["used"][r] == len(slots)
        for out in (al, sh, first):
            assert out["labelled"][r] == sum(t != IGN for t in out["labels"][r])
    assert len(al["row_first"]) == len(al["ids"]) + 1 and al["row_first"][-1] == len(al["placed"]) == sum(n > 0 for n in BATCHES[name])


def test_an_over_long_sequence_is_cut_on_the_right():
    ids, labels = [list(range(50, 61))], [list(range(150, 161))]
    out = TOK.fit_labelled(ids, labels, C, pad_id=0)
    assert out["ids"] == [ids[0][:C]] and out["labels"] == [labels[0][1:C] + [IGN]] and out["placed"] == [(0, 0, C)]


@pytest.mark.parametrize("bad", [{"seq_len": 0}, {"seq_len": 1 << 24}, {"seq_len": 2.5}, {"labels": "left"}, {"ignore": 1 << 31}, {"pad_id": -1},
                                 {"labels_batch": [[1]]}, {"labels_batch": [[1, 2], []]}])
def test_refused_arguments(bad):
    args = {"ids_batch": [[1, 2]], "labels_batch": [[1, 2]], "seq_len": 4, **bad}
    with pytest.raises(ValueError):
        TOK.fit_labelled(args.pop("ids_batch"), args.pop("labels_batch"), args.pop("seq_len"), **args)
