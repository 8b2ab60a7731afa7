"""engine.collapse_lists: the rule of segvlad_search_grouped stated on the host (the yardstick of tests/test_gpu_group.py), on
hand-written lists."""
import numpy as np
import pytest

from revisit_anything_amd.engine import collapse_lists


def _lists(rows):
    """rows: per query row a list of (d2, id) pairs; padded with (+inf, -1) to one length."""
    L = max(len(r) for r in rows)
    d2 = np.full((len(rows), L), np.inf, np.float32)
    idx = np.full((len(rows), L), -1, np.int64)
    for q, r in enumerate(rows):
        for j, (d, i) in enumerate(r):
            d2[q, j], idx[q, j] = d, i
    return d2, idx


#                    row id:  0  1  2  3  4  5  6  7   8   9
IMG = np.array([3, 3, 3, 5, 5, 9, 9, 9, -1, -7], np.int32)


def test_counts_per_image():
    d2, idx = _lists([[(0.1, 0), (0.2, 1), (0.3, 3), (0.4, 2), (0.5, 4), (0.6, 5), (0.7, 6), (0.8, 7)]])
    od, oi = collapse_lists(d2, idx, IMG, 8, 1)
    assert oi[0].tolist() == [0, 3, 5, -1, -1, -1, -1, -1]
    assert od[0, :3].tolist() == [np.float32(0.1), np.float32(0.3), np.float32(0.6)] and np.isinf(od[0, 3:]).all()
    od, oi = collapse_lists(d2, idx, IMG, 8, 2)
    assert oi[0].tolist() == [0, 1, 3, 4, 5, 6, -1, -1]
    # k cuts the kept entries, not the list: the third kept entry of per_image = 1 sits at list position 5
    od, oi = collapse_lists(d2, idx, IMG, 2, 1)
    assert oi[0].tolist() == [0, 3] and od.dtype == np.float32 and oi.dtype == np.int64
    # every row on its own
    d2, idx = _lists([[(0.1, 0), (0.2, 1), (0.3, 3)], [(0.0, 4), (0.2, 3), (0.3, 0)]])
    od, oi = collapse_lists(d2, idx, IMG, 2, 1)
    assert oi.tolist() == [[0, 3], [4, 0]]


def test_negative_ids_are_always_kept():
    d2, idx = _lists([[(0.1, 8), (0.2, 8), (0.3, 9), (0.4, 0), (0.5, 9), (0.6, 1), (0.7, 8)]])
    od, oi = collapse_lists(d2, idx, IMG, 7, 1)
    assert oi[0].tolist() == [8, 8, 9, 0, 9, 8, -1]
    assert od[0, 5] == np.float32(0.7)


def test_padding_in_and_out():
    # padding slots of the input are skipped (not kept, and they do not end the walk early for the entries before them)
    d2, idx = _lists([[(0.1, 0), (0.2, 3)], [(0.1, 5), (0.2, 6), (0.3, 0), (0.4, 3)]])
    od, oi = collapse_lists(d2, idx, IMG, 3, 1)
    assert oi.tolist() == [[0, 3, -1], [5, 0, 3]]
    assert np.isinf(od[0, 2]) and od[0, 2] > 0
    # an empty list
    od, oi = collapse_lists(np.zeros((2, 0), np.float32), np.zeros((2, 0), np.int64), IMG, 2, 1)
    assert (oi == -1).all() and np.isinf(od).all()


def test_per_image_at_least_the_largest_group_is_the_identity():
    rng = np.random.default_rng(0)
    ids = np.stack([rng.permutation(8) for _ in range(5)]).astype(np.int64)
    d2 = np.sort(rng.random((5, 8)).astype(np.float32), axis=1)
    for m in (3, 4, 16):
        od, oi = collapse_lists(d2, ids, IMG, 8, m)
        assert np.array_equal(oi, ids) and np.array_equal(od.view(np.uint32), d2.view(np.uint32))
    od, oi = collapse_lists(d2, ids, IMG, 5, 3)
    assert np.array_equal(oi, ids[:, :5])
    # all image ids distinct: per_image = 1 is the identity
    od, oi = collapse_lists(d2, ids, np.arange(8)[::-1], 8, 1)
    assert np.array_equal(oi, ids)


def test_ties_in_distance_keep_id_order():
    # the list is ordered by (d2, lower id): among equal distances the entry that comes first in the LIST is the earlier one
    d2, idx = _lists([[(0.5, 1), (0.5, 2), (0.5, 4), (0.5, 6), (0.5, 7)]])
    od, oi = collapse_lists(d2, idx, IMG, 5, 1)
    assert oi[0].tolist() == [1, 4, 6, -1, -1]
    od, oi = collapse_lists(d2, idx, IMG, 5, 2)
    assert oi[0].tolist() == [1, 2, 4, 6, 7]


def test_bad_input():
    d2, idx = _lists([[(0.1, 0)]])
    with pytest.raises(ValueError):
        collapse_lists(d2, idx[:, :0], IMG, 1, 1)
    with pytest.raises(ValueError):
        collapse_lists(d2, idx + 10, IMG, 1, 1)
    with pytest.raises(ValueError):
        collapse_lists(d2, idx, IMG, 0, 1)
    with pytest.raises(ValueError):
        collapse_lists(d2, idx, IMG, 1, 0)
