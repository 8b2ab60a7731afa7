"""Host side of the range search (revisit_anything_amd/engine.py): range_from_topk against a brute-force model (strictness at
attained values, planted exact ties, degenerate radii, the "list too shallow" error), radius2_from_sim, range_image_counts, and
range_search's argument validation, which raises before any library call.  No GPU."""
import numpy as np
import pytest

from revisit_anything_amd.engine import (SegVLADEngine, expand_radius2, radius2_from_sim, range_from_topk, range_image_counts)


def _lists(nq=12, n=60, d=8, k=60, seed=0):
    """Ascending (d2, id) top-k lists of random fp32 data with planted exact ties (duplicate rows)."""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((n, d)).astype(np.float32)
    R[41], R[42], R[7] = R[3], R[3], R[50]
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    D = ((Q[:, None, :] - R[None, :, :]) ** 2).sum(2).astype(np.float32)
    ids = np.arange(n)
    order = np.stack([np.lexsort((ids, D[q])) for q in range(nq)])
    d2 = np.take_along_axis(D, order, 1)
    idx = order.astype(np.int64)
    if k > n:
        d2 = np.concatenate([d2, np.full((nq, k - n), np.inf, np.float32)], 1)
        idx = np.concatenate([idx, np.full((nq, k - n), -1, np.int64)], 1)
    return D, d2[:, :k], idx[:, :k]


def _brute(D, radius2):
    nq, n = D.shape
    r = np.broadcast_to(np.asarray(radius2, np.float32), (nq,))
    lims, dd, ii = [0], [], []
    for q in range(nq):
        hits = [(D[q, j], j) for j in range(n) if r[q] > 0 and D[q, j] < r[q]]
        hits.sort()
        dd += [h[0] for h in hits]
        ii += [h[1] for h in hits]
        lims.append(lims[-1] + len(hits))
    return np.array(lims, np.int64), np.array(dd, np.float32), np.array(ii, np.int64)


def _eq(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[0][0] == 0 and np.all(np.diff(got[0]) >= 0)
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64


def test_range_from_topk_equals_the_brute_force_model():
    D, d2, idx = _lists(k=64)                              # deeper than the index: (+inf, -1) padding
    for r in (np.float32(4.0), np.float32(np.median(D)), np.linspace(0.5, 20.0, D.shape[0]).astype(np.float32)):
        _eq(range_from_topk(d2, idx, r), _brute(D, r))


def test_strictness_at_an_attained_value_and_its_ties():
    D, d2, idx = _lists(k=64)
    nq = D.shape[0]
    tie_rows = [q for q in range(nq) if np.any(np.diff(d2[q, :60]) == 0)]
    assert len(tie_rows) == nq                              # (the duplicates tie in every row)
    for c in (0, 1, 5, 30):
        r = d2[:, c].copy()                                 # ON a list value: that entry and everything tied with it is out
        got = range_from_topk(d2, idx, r)
        _eq(got, _brute(D, r))
        assert np.all(np.diff(got[0]) == (d2[:, :60] < r[:, None]).sum(1)) and np.all(np.diff(got[0]) <= c)
        up = np.nextafter(r, np.float32(np.inf))            # just above: they are all in
        got = range_from_topk(d2, idx, up)
        _eq(got, _brute(D, up))
        assert np.all(np.diff(got[0]) == (d2[:, :60] <= r[:, None]).sum(1)) and np.all(np.diff(got[0]) >= c + 1)
    # a radius on the tied value itself: every twin out, then every twin in, lower id first
    q = 0
    j = int(np.nonzero(np.diff(d2[q, :60]) == 0)[0][0])
    r = np.full(nq, d2[q, j], np.float32)
    lims, dd, ii = range_from_topk(d2, idx, r)
    assert lims[1] == j
    lims, dd, ii = range_from_topk(d2, idx, np.nextafter(r, np.float32(np.inf)))
    assert lims[1] >= j + 2 and ii[j] < ii[j + 1] and dd[j] == dd[j + 1]


def test_degenerate_radii():
    D, d2, idx = _lists(k=64)
    nq, n = D.shape
    r = np.full(nq, 5.0, np.float32)
    r[0], r[1], r[2], r[3], r[4] = 0.0, -3.0, np.nan, -np.inf, np.inf
    got = range_from_topk(d2, idx, r)
    _eq(got, _brute(D, r))
    cnt = np.diff(got[0])
    assert list(cnt[:4]) == [0, 0, 0, 0] and cnt[4] == n
    lims, dd, ii = range_from_topk(d2[:, :0], idx[:, :0], 1.0)   # no depth at all: nothing to report, nothing to doubt
    assert lims.tolist() == [0] * (nq + 1) and dd.size == 0 and ii.size == 0


def test_a_list_too_shallow_to_decide_raises():
    D, d2, idx = _lists(k=10)
    r = d2[:, 9].copy()
    range_from_topk(d2, idx, r)                             # the last entry is NOT below the radius: decidable
    with pytest.raises(ValueError, match="too shallow"):
        range_from_topk(d2, idx, np.nextafter(r, np.float32(np.inf)))
    with pytest.raises(ValueError, match="too shallow"):
        range_from_topk(d2, idx, np.float32(np.inf))
    _, d2f, idxf = _lists(k=64)                             # a list that holds the whole index is never too shallow
    assert range_from_topk(d2f, idxf, np.float32(np.inf))[0][-1] == D.size
    with pytest.raises(ValueError):
        range_from_topk(d2, idx[:, :5], 1.0)
    with pytest.raises(ValueError):
        range_from_topk(d2, idx, np.ones(3, np.float32))


def test_radius2_from_sim():
    assert radius2_from_sim(0.5) == np.float32(1.5) and isinstance(radius2_from_sim(0.5), np.float32)
    out = radius2_from_sim([2.0, 1.0, -1.0])
    assert out.dtype == np.float32 and out.tolist() == [0.0, 1.0, 3.0]
    assert radius2_from_sim(np.float32(0.1)) == np.float32(2.0) - np.float32(0.1)


def test_range_image_counts():
    img = np.array([0, 0, 1, 1, 1, 2, 5, 5], np.int32)
    lims = np.array([0, 2, 2, 5, 6], np.int64)              # 4 query rows
    idx = np.array([0, 7, 2, 3, 1, 6], np.int64)
    out = range_image_counts(lims, idx, img, [0, 2, 3, 4])  # images own rows {0, 1}, {2}, {3}
    assert out[0][0].tolist() == [0, 5] and out[0][1].tolist() == [1, 1]
    assert out[1][0].tolist() == [0, 1] and out[1][1].tolist() == [1, 2]
    assert out[2][0].tolist() == [5] and out[2][1].tolist() == [1]
    out = range_image_counts(lims, idx, img, [0, 0, 4])     # an image without rows
    assert out[0][0].size == 0 and out[1][0].tolist() == [0, 1, 5] and out[1][1].tolist() == [2, 2, 2]
    with pytest.raises(ValueError):
        range_image_counts(lims, idx, img, [0, 2, 3])


def test_expand_radius2_shapes():
    assert expand_radius2(1.5, 4).tolist() == [1.5] * 4
    assert expand_radius2([1, 2, 3, 4], 4).tolist() == [1, 2, 3, 4]
    assert expand_radius2([1, 2], 5, [0, 2, 5]).tolist() == [1, 1, 2, 2, 2]
    assert expand_radius2([1, 2, 3, 4, 5], 5, [0, 2, 5]).tolist() == [1, 2, 3, 4, 5]
    for args in (([1, 2, 3], 4), ([1, 2, 3], 5, [0, 2, 5]), ([[1, 2]], 2), ([1, 2], 5, [0, 2, 4]), ([1, 2], 5, [1, 2, 5])):
        with pytest.raises(ValueError):
            expand_radius2(*args)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_range_search_validates_before_any_library_call():
    eng = object.__new__(SegVLADEngine)                     # no context: every library call would be an error
    eng.lib, eng._h = _NoLib(), None
    Q = np.zeros((6, 8), np.float32)
    with pytest.raises(ValueError):
        eng.range_search(Q, np.ones(5, np.float32))
    with pytest.raises(ValueError):
        eng.range_search(Q, np.ones(2, np.float32), qseg_offsets=[0, 2, 4, 6])
    with pytest.raises(ValueError):
        eng.range_search(Q, np.ones(3, np.float32), qseg_offsets=[0, 2, 4, 5])
    with pytest.raises(ValueError):
        eng.range_search(Q, np.ones((6, 1), np.float32))
    with pytest.raises(ValueError):
        eng.range_search(Q, 1.0, capacity=-1)
    eng._h = None
