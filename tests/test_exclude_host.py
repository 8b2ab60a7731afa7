"""Host side of the search that excludes image-id windows: the interval helpers against a numpy restatement, the validation of
malformed input, and the timing tool's CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pad_intervals():
    from revisit_anything_amd.engine import pad_intervals

    a = pad_intervals([[(3, 5), (1, 1)], [], [(7, 9)]])
    assert a.dtype == np.int32 and a.shape == (3, 2, 2)
    assert a.tolist() == [[[3, 5], [1, 1]], [[0, -1], [0, -1]], [[7, 9], [0, -1]]]
    assert pad_intervals([[], []]).shape == (2, 1, 2)
    assert pad_intervals([[(4, 6)]], E=3).tolist() == [[[4, 6], [0, -1], [0, -1]]]
    assert pad_intervals([[(-5, 2_000_000_000)]]).tolist() == [[[-5, 2_000_000_000]]]
    for bad, kw in (([[(1, 2), (3, 4), (5, 6)]], {"E": 2}), ([[(i, i) for i in range(9)]], {}), ([[(1, 2)]], {"E": 0}), ([[(1, 2)]], {"E": 9}),
                    ([[(1, 2, 3)]], {}), ([[1, 2, 3]], {}), ([[(0, 2 ** 31)]], {})):
        with pytest.raises(ValueError):
            pad_intervals(bad, **kw)


def test_window_intervals():
    from revisit_anything_amd.engine import window_intervals

    w = window_intervals([0, 7, 19999], 5)
    assert w.dtype == np.int32 and w.shape == (3, 1, 2)
    assert w[:, 0].tolist() == [[-5, 5], [2, 12], [19994, 20004]]
    assert window_intervals([4], 0)[0, 0].tolist() == [4, 4]
    assert window_intervals([], 3).shape == (0, 1, 2)
    with pytest.raises(ValueError):
        window_intervals([1], -1)
    with pytest.raises(ValueError):
        window_intervals([2 ** 31 - 2], 5)


def test_check_intervals():
    from revisit_anything_amd.engine import check_intervals

    check_intervals(np.zeros((2, 8, 2), np.int64), 2)
    for bad, n_img in ((np.zeros((2, 1, 2), np.int64), 3), (np.zeros((1, 9, 2), np.int64), 1), (np.zeros((1, 0, 2), np.int64), 1),
                       (np.zeros((1, 2), np.int64), 1), (np.zeros((1, 1, 3), np.int64), 1), (np.full((1, 1, 2), 2 ** 31, np.int64), 1)):
        with pytest.raises(ValueError):
            check_intervals(bad, n_img)


def _covered(ivs, n):
    """The restatement: the set of ids 0 .. n-1 that any interval covers, id by id."""
    m = np.zeros(n, bool)
    ids = np.arange(n)
    for lo, hi in np.asarray(ivs, np.int64).reshape(-1, 2):
        m |= (ids >= lo) & (ids <= hi)
    return m


def test_merge_and_excluded_rows_against_numpy():
    from revisit_anything_amd.engine import excluded_rows, merge_intervals

    assert merge_intervals([(5, 7), (1, 2), (3, 3), (9, 8), (6, 12)]) == [(1, 3), (5, 12)]
    assert merge_intervals([(4, 3)]) == [] and merge_intervals([]) == []
    rng = np.random.default_rng(0)
    n_ref = 60
    counts = rng.integers(0, 9, n_ref)                  # rows per reference image; some carry none
    for e in (1, 3, 8):
        ex = np.zeros((40, e, 2), np.int64)
        ex[:, :, 0] = rng.integers(-10, n_ref + 10, (40, e))
        ex[:, :, 1] = ex[:, :, 0] + rng.integers(-2, 15, (40, e))
        ex[0, 0] = (-2_000_000_000, 2_000_000_000)
        X = excluded_rows(ex, counts)
        for b in range(40):
            m = merge_intervals(ex[b])
            assert all(lo <= hi for lo, hi in m) and all(m[i][1] + 1 < m[i + 1][0] for i in range(len(m) - 1))   # sorted, disjoint, not adjacent
            if b > 0:   # the merged intervals cover exactly the ids the given ones cover (ids shifted by 20: some lie below 0)
                assert np.array_equal(_covered(np.array(m, np.int64).reshape(-1, 2) + 20, n_ref + 60), _covered(ex[b] + 20, n_ref + 60))
            assert X[b] == counts[_covered(ex[b], n_ref)].sum()
        assert X[0] == counts.sum()


def test_exclude_sim_cli():
    tool = os.path.join(ROOT, "tools", "exclude_sim.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--radius" in r.stdout and "--crowd" in r.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import exclude_sim
    finally:
        sys.path.pop(0)
    a = exclude_sim.parse([])
    assert a.k == [50, 200] and a.radius == [0, 5, 20, 200] and a.n_ref_img == 20000 and a.segs == 50 and a.n_q_img == 200 and a.reps >= 20
    a = exclude_sim.parse(["--k", "10,1024", "--radius", "3", "--reps", "2", "--alt", "--crowd", "11"])
    assert a.k == [10, 1024] and a.radius == [3] and a.reps == 2 and a.alt and a.crowd == 11
    for bad in (["--k", "0"], ["--k", "1025"], ["--radius", "-1"], ["--reps", "0"], ["--n-q-img", "30000"]):
        with pytest.raises(SystemExit):
            exclude_sim.parse(bad)
