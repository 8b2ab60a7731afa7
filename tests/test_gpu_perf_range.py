"""The range search against the top-k search it replaces, on a real MI355X (marker gpu_perf; run with SEGVLAD_GUARD=0).  Through
tools/range_sim.py: 1 M x 1024, 20 000 images x 50 rows, HIP events, warm, median of 20, a batch of 200 images x 50 rows and one
image alone; radii taken from a search(Q, 1024), so every row's count is known.  The baseline is segvlad_search on the same
index in the same process -- code the range search does not touch.  What is timed is ONE segvlad_range_search call whose
capacity suffices; the engine's retry is the caller's cost of a bad guess and is only reported.

Deep (1000 hits per row: what needs k = 1024 and the distance-matrix path today): range_ms < search_ms(k = 1024), no margin.
Shallow (50 hits per row) against search(k = 50): the two share the full-level filter launch; the range search drops the
sampled and stride-16 levels with their selects and adds the exact evaluation of whole candidate lists.  The bound: see
SHALLOW_BOUND below."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu_perf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tripwire was 1.5 x the search at the same depth (the estimate above plus the 3 % run-to-run spread the other perf tests
# allow).  Measured: batch 15.85 ms against 17.23 ms = 0.92 x (0.91 x in a second session), one image 0.477 ms against 0.380 ms
# = 1.26 x (the same filter launch plus two host round trips: the query scale and the total).  Both well below, so the bounds
# are the measured ratios x 1.15.
SHALLOW_BOUND = {"batch": 1.06, "single": 1.45}


def _runs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import range_sim
    finally:
        sys.path.pop(0)
    out = range_sim.run(range_sim.parse(["--depth", "50,1000", "--reps", "20"]))
    for r in out["runs"]:
        print(f"[range] {r['shape']:6s} depth {r['depth']:4d}: range_search {r['range_ms']:.3f} ms (with a retry {r['range_retry_ms']:.3f}), "
              f"search(k={r['depth']}) {r['search_k_ms']:.3f} ms = {r['ratio_vs_search_k']:.3f} x, search(k={r['k_cut']}) "
              f"{r['search_k_cut_ms']:.3f} ms = {r['ratio_vs_search_k_cut']:.3f} x; candidates mean {r['cand_mean']:.0f} max {r['cand_max']}, "
              f"long rows {r['long_rows']}, path {r['path']}")
    return out["runs"]


@pytest.fixture(scope="module")
def runs():
    return _runs()


def test_deep_radius_beats_the_search_at_k_1024(runs):
    deep = [r for r in runs if r["depth"] == 1000]
    assert len(deep) == 2
    for r in deep:
        assert r["k_cut"] == 1024 and r["path"] == "f16" and r["long_rows"] == 0, r
        assert r["range_ms"] < r["search_k_cut_ms"], r


def test_shallow_radius_costs_no_more_than_the_search_at_that_depth(runs):
    shallow = [r for r in runs if r["depth"] == 50]
    assert len(shallow) == 2
    for r in shallow:
        assert r["path"] == "f16" and r["long_rows"] == 0, r
        assert r["range_ms"] <= SHALLOW_BOUND[r["shape"]] * r["search_k_ms"], r
