"""The exclusion's overhead on a real MI355X (marker gpu_perf; run with SEGVLAD_GUARD=0): segvlad_search_excluding against
segvlad_search at the SAME depth k_fetch on the same index -- the inner search, which the exclusion does not touch -- in one process
(tools/exclude_sim.py: 1 M x 1024, 20 000 images x 50 rows, HIP events, warm, median of 20), for a batch of 200 images x 50 rows and
for one image alone.

The bounds are the baseline plus a stated margin, not figures read off the new code: the head path adds one pass over nq x k_fetch
12-byte records (90 MB at 10 000 x 750: ~20 us at 5 TB/s) and one kernel boundary plus one small host -> device copy (4-5 us each) --
under 1 % of a 17-19 ms batch search, inside the 3 % run-to-run spread of the step times: <= 1.05 x; about 10 % of a 0.4 ms
single-image pass plus that spread: <= 1.25 x.  Radius 20 (k_fetch = 1024) is the head path with the tail's three kernels launched and
nothing flagged -- where a kernel boundary more than counted would show; the same bounds hold there (the baseline at that depth
is the distance-matrix path, 14.5 ms for one image: the three launches are well inside them)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu_perf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exclusion_costs_no_more_than_its_depth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import exclude_sim
    finally:
        sys.path.pop(0)
    out = exclude_sim.run(exclude_sim.parse(["--k", "50,200", "--radius", "0,5,20", "--reps", "20"]))
    for r in out["runs"]:
        print(f"[exclude] {r['shape']:6s} k={r['k']:3d} radius={r['radius']}: k_fetch {r['exclude_stats']['k_fetch']}, search(k) "
              f"{r['search_k_ms']:.3f} ms, search(k_fetch) {r['search_k_fetch_ms']:.3f} ms, search_excluding {r['exclude_ms']:.3f} ms "
              f"= {r['ratio_vs_k_fetch']:.3f} x the baseline (depth itself: {r['depth_cost']:.3f} x)")
    for r in out["runs"]:
        assert r["exclude_stats"]["tail_rows"] == 0
        assert r["exclude_stats"]["k_fetch"] == min(1024, r["k"] + (2 * r["radius"] + 1) * 50)
        assert r["ratio_vs_k_fetch"] <= (1.05 if r["shape"] == "batch" else 1.25), r
