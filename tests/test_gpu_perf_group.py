"""The grouped search against the plain search it runs on, on a real MI355X (marker gpu_perf; run with SEGVLAD_GUARD=0).
Through tools/group_sim.py: 1 M x 1024, 20 000 images x 50 rows, HIP events, warm, median of 20, a batch of 200 query images x 50
rows, k = 50, per_image = 1, on the plain database and on the planted near-duplicate one (sibling groups of 31).  The baseline is
segvlad_search at depth k_fetch in the same process: the inner search, code the grouped search does not touch.

The bounds are the ratios recorded in profiles/search_grouped.json x 1.15, the margin tests/test_gpu_perf_match.py uses for the
run-to-run spread: see `bound` below.  The default depth factor rests on tail_rows == 0 on the planted database there.  Recorded:
plain 19.66 against 19.43 ms = 1.012 x, planted 19.53 against 19.18 ms = 1.018 x; no row in the tail on either."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu_perf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorded():
    with open(os.path.join(ROOT, "profiles", "search_grouped.json")) as f:
        rec = json.loads(f.readline())
    return {r["db"]: r["ratio"] for r in rec["runs"] if r["group_fetch"] == 0}


@pytest.fixture(scope="module")
def bound():
    return {db: 1.15 * ratio for db, ratio in _recorded().items()}


@pytest.fixture(scope="module")
def runs(bound):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import group_sim
    finally:
        sys.path.pop(0)
    out = group_sim.run(group_sim.parse(["--reps", "20"]))
    for r in out["runs"]:
        print(f"[group] {r['db']:8s}: search_grouped {r['grouped_ms']:.3f} ms, search(k_fetch={r['k_fetch']}) {r['search_k_fetch_ms']:.3f} ms "
              f"= {r['ratio']:.3f} x (bound {bound.get(r['db'], float('nan')):.3f}); tail_rows {r['tail_rows']}, max_read {r['max_read']}")
    return out["runs"]


def test_costs_no_more_than_the_recorded_ratio_of_the_plain_search(runs, bound):
    assert sorted(r["db"] for r in runs) == ["plain", "planted"]
    for r in runs:
        assert r["db"] in bound, f"profiles/search_grouped.json holds no recorded ratio for the {r['db']} database"
        assert r["grouped_ms"] <= bound[r["db"]] * r["search_k_fetch_ms"], r
        assert r["images_over_cap"] == 0, r


def test_no_row_needs_the_tail_at_the_default_depth(runs):
    for r in runs:                                       # (the issue asks it of the plain database; the planted one is what the factor rests on)
        assert r["tail_rows"] == 0, r
