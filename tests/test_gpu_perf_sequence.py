"""The sequence re-ranking against the vote that produces its input, on a real MI355X (marker gpu_perf; run with SEGVLAD_GUARD=0).
Through tools/sequence_sim.py: 1 M x 1024, 20 000 images x 50 rows, a traversal of 200 query frames x 50 rows searched k = 50 deep,
HIP events, warm, median of 20; ONE segvlad_sequence_rerank call with every output (back = fwd = 5, five velocities, tol = 1)
against ONE segvlad_vote call with n_top = C and scores, in the same process, both through the C entry points on preallocated
device outputs, for C = 5 and C = 20.  The stage reads the vote's two [200][C] tensors and nothing else: two launches.

The bound set before any measurement was sequence_ms <= 1.0 x vote_ms on both shapes: a stage that reads lists must not cost more
than the stage that builds them.  Measured (profiles/sequence_rerank.json): 0.0252 ms against 0.0716 ms = 0.352 x at C = 5 and
0.0286 against 0.0852 ms = 0.336 x at C = 20 (three more runs: 0.348 .. 0.355 and 0.314 .. 0.339).  Both below 1.0, so the bounds are
the measured ratios x 1.15 (the rule of test_gpu_perf_match.py): see BOUND below.  The heaviest legal shape on its own -- 10 000
frames, C = 64, back = fwd = 32, 16 velocities, 666 M lookups -- took 4.97 ms; it is reported, not bounded.  In 37 of the 200 frames
a distant frame out-votes the true one: the true frame comes first in 0.815 of the frames before the stage and in 1.000 after
(reported by the tool, not asserted here)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu_perf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOUND = {5: 0.404, 20: 0.386}


def _run():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sequence_sim
    finally:
        sys.path.pop(0)
    out = sequence_sim.run(sequence_sim.parse(["--cands", "5,20", "--reps", "20"]))
    for r in out["runs"]:
        print(f"[sequence] {r['shape']:6s} C {r['C']:2d}: sequence_rerank {r['sequence_ms']:.4f} ms, vote {r['vote_ms']:.4f} ms = {r['ratio']:.3f} x; "
              f"true frame first {r['true_first_before']:.3f} -> {r['true_first_after']:.3f} ({r['aliased_frames']} aliased frames)")
    h = out["heavy"]
    print(f"[sequence] heavy  T {h['T']} C {h['C']} window {h['back']}+{h['fwd']} velocities {h['n_vel']}: {h['sequence_ms']:.3f} ms")
    return out


@pytest.fixture(scope="module")
def result():
    return _run()


def test_sequence_rerank_costs_no_more_than_the_vote_it_follows(result):
    assert sorted(r["C"] for r in result["runs"]) == [5, 20]
    for r in result["runs"]:
        assert r["sequence_ms"] <= BOUND[r["C"]] * r["vote_ms"], r
