"""Host side of the sequence re-ranking (segvlad_sequence_rerank): the NumPy reference (tests/sequence_ref.py) on a planted traversal
whose outcome follows from the arithmetic alone, the helpers next to pad_candidates, sequence_rerank's validation (which raises
before any library call), the entry point's presence in the header and the ctypes table, and the timing tool's command line.
No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sequence_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VELS = [0.5, 1.0, 1.5, -1.0]
SEQ = [0, 17, 40]


@pytest.mark.parametrize("tol", [0, 1])
@pytest.mark.parametrize("v_true", VELS)
def test_planted_true_frame_comes_first_with_its_velocity(v_true, tol):
    """T = 40 in two sequences (17 + 23), C = 8, back = fwd = 5.  A distractor out-scores the true place in every frame (1.5
    against 1.0) and has no support: its id is thousands of map frames from every id of the neighbouring frames, a line reaches
    1.5 x 5 + 1 at most.  The true place finds its line."""
    cand, score, slot = S.planted_case(v_true)
    out = S.sequence_rerank(cand, score, SEQ, 5, 5, VELS, tol)
    t = np.arange(40)
    assert np.array_equal(out["order"][:, 0], slot)
    assert np.array_equal(out["vel"][t, slot], np.full(40, VELS.index(v_true)))
    others = np.ones((40, 8), bool)
    others[t, slot] = False
    assert np.array_equal(out["seq_score"][others], score[others]) and not out["n_hit"][others].any()   # no distractor is supported
    assert np.array_equal(out["seq_score"][t, slot], 1.0 + out["n_hit"][t, slot])                        # every support adds 1.0
    for row in out["order"]:
        assert sorted(row.tolist()) == list(range(8))
    if v_true in (1.0, -1.0):   # an integer velocity: every frame of the window that exists is a hit
        want = [min(5, i) + min(5, n - 1 - i) for n in (17, 23) for i in range(n)]
        assert out["n_hit"][t, slot].tolist() == want
    if v_true == 0.5:           # floor(t / 2) against rint(tau / 2), half to even: rounding costs support that the tolerance returns
        sc = out["seq_score"][t, slot]
        assert (sc.min(), sc.max()) == ((4.0, 8.0) if tol == 0 else (6.0, 11.0))


@pytest.mark.parametrize("tol", [0, 1])
@pytest.mark.parametrize("v_true", VELS)
def test_planted_causal_window_needs_one_frame_of_history(v_true, tol):
    """fwd = 0, back = 5, one sequence: frame 0 has nothing behind it and its distractor stays first; every later frame has."""
    cand, score, slot = S.planted_case(v_true)
    out = S.sequence_rerank(cand, score, None, 5, 0, VELS, tol)
    assert np.array_equal(out["order"][1:, 0], slot[1:])
    assert out["order"][0, 0] != slot[0] and out["n_hit"][0].tolist() == [0] * 8
    assert np.array_equal(out["seq_score"][0], score[0])


def test_reference_on_hand_made_cases():
    # two frames, one velocity: 10 -> 11 is on the line v = 1, 10 -> 13 is not; tol = 2 reaches it, and takes the LARGEST score in reach
    cand = np.array([[10, 50], [13, 11]], np.int32)
    score = np.array([[1.0, 2.0], [4.0, 0.5]])
    out = S.sequence_rerank(cand, score, None, 1, 1, [1.0], 0)
    assert out["seq_score"].tolist() == [[1.5, 2.0], [4.0, 1.5]] and out["n_hit"].tolist() == [[1, 0], [0, 1]]
    assert out["order"].tolist() == [[1, 0], [0, 1]] and out["vel"].tolist() == [[0, 0], [0, 0]]
    out = S.sequence_rerank(cand, score, None, 1, 1, [1.0], 2)
    assert out["seq_score"].tolist() == [[5.0, 2.0], [5.0, 1.5]]
    # a sequence boundary between the two frames: nothing is supported
    out = S.sequence_rerank(cand, score, [0, 1, 1, 2], 1, 1, [1.0], 2)
    assert out["seq_score"].tolist() == score.tolist() and not out["n_hit"].any()
    # empty slots: a negative id, NaN and inf scores -- zeros, -1, last in slot order, and no support for anybody
    cand = np.array([[-1, 10, 10, 10], [11, 11, 11, -5]], np.int32)
    score = np.array([[3.0, np.nan, 1.0, np.inf], [2.0, -np.inf, 0.25, 9.0]])
    out = S.sequence_rerank(cand, score, None, 1, 1, [1.0], 0)
    assert out["seq_score"].tolist() == [[0.0, 0.0, 3.0, 0.0], [3.0, 0.0, 1.25, 0.0]]
    assert out["vel"].tolist() == [[-1, -1, 0, -1], [0, -1, 0, -1]] and out["order"].tolist() == [[2, 0, 1, 3], [0, 2, 1, 3]]
    # half-way products round to even: rint(0.5) = 0, rint(1.5) = 2, rint(-2.5) = -2; ties between velocities go to the lowest index
    one = np.ones((3, 1))
    assert S.sequence_rerank(np.array([[100], [100], [101]], np.int32), one, None, 0, 2, [1.0, 0.5, 1.5], 0)["vel"][:, 0].tolist() == [1, 0, 0]
    assert S.sequence_rerank(np.array([[100], [100], [102]], np.int32), one, None, 0, 2, [1.0, 0.5, 1.5], 0)["vel"][:, 0].tolist() == [0, 2, 0]
    assert S.sequence_rerank(np.array([[100], [102]], np.int32), one[:2], None, 1, 0, [2.5, 3.0], 0)["n_hit"].tolist() == [[0], [1]]
    assert S.sequence_rerank(np.array([[100], [101]], np.int32), one[:2], None, 0, 1, [2.0, 1.0, 1.0], 0)["vel"].tolist() == [[1], [0]]
    # ids next to INT32_MAX: p and p +- tol live in int64
    big = np.iinfo(np.int32).max
    out = S.sequence_rerank(np.array([[big - 1], [big]], np.int32), one[:2], None, 1, 1, [1.0], 0)
    assert out["n_hit"].tolist() == [[1], [1]]
    assert S.sequence_rerank(np.array([[big], [big]], np.int32), one[:2], None, 1, 1, [2.0], 2)["n_hit"].tolist() == [[1], [1]]
    assert S.sequence_rerank(np.array([[big], [big]], np.int32), one[:2], None, 1, 1, [2.0], 1)["n_hit"].tolist() == [[0], [0]]


def test_helpers():
    from revisit_anything_amd.engine import check_sequence_args, velocity_grid

    v = velocity_grid()
    assert v.dtype == np.float64 and np.array_equal(v, np.linspace(0.8, 1.2, 5)) and v[2] == 1.0
    assert velocity_grid(1.0, 1.0, 1).tolist() == [1.0] and velocity_grid(-1.5, -0.5, 3).tolist() == [-1.5, -1.0, -0.5]
    for bad in (dict(n=0), dict(n=17), dict(vmin=float("nan")), dict(vmax=float("inf")), dict(vmin=2.0, vmax=1.0), dict(vmax=2.0 ** 21)):
        with pytest.raises(ValueError):
            velocity_grid(**bad)
    so, vel = check_sequence_args(40, 8)
    assert so.dtype == np.int32 and so.tolist() == [0, 40] and np.array_equal(vel, velocity_grid())
    so, vel = check_sequence_args(40, 64, [0, 17, 17, 40], 32, 0, [-2.0 ** 20], 2 ** 30)
    assert so.tolist() == [0, 17, 17, 40] and vel.dtype == np.float64 and vel.tolist() == [-2.0 ** 20]
    assert check_sequence_args(0, 1, [0])[0].tolist() == [0]
    good = dict(T=40, C=8, seq_offsets=[0, 17, 40], back=5, fwd=5, velocities=[1.0], tol=1)
    for bad in (dict(T=-1), dict(C=0), dict(C=65), dict(seq_offsets=[0, 17, 39]), dict(seq_offsets=[1, 17, 40]), dict(seq_offsets=[0, 20, 17, 40]),
                dict(seq_offsets=[]), dict(seq_offsets=[0.0, 40.0]), dict(seq_offsets=[[0, 40]]), dict(back=-1), dict(back=33), dict(fwd=-1),
                dict(fwd=33), dict(fwd=2.5), dict(velocities=[]), dict(velocities=[1.0] * 17), dict(velocities=[[1.0]]),
                dict(velocities=[float("nan")]), dict(velocities=[float("inf")]), dict(velocities=[2.0 ** 20 + 1]), dict(tol=-1),
                dict(tol=2 ** 30 + 1), dict(tol=0.5)):
        with pytest.raises(ValueError):
            check_sequence_args(**{**good, **bad})


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_sequence_rerank_validates_before_any_library_call():
    from revisit_anything_amd.engine import SegVLADEngine

    eng = object.__new__(SegVLADEngine)                                 # no context: every library call would be an error
    eng.lib, eng._h = _NoLib(), None
    cand, score = np.zeros((6, 3), np.int32), np.ones((6, 3))
    good = dict(cand=cand, score=score)
    for bad in (dict(cand=np.zeros((6, 3), np.float32)), dict(cand=np.zeros(18, np.int32), score=np.ones(18)), dict(score=np.ones((6, 2))),
                dict(score=np.ones((5, 3))), dict(cand=np.zeros((6, 65), np.int32), score=np.ones((6, 65))),
                dict(cand=np.zeros((6, 0), np.int32), score=np.ones((6, 0))), dict(seq_offsets=[0, 5]), dict(back=33), dict(fwd=-1),
                dict(velocities=[float("nan")]), dict(velocities=np.ones(17)), dict(tol=-1)):
        with pytest.raises(ValueError):
            eng.sequence_rerank(**{**good, **bad})


def test_entry_point_is_declared_and_bound():
    """The prototype of the issue, parameter for parameter: the context and 15 arguments."""
    from revisit_anything_amd import _lib, build

    src = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+segvlad_sequence_rerank\s*\(([^)]*)\)\s*;", decl)
    assert m, "include/segvlad.h does not declare segvlad_sequence_rerank"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["segvlad_ctx* ctx", "const int32_t* cand", "const double* score", "int T", "int C", "const int32_t* seq_offsets",
                      "int n_seq", "int back", "int fwd", "const double* vel", "int n_vel", "int tol", "double* seq_score_out",
                      "int32_t* n_hit_out", "int32_t* vel_out", "int32_t* order_out"]
    assert "segvlad_sequence_rerank" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["segvlad_sequence_rerank"]
    assert len(args) == len(params) and res is C.c_int
    assert [i for i, a in enumerate(args) if a is C.c_int] == [3, 4, 6, 7, 8, 10, 11]
    assert "sequence_kernels.hip" in build.SOURCES
    # the calls it follows keep their surfaces
    assert len(_lib.SIGNATURES["segvlad_verify_pairs"][1]) == 18 and len(_lib.SIGNATURES["segvlad_vote"][1]) == 14
    # the contract is stated where the entry is declared
    doc = src[:src.index("int segvlad_sequence_rerank")]
    doc = doc[doc.rindex("/*"):]
    for phrase in ("frame numbers along the map", "truncation to C candidates", "rounded half to even", "ties to the lowest u",
                   "LARGEST score", '"sequence_rerank"', "never crosses a sequence boundary", "seq_offsets or vel in device memory"):
        assert phrase in doc, phrase
    # the scratch goes through the context's buffer lists
    ctx = open(os.path.join(ROOT, "revisit-anything_amd", "csrc", "ctx.h")).read()
    assert "X(s_sq_id)" in ctx and "X(s_sq_sc)" in ctx


def test_sequence_sim_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sequence_sim
    finally:
        sys.path.pop(0)
    a = sequence_sim.parse([])
    assert (a.n_ref_img, a.segs, a.d, a.n_q_img, a.k, a.cands, a.back, a.fwd, a.n_vel, a.tol, a.reps, a.seed, a.out) == \
        (20000, 50, 1024, 200, 50, [5, 20], 5, 5, 5, 1, 20, 0, None)
    assert (a.heavy_frames, a.heavy_c, a.heavy_window, a.heavy_vel) == (10000, 64, 32, 16)
    assert sequence_sim.parse(["--cands", "3,7", "--reps", "4", "--out", "x.json", "--heavy-frames", "0"]).cands == [3, 7]
    for bad in (["--cands", "65"], ["--cands", "0"], ["--reps", "0"], ["--n-q-img", "30000"], ["--back", "33"], ["--fwd", "-1"], ["--n-vel", "17"],
                ["--tol", "-1"], ["--heavy-c", "65"], ["--heavy-window", "33"], ["--heavy-vel", "0"]):
        with pytest.raises(SystemExit):
            sequence_sim.parse(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sequence_sim.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--cands" in r.stdout
    # the heavy shape's lists: ids of a small range so that most lookups hit, every slot filled
    cand, score = sequence_sim.make_heavy_lists(50, 64, np.random.default_rng(0))
    assert cand.shape == score.shape == (50, 64) and cand.dtype == np.int32 and score.dtype == np.float64
    assert cand.min() >= 0 and np.isfinite(score).all() and (score >= 0).all()
    out = S.sequence_rerank(cand[:8], score[:8], None, 3, 3, [1.0], 1)
    assert out["n_hit"].max() >= 3
