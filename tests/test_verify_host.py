"""Host side of the spatial verification (segvlad_verify_pairs): the NumPy reference (tests/verify_ref.py) against an independent
formulation on integer coordinates and against hand-made cases, verify_pairs' validation (which raises before any library call),
the entry point's presence in the header and the ctypes table, and the timing tool's command line.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planted(rng, M, n_in, a, t):
    """Integer query points in [0, 128), the first n_in moved by the integer similarity (a, t), the rest integer outliers."""
    p = rng.integers(0, 128, (M, 2)).astype(np.float64)
    sc = a * (p[:, 0] + 1j * p[:, 1]) + t
    s = np.stack([sc.real, sc.imag], 1)
    s[n_in:] = rng.integers(-128, 256, (M - n_in, 2))
    return p, s


def test_reference_agrees_with_the_complex_formulation_on_integers():
    """Integer coordinates below 2^9: every intermediate of the contract's arithmetic is an integer below 2^53, hence exact, and
    the division-free test is the textbook one multiplied through by n.  The complex formulation rounds (a division, an abs), but
    a squared residual times n^2 is an integer and tol^2 n^2 = 4 n^2 is one too: a residual that differs from tol differs by at least
    1 / (2 tol n^2) > 1e-10, far beyond the rounding of a few fp64 operations.  Counts, winners and flags must agree."""
    rng = np.random.default_rng(11)
    for trial in range(20):
        a = (1, 1j, 1 + 1j, 2)[trial % 4]
        p, s = _planted(rng, 20, 12, a, complex(5, -3))
        cnt, i, j, flags, model = V.verify_slot(p, s, 2.0, 0.25, 4.0)
        cnt2, i2, j2, flags2 = V.verify_slot_complex(p, s, 2.0, 0.25, 4.0)
        assert (cnt, i, j) == (cnt2, i2, j2) and np.array_equal(flags, flags2)
        assert cnt >= 12 and flags.sum() == cnt and flags[i] and flags[j]
        if flags[:12].all() and i < 12 and j < 12:
            assert np.allclose(model, [a.real, a.imag, 5, -3], atol=1e-12)


def test_reference_on_hand_made_cases():
    # fewer than two correspondences, and a repeated query point (n = 0): nothing is eligible
    for p, s in (([], []), ([[1, 2]], [[3, 4]]), ([[1, 2], [1, 2]], [[0, 0], [5, 5]])):
        cnt, i, j, flags, model = V.verify_slot(np.array(p, float).reshape(-1, 2), np.array(s, float).reshape(-1, 2), 1.0, 0.5, 2.0)
        assert (cnt, i, j) == (0, -1, -1) and not flags.any() and np.isnan(model).all()
    # a pure shift: every hypothesis has all four inliers, the lowest h = (0, 1) wins
    p = np.array([[0, 0], [10, 0], [0, 10], [7, 3]], float)
    cnt, i, j, flags, model = V.verify_slot(p, p + [3, 4], 0.5, 0.5, 2.0)
    assert (cnt, i, j) == (4, 0, 1) and flags.all() and np.array_equal(model, [1, 0, 3, 4])
    # scale 3 is outside 0.5 .. 2: not eligible; inside 0.5 .. 4 it is
    assert V.verify_slot(p, 3 * p, 0.5, 0.5, 2.0)[0] == 0
    assert V.verify_slot(p, 3 * p, 0.5, 0.5, 4.0)[:3] == (4, 0, 1)
    # the bound is strict: a residual of exactly tol is no inlier
    s = p + [3, 4]
    s[3] += [2, 0]
    assert V.verify_slot(p, s, 2.0, 0.5, 2.0)[0] == 3 and V.verify_slot(p, s, 2.0 + 1e-9, 0.5, 2.0)[0] == 4
    # dropped rows: not mutual, id out of range, a non-finite coordinate on either side
    q_xy = np.array([[0, 0], [10, 0], [0, 10], [7, 3], [np.nan, 1], [2, 2], [4, 4]], float)
    r_xy = np.vstack([q_xy[:4] + [3, 4], [[np.inf, 0]]])
    fwd = np.array([0, 1, 2, 3, 0, 4, 7], np.int64).reshape(-1, 1)
    mut = np.array([1, 1, 0, 1, 1, 1, 1], np.uint8).reshape(-1, 1)
    out = V.verify_pairs(q_xy, r_xy, [0, 7], fwd, mut, 0.5)
    assert out["n_inlier"].tolist() == [[3]] and out["pair"].tolist() == [[[0, 1]]] and out["inlier"][:, 0].tolist() == [1, 1, 0, 1, 0, 0, 0]
    fwd[6] = -1
    assert V.verify_pairs(q_xy, r_xy, [0, 7], fwd, mut, 0.5)["n_inlier"].tolist() == [[3]]
    # order: (n_inlier desc, slot asc); an image without rows reports zeros and the identity order
    out = V.verify_pairs(q_xy, r_xy, [0, 0, 7], np.tile(fwd, 3), np.stack([mut[:, 0] * 0, mut[:, 0], mut[:, 0]], 1), 0.5)
    assert out["order"].tolist() == [[0, 1, 2], [1, 2, 0]] and out["n_inlier"].tolist() == [[0, 0, 0], [0, 3, 3]]
    assert out["pair"][0].tolist() == [[-1, -1]] * 3 and np.isnan(out["model"][0]).all()


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_verify_pairs_validates_before_any_library_call():
    from revisit_anything_amd.engine import SegVLADEngine

    eng = object.__new__(SegVLADEngine)                                 # no context: every library call would be an error
    eng.lib, eng._h = _NoLib(), None
    q_xy, r_xy = np.zeros((6, 2)), np.zeros((9, 2))
    qoff = [0, 2, 6]
    fwd, mut = np.zeros((6, 3), np.int64), np.ones((6, 3), np.uint8)
    good = dict(q_xy=q_xy, r_xy=r_xy, qseg_offsets=qoff, fwd_idx=fwd, mutual=mut, tol=2.0)
    for bad in (dict(q_xy=np.zeros((6, 3))), dict(q_xy=np.zeros(12)), dict(r_xy=np.zeros((9, 1))), dict(qseg_offsets=[0, 2, 5]),
                dict(qseg_offsets=[1, 2, 6]), dict(qseg_offsets=[0, 4, 2, 6]), dict(qseg_offsets=[]),
                dict(fwd_idx=np.zeros((5, 3), np.int64)), dict(fwd_idx=np.zeros((6, 3), np.float32)), dict(fwd_idx=np.zeros(6, np.int64)),
                dict(fwd_idx=np.zeros((6, 65), np.int64), mutual=np.ones((6, 65), np.uint8)),
                dict(fwd_idx=np.zeros((6, 0), np.int64), mutual=np.ones((6, 0), np.uint8)),
                dict(mutual=np.ones((6, 2), np.uint8)), dict(mutual=np.ones((6, 3), np.float64)),
                dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
                dict(min_scale=0.0), dict(min_scale=3.0), dict(max_scale=float("inf")), dict(min_scale=float("nan")),
                dict(q_xy=np.zeros((300, 2)), qseg_offsets=[0, 257, 300], fwd_idx=np.zeros((300, 3), np.int64),
                     mutual=np.ones((300, 3), np.uint8))):
        with pytest.raises(ValueError):
            eng.verify_pairs(**{**good, **bad})


def test_entry_point_is_declared_and_bound():
    """The prototype of the issue, parameter for parameter: the context and 17 arguments, 18 in all (the issue's prose says
    19; its prototype, which this pins, has 18)."""
    from revisit_anything_amd import _lib

    src = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+segvlad_verify_pairs\s*\(([^)]*)\)\s*;", decl)
    assert m, "include/segvlad.h does not declare segvlad_verify_pairs"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["segvlad_ctx* ctx", "const double* q_xy", "int nq", "const double* r_xy", "int64_t n_r",
                      "const int32_t* qseg_offsets", "int n_img", "int C", "const int64_t* fwd_idx", "const uint8_t* mutual",
                      "double tol", "double min_scale", "double max_scale", "int32_t* n_inlier_out", "int32_t* pair_out",
                      "double* model_out", "int32_t* order_out", "uint8_t* inlier_out"]
    assert "segvlad_verify_pairs" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["segvlad_verify_pairs"]
    import ctypes as C

    assert len(args) == len(params) and res is C.c_int
    assert [i for i, a in enumerate(args) if a is C.c_int] == [2, 6, 7] and args[4] is C.c_int64
    assert [i for i, a in enumerate(args) if a is C.c_double] == [10, 11, 12]
    # the match call it follows keeps its surface
    assert len(_lib.SIGNATURES["segvlad_match_pairs"][1]) == 14
    # the contract is stated where the entry is declared
    doc = src[:src.index("int segvlad_verify_pairs")]
    doc = doc[doc.rindex("/*"):]
    for phrase in ("ux*ux + uy*uy < ((tol*tol)*n)*n", "lowest h", "more than 256 rows", "SEGVLAD_ERR_LIMIT", '"verify_pairs"', "lexicographic"):
        assert phrase in doc, phrase


def test_verify_sim_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import verify_sim
    finally:
        sys.path.pop(0)
    a = verify_sim.parse([])
    assert (a.n_ref_img, a.segs, a.d, a.n_q_img, a.cands, a.reps, a.seed, a.tol, a.out) == (20000, 50, 1024, 200, [5, 20], 20, 0, 3.0, None)
    assert verify_sim.parse(["--cands", "3,7", "--reps", "4", "--out", "x.json"]).cands == [3, 7]
    for bad in (["--cands", "65"], ["--cands", "0"], ["--reps", "0"], ["--n-q-img", "30000"], ["--segs", "257"], ["--tol", "0"]):
        with pytest.raises(SystemExit):
            verify_sim.parse(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "verify_sim.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--cands" in r.stdout
    # the planted centroids: the true rows' pairs follow one similarity per image, and the reference finds them all
    rng = np.random.default_rng(0)
    rows = np.concatenate([np.arange(40, 60), np.arange(0, 20)])
    q_xy, r_xy = verify_sim.make_centroids(100, rows, 20, rng, noise=0.0)
    assert q_xy.shape == (40, 2) and r_xy.shape == (100, 2) and q_xy.dtype == np.float64
    out = V.verify_pairs(q_xy, r_xy, [0, 20, 40], rows.reshape(-1, 1), np.ones((40, 1), np.uint8), 1e-6)
    assert out["n_inlier"].tolist() == [[20], [20]]
    s = np.hypot(*out["model"][:, 0, :2].T)
    assert ((s > 0.69) & (s < 1.41)).all()
