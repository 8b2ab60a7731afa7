"""Host side of the mutual-nearest-segment re-ranking (segvlad_match_pairs): pad_candidates / check_candidates against hand-written
cases and malformed input, match_pairs' validation (which raises before any library call), the timing tool's command line, and
the entry point's presence in the header and the ctypes table.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pad_candidates():
    from revisit_anything_amd.engine import pad_candidates

    out = pad_candidates([[3, 1, 2], [], [7]])
    assert out.dtype == np.int32 and out.tolist() == [[3, 1, 2], [-1, -1, -1], [7, -1, -1]]
    assert pad_candidates([[4], [5, 6]], C=4).tolist() == [[4, -1, -1, -1], [5, 6, -1, -1]]
    assert pad_candidates([[], []]).tolist() == [[-1], [-1]]            # at least one slot
    assert pad_candidates([]).shape == (0, 1)
    assert pad_candidates([np.arange(64)]).shape == (1, 64)
    assert pad_candidates([[2, 2, -1, 2]]).tolist() == [[2, 2, -1, 2]]  # duplicates and padding pass through, in order
    for lists, C in (([[1, 2, 3]], 2), ([np.arange(65)], None), ([[1]], 0), ([[1]], 65), ([[2 ** 31]], None), ([[-2 ** 31 - 1]], None)):
        with pytest.raises(ValueError):
            pad_candidates(lists, C)


def test_check_candidates():
    from revisit_anything_amd.engine import check_candidates

    check_candidates(np.array([[0, -1, 5], [5, 5, 10 ** 9]], np.int32), 2)
    check_candidates(np.zeros((3, 64), np.int64), 3)
    check_candidates(np.zeros((0, 4), np.int32), 0)
    for cand, n_img in ((np.zeros((2, 3), np.int32), 3),                # rows != n_img
                        (np.zeros(4, np.int32), 4),                     # not 2-D
                        (np.zeros((2, 0), np.int32), 2),                # C = 0
                        (np.zeros((2, 65), np.int32), 2),               # C = 65
                        (np.array([[0, -2]], np.int32), 1),             # -1 is the only padding value
                        (np.array([[2 ** 31]], np.int64), 1),           # beyond int32
                        (np.zeros((1, 2), np.float32), 1)):             # not integers
        with pytest.raises(ValueError):
            check_candidates(cand, n_img)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_match_pairs_validates_before_any_library_call():
    from revisit_anything_amd.engine import SegVLADEngine

    eng = object.__new__(SegVLADEngine)                                 # no context: every library call would be an error
    eng.lib, eng._h = _NoLib(), None
    Q = np.zeros((6, 32), np.float32)
    qoff = [0, 2, 6]
    for cand in (np.zeros((3, 2), np.int32), np.zeros((2, 65), np.int32), np.array([[0, -2], [1, 1]], np.int32),
                 [[1, 2], list(range(65))], np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError):
            eng.match_pairs(Q, qoff, cand)


def test_match_sim_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import match_sim
    finally:
        sys.path.pop(0)
    a = match_sim.parse([])
    assert (a.n_ref_img, a.segs, a.d, a.n_q_img, a.cands, a.reps, a.seed) == (20000, 50, 1024, 200, [5, 20], 20, 0)
    assert match_sim.parse(["--cands", "3,7", "--reps", "4"]).cands == [3, 7]
    for bad in (["--cands", "65"], ["--cands", "0"], ["--reps", "0"], ["--n-q-img", "30000"]):
        with pytest.raises(SystemExit):
            match_sim.parse(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "match_sim.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--cands" in r.stdout
    rng = np.random.default_rng(0)
    frames = np.array([0, 7, 19])
    cand, slot = match_sim.make_candidates(frames, 20, 5, rng)
    assert cand.shape == (3, 5) and cand.dtype == np.int32 and ((cand >= 0) & (cand < 20)).all()
    assert all(len(set(row)) == 5 for row in cand.tolist()) and np.array_equal(cand[np.arange(3), slot], frames)


def test_entry_point_is_declared_and_bound():
    from revisit_anything_amd import _lib

    src = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    assert "func_vpr.py:247-270" in src                                 # the use it serves is cited where it is documented
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+segvlad_match_pairs\s*\(([^)]*)\)\s*;", decl)
    assert m, "include/segvlad.h does not declare segvlad_match_pairs"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and params[7] == "float max_d2" and params[6] == "int C"
    assert "segvlad_match_pairs" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["segvlad_match_pairs"]
    assert len(args) == len(params)
    import ctypes as C

    assert res is C.c_int and args[7] is C.c_float and args[2] is C.c_int and args[4] is C.c_int and args[6] is C.c_int
