"""segvlad_search over the shape table of tests/search_plan_cases.py: one case per decision of plan_search / chunk_path and per load
path of the exact GEMM (scalar and vector operand loads, fast and guarded main loops, query views off their 16-byte boundary).
Every case builds a fresh index, asserts the branch it was written for from search_stats() and the stage launch counts BEFORE
anything else -- no case passes on another kernel -- and is then held against two references that share nothing with the library:

    the emulated fp32 arithmetic (tests/fp32_emu.py), bit for bit, ties included, on the first and last query rows, both sides of
    the 128- and 16384-row boundaries and others up to min(nq, 8) (every row of the margin-stress cases);
    float64 distances for EVERY query row (a torch GEMM on the device, a tool of the test): no neighbour outside the tolerance
    band of the k-th distance is missing or listed, |d2 - d64| <= 4e-6 x scale, (distance, id) order, padding beyond the index.
    The pairs inside the band are undecided; tests/test_search_plan_cases.py shows on the CPU that they stay below 1 %.

Run with `-m gpu` on an MI355X."""
import time

import pytest
from conftest import engine_scope

import fp32_emu as E
import search_plan_cases as T

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = {"level_carry": 1, "knn_heuristic": 1, "knn_filter": "auto"}


@pytest.fixture(scope=engine_scope)
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _query_view(Q, offset):
    """Q [nq, d] (NumPy) as a contiguous device view `offset` floats past a 16-byte boundary."""
    import torch

    nq, d = Q.shape
    buf = torch.empty(nq * d + 8, dtype=torch.float32, device="cuda:0")
    off = offset + (-(buf.data_ptr() // 4) % 4)
    Qv = buf[off:off + nq * d].view(nq, d)
    Qv.copy_(torch.from_numpy(Q))
    assert Qv.data_ptr() % 16 == 4 * offset and Qv.is_contiguous()
    return Qv


def _launches(eng, stage):
    from revisit_anything_amd._lib import SegVLADError

    try:
        return eng.stage_ms(stage)[1]
    except SegVLADError as e:
        assert "has not run" in str(e), e                 # the matrix path has no level 0
        return 0


def _search(eng, R, Q, k, opts):
    """A search on a fresh index: (d2, idx, search_stats(), launches of the stages knn_gemm + knn_level0)."""
    eng.db_reset()
    eng.db_add(R)
    try:
        eng.set_option("search_stats", 1)
        for name, v in opts.items():
            eng.set_option(name, v)
        eng.set_profiling(True)
        eng.profile_reset()
        d2, idx = eng.search(Q, k)
        launches = _launches(eng, "knn_gemm") + _launches(eng, "knn_level0")
        st = eng.search_stats()
    finally:
        eng.set_profiling(False)
        for name in opts:
            eng.set_option(name, OPTION_DEFAULTS[name])
        eng.set_option("search_stats", 0)
    return d2, idx, st, launches


def _assert_branch(c, st, launches):
    p = T.case_plan(c)
    assert st["filter"] == c.filter and st["levels"] == c.levels and st["n_queries"] == c.nq, st
    assert st["carry_rows"] == (p["carry_rows"] if c.carry else 0), (st, p)
    assert launches == p["launches"], (launches, p)          # chunks x (level 0 [+ its K split's reduction] + the filter levels)
    if c.flags == "zero":
        assert st["n_fallback"] == 0 and st["n_redo"] == 0, st
    elif c.flags == "rare":
        assert st["n_fallback"] == 0 and st["n_redo"] <= 1 + c.nq // 4096, st
    else:
        assert st["n_fallback"] + st["n_redo"] > 0, st


@pytest.mark.parametrize("c", T.CASES, ids=[c.name for c in T.CASES])
def test_search_plan_case(eng, c):
    import torch

    t0 = time.perf_counter()
    Rn, Qn = T.make_data(c)
    R = torch.from_numpy(Rn).cuda()
    Q = _query_view(Qn, c.q_offset)
    d2, idx, st, launches = _search(eng, R, Q, c.k, c.opts)
    print(f"{c.name}: launches {launches}", st)
    _assert_branch(c, st, launches)
    rows = T.emulated_rows(c)
    contested, ties, worst = E.check_contested(Q, R, d2, idx, c.k, queries=rows, tol64=c.tol64, q_aligned=c.q_offset == 0)
    print(f"{c.name}: {len(rows)} rows emulated, {contested} contested pairs, {ties} exact ties, emulation - fp64 {worst:.2e}")
    if c.data == "shell":
        assert ties > 0                                   # the planted duplicates: the id alone orders them
    if c.fp64:
        und, total = T.check_all_queries(Q, R, d2, idx, c.k)
        print(f"{c.name}: {und} of {total} pairs undecided")
        assert und <= 0.01 * total, (und, total)
    print(f"{c.name}: {time.perf_counter() - t0:.2f} s")


OFFSET_CASES = [c for c in T.CASES if c.q_offset]


@pytest.mark.parametrize("c", OFFSET_CASES, ids=[c.name for c in OFFSET_CASES])
def test_offset_view_differs_from_its_aligned_copy_as_the_emulations_do(eng, c):
    """The same query rows through a view one float past a 16-byte boundary and through an aligned copy: each result equals, bit for
    bit on every row, the emulation told which alignment it had -- so the two results differ exactly where the two emulations
    do: in the query norms, which row_sumsq forms element by element for the view.  At d % 4 == 0 some norms do differ: the scalar
    path really ran."""
    import torch

    Rn, Qn = T.make_data(c)
    R = torch.from_numpy(Rn).cuda()
    Qv, Qa = _query_view(Qn, 1), _query_view(Qn, 0)
    dv, iv, stv, _ = _search(eng, R, Qv, c.k, c.opts)
    da, ia, sta, _ = _search(eng, R, Qa, c.k, c.opts)
    assert stv["filter"] == sta["filter"] == c.filter and stv["levels"] == sta["levels"] == c.levels
    rows = list(range(min(c.nq, 64)))
    E.check_contested(Qv, R, dv, iv, c.k, queries=rows, q_aligned=False)
    E.check_contested(Qa, R, da, ia, c.k, queries=rows, q_aligned=True)
    q2v, q2a = E.row_sumsq(Qn, aligned=False), E.row_sumsq(Qn, aligned=True)
    kk = min(c.k, c.n)
    n_d2 = int((dv[:, :kk] != da[:, :kk]).sum())
    rows_differ = (dv[:, :kk] != da[:, :kk]).any(1).cpu().numpy()
    print(f"{c.name}: {n_d2} of {c.nq * kk} d2 values differ between the offset view and its aligned copy; "
          f"{int((q2v != q2a).sum())} of {c.nq} query norms differ between the two forms")
    assert not rows_differ[q2v == q2a].any()              # equal norms: equal rows
    if c.d % 4 == 0:
        assert n_d2 > 0
