"""The search front's shape table (tests/search_plan_cases.py) against itself, on the CPU: every case's declared branch is what the
restatement of plan_search plans for its shape, every value of every branch field and both sides of every boundary are in the
table, the stress data does to the margin what its case says, and the all-queries float64 check -- with the float64 distances' own
top-k standing in for the device's result -- leaves at most 1 % of the pairs of every case undecided (a property of the data
and the tolerance alone).  The device's side is tests/test_gpu_search_plan.py."""
import numpy as np
import pytest

import fp32_emu as E
import search_plan_cases as T

CASES = T.CASES
PLANS = {c.name: T.case_plan(c) for c in CASES}
CPU_CASES = [c for c in CASES if c.n * c.nq * c.d <= 2 ** 31]


def _find(**want):
    """The cases whose attributes / plan entries equal `want`."""
    out = []
    for c in CASES:
        p = PLANS[c.name]
        if all((getattr(c, f) if hasattr(c, f) else p[f]) == v for f, v in want.items()):
            out.append(c)
    return out


def test_restatement_reproduces_the_plans_the_library_documents():
    # DESIGN.md / search.hip: 1 M rows plan strides 256, 16, 1 (rigorous), 4096, 256, 16, 1 (guessed batch), 256 | 1 (one image)
    p = T.plan(1_000_000, 1024, 10_000, 200)
    assert (p["rig_levels"], p["rig_stride0"], p["levels"], p["stride0"], p["guessed"]) == (2, 256, 3, 4096, True)
    p = T.plan(1_000_000, 1024, 50, 200)
    assert (p["small"], p["levels"], p["stride0"], p["form"]) == (True, 1, 256, "single")
    assert T.plan(250_000, 1024, 50, 200)["stride0"] == 64 and T.plan(125_000, 1024, 10_000, 200)["stride0"] == 256
    assert T.heur_rank(20) == 19 and T.heur_rank(19) == 19 and T.heur_rank_small(200, 256) == 7
    # tests/test_gpu_select_regimes.py: 65543 rows, k = 20: two levels, 1040 rows carry 4097 rows, 192 rows do not
    assert T.plan(65543, 64, 1040, 20)["carry_rows"] == 4097 and T.plan(65543, 64, 192, 20)["carry_rows"] == 0
    assert T.plan(65543, 64, 1040, 20)["levels"] == 2 and T.plan(65543, 64, 1040, 10)["levels"] == 1


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_declared_branch_is_the_planned_one(c):
    p = PLANS[c.name]
    assert T.declared(c) == T.planned(p), p
    assert 1 <= c.k <= 1024 and c.q_offset in (0, 1)
    assert (c.flags == "zero") == (not p["guessed"] and c.data != "mixed"), "rigorous thresholds never flag but for the margin's overflow"
    assert c.fp64 == (c.data in ("gauss", "unit", "unit_far")) and c.emulate_all == (not c.fp64)
    if c.emulate_all:
        assert c.d == 64 and 32768 < c.n <= 33500 and c.nq <= 16
    rows = T.emulated_rows(c)
    assert len(rows) >= min(c.nq, 8) and {0, c.nq - 1} <= set(rows) and {r for r in (127, 128, 16383, 16384) if r < c.nq} <= set(rows)


def test_every_branch_value_is_reached():
    assert {c.filter for c in CASES} == {"none", "f16", "bf16x3", "fp32"}
    assert {c.levels for c in CASES} == {0, 1, 2}
    assert {c.carry for c in CASES} == {False, True}
    assert {c.form for c in CASES} == {"matrix", "single", "batch"}
    assert {c.flags for c in CASES} == {"zero", "rare", "nonzero"}
    assert {c.q_offset for c in CASES if c.filter == "none"} == {0, 1} and {c.q_offset for c in CASES if c.filter == "f16"} == {0, 1}
    for f in ("f16", "bf16x3"):
        assert {PLANS[c.name]["guessed"] for c in CASES if c.filter == f} == {False, True}, f
        assert {c.form for c in CASES if c.filter == f and PLANS[c.name]["guessed"]} == {"single", "batch"}, f
    assert not any(PLANS[c.name]["guessed"] for c in CASES if c.filter == "fp32")
    # level 0's forms (FilterLists needs rows of d >= 4096: see the table's docstring), the K split, two chunks, both preparations
    assert {f for c in CASES for f in PLANS[c.name]["l0"]} == {"SplitReduce", "SampleF16", "ExactGemm"}
    assert any(len(PLANS[c.name]["l0"]) == 2 for c in CASES)
    assert {PLANS[c.name]["fuse_qn"] for c in CASES if c.filter == "f16" and c.form == "single"} == {False, True}
    assert {PLANS[c.name]["wide_prep"] for c in CASES if c.filter == "f16" and c.form == "single"} == {False, True}
    # the matrix path's axes
    m = [c for c in CASES if c.filter == "none" and c.n <= 257]
    assert {c.d for c in m} == {1, 3, 5, 30, 33, 50, 63, 65, 100, 4, 36, 32, 64}
    assert {c.n for c in m} == {1, 127, 128, 129, 257} and {c.nq for c in m} == {1, 127, 128, 129, 257}
    assert {"1" if c.k == 1 else {-1: "n-1", 0: "n", 3: "n+3"}.get(c.k - c.n) for c in m if not c.q_offset} == {"1", "n-1", "n", "n+3"}
    for axis in ("d", "n", "nq"):
        # every value of every axis meets a guarded (partial tile) and an unguarded (whole tile) neighbour on another axis
        for v in {getattr(c, axis) for c in m}:
            others = [(c.n % 128 == 0, c.nq % 128 == 0, c.d % 32 == 0) for c in m if getattr(c, axis) == v]
            drop = {"n": 0, "nq": 1, "d": 2}[axis]
            seen = {tuple(x for i, x in enumerate(o) if i != drop) for o in others}
            assert any(True in s for s in seen) and any(False in s for s in seen), (axis, v, seen)
    # the filter path's sizes and widths
    f = [c for c in CASES if c.filter != "none" and c.data in ("unit", "unit_far")]
    assert {32769, 32784, 32785} <= {c.n for c in f if c.d == 64}
    assert {c.d for c in f} >= {64, 96, 32, 48, 50, 2112}
    for flt in ("f16", "bf16x3", "fp32"):
        assert {1, 128, 129} <= {c.nq for c in f if c.filter == flt}, flt
    for nq in (40, 192):
        assert {1, 19, 20} <= {c.k for c in f if c.d == 64 and c.nq == nq and c.n == 32769}


def test_both_sides_of_every_boundary():
    # n = 32768 | 32769 at d = 64: the last matrix-path size, the first filtered one
    assert _find(n=32768, d=64, filter="none") and _find(n=32769, d=64, filter="f16")
    # k = 19 | 20: rigorous | guessed, one image and a batch, same index
    for nq in (40, 192):
        assert _find(n=32769, d=64, nq=nq, k=19, guessed=False) and _find(n=32769, d=64, nq=nq, k=20, guessed=True)
    # nq = 128 | 129: one image | a batch, on each arithmetic
    for flt in ("f16", "bf16x3", "fp32"):
        assert _find(filter=flt, nq=128, form="single") and _find(filter=flt, nq=129, form="batch"), flt
    # nq d <= 2^18 | beyond: the one-workgroup preparation | the many-workgroup one
    assert _find(filter="f16", form="single", wide_prep=False) and _find(filter="f16", d=2112, nq=128, wide_prep=True)
    assert 128 * 2048 == 2 ** 18 < 128 * 2112
    # n / stride0 < 4 k on more than 32768 rows: the matrix path | the filter
    assert _find(n=40000, k=700, filter="none") and _find(n=40000, k=600, filter="f16")
    assert T.plan(40000, 64, 16, 625)["matrix"] is False and T.plan(40000, 64, 16, 626)["matrix"] is True      # 2500 < 4 k from k = 626
    # 16384 | 16385 query rows: one chunk | two; carry | the same case without
    assert len(PLANS[_find(nq=16385)[0].name]["l0"]) == 2 and all(len(PLANS[c.name]["l0"]) == 1 for c in CASES if c.nq <= 16384 and c.filter != "none")
    a, b = _find(nq=1040, carry=True), _find(nq=1040, carry=False)
    assert a and b and (a[0].n, a[0].d, a[0].k) == (b[0].n, b[0].d, b[0].k) and b[0].opts == {"level_carry": 0}


@pytest.mark.parametrize("c", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_fp64_check_decides_all_but_one_percent(c):
    """The all-queries check on the float64 distances' own top-k: it passes, and what it leaves undecided is the data's doing."""
    import torch

    R, Q = (torch.from_numpy(x) for x in T.make_data(c))
    d2, idx = T.fp64_topk(Q, R, c.k)
    if not c.fp64:
        # the stress data: the band of the k-th neighbour holds more rows than any tolerance can tell apart
        und, total = T.check_all_queries(Q, R, d2, idx, c.k)
        assert und > 0.5 * total, (und, total)
        return
    und, total = T.check_all_queries(Q, R, d2, idx, c.k)
    print(f"{c.name}: {und} of {total} pairs undecided")
    assert und <= 0.01 * total, (und, total)
    # and the check bites: one neighbour replaced by a row far outside the band fails it
    if min(c.k, c.n) < c.n:
        far = torch.from_numpy(np.argmax(((Q[0].double()[None, :] - R.double()) ** 2).sum(1).numpy())[None])
        bad = idx.clone()
        bad[0, 0] = far[0]
        with pytest.raises(AssertionError):
            T.check_all_queries(Q, R, d2, bad, c.k)


def test_stress_data_does_what_its_case_says():
    for c in T.STRESS:
        R, Q = T.make_data(c)
        over = T.margin_overflows(Q, R, c.k)
        if c.data == "clump":
            assert not over.any()
            continue
        if c.data == "mixed":
            assert over.all() and c.flags == "nonzero"            # every list outgrows its 8192 entries
            r2 = (R.astype(np.float64) ** 2).sum(1)
            assert (r2 > 1e5).sum() == 6 and abs(np.sqrt((Q[-1].astype(np.float64) ** 2).sum()) - 1e-2) < 1e-6
        else:
            assert not over.any() and c.flags == "rare"
            # the shell: 3 k rows per query within 1e-6 relative of one distance, closer than every other row; the emulated top-k
            # holds exact ties (the duplicates, and whatever else fp32 makes equal)
            m, ties = 3 * c.k, 0
            q2 = E.row_sumsq(Q)
            for j in range(c.nq):
                ids = 5 + T.SHELL_STEP * (m * j + np.arange(m))
                d64 = ((Q[j].astype(np.float64)[None, :] - R.astype(np.float64)) ** 2).sum(1)
                shell = d64[ids]
                assert (shell.max() - shell.min()) <= 1e-6 * shell.min()
                rest = np.delete(d64, ids)
                assert rest.min() > 1.5 * shell.max()
                assert np.array_equal(R[ids[3]], R[ids[m // 2]])
                demu = E.d2(q2[j], E.row_sumsq(R[ids]), E.dot_chain(Q[j], R[ids]))
                top = np.sort(demu)[:c.k]
                ties += int((np.diff(top) == 0).sum())
                assert len(np.unique(demu)) > 1 or j > 0          # ... and not ONE value either: the order is decided by bits
            assert ties > 0


def test_clump_sits_at_three_quarters_of_the_margin():
    """The clump case's data against a NumPy model of the filter's product (operands scaled by a power of two and rounded to fp16, as
    tests/test_knn_model.py models it): every pair's d2~ stays within the margin eps = c_eps ||q|| max||r|| -- and the k nearest rows
    of every query lie more than eps / 2 above level 0's exact threshold, so a margin of half the size would lose them."""
    from test_knn_model import pow2_scale

    (c,) = [c for c in T.STRESS if c.data == "clump"]
    R, Q = T.make_data(c)
    ids = T.clump_ids(c.k)
    assert len(ids) == 3 * c.k and (ids % 16 == 0).sum() >= c.k and (ids % 16 != 0).sum() >= c.k
    Q64, R64 = Q.astype(np.float64), R.astype(np.float64)
    q2, r2 = (Q64 * Q64).sum(1), (R64 * R64).sum(1)
    D = q2[:, None] + r2[None, :] - 2.0 * (Q64 @ R64.T)
    sq, sr = pow2_scale(np.abs(Q).max()), pow2_scale(np.abs(R).max())
    Qh = (Q * np.float32(sq)).astype(np.float16).astype(np.float64)
    Rh = (R * np.float32(sr)).astype(np.float16).astype(np.float64)
    Dt = q2[:, None] + r2[None, :] - 2.0 * (Qh @ Rh.T) / (sq * sr)
    eps = T.f16_c_eps(c.d) * np.sqrt(q2 * r2.max())
    assert (np.abs(Dt - D) <= eps[:, None]).all()
    t0 = np.sort(D[:, ::16], axis=1)[:, c.k - 1]                      # level 0: the exact k-th distance of the stride-16 sample
    near = np.argsort(D, axis=1)[:, :c.k]
    assert np.isin(near, ids).all() and (np.delete(D, ids, axis=1).min(1) > 1.0).all()
    over = np.take_along_axis(Dt, near, 1) - t0[:, None]
    print(f"clump: d2~ - T0 over eps in [{(over / eps[:, None]).min():.3f}, {(over / eps[:, None]).max():.3f}]")
    assert (over > 0.5 * eps[:, None]).all() and (over <= eps[:, None]).all()
    assert not T.margin_overflows(Q, R, c.k).any()


def test_wide_case_tol64():
    """The widest case's tol64 is twice the emulation's own worst deviation from float64 on that case's data."""
    (c,) = [c for c in CASES if c.d == 2112]
    R, Q = T.make_data(c)
    worst = 0.0
    for q in T.emulated_rows(c):
        near = np.argsort(-(R @ Q[q]), kind="stable")[:c.k + 64]           # unit rows: a plain fp32 product finds the neighbourhood
        d64 = ((Q[q].astype(np.float64)[None, :] - R[near].astype(np.float64)) ** 2).sum(1)
        order = np.argsort(d64, kind="stable")[:c.k]
        ids, d64 = near[order], d64[order]
        demu = E.d2(E.row_sumsq(Q[q:q + 1])[0], E.row_sumsq(R[ids]), E.dot_chain(Q[q], R[ids]))
        worst = max(worst, float(np.abs(demu - d64).max()))                # unit rows: the scale is 1
    print(f"emulated fp32 against float64 at d = {c.d}: worst {worst:.3e}")
    assert worst <= c.tol64 <= 2.0 * worst * 1.02 and c.tol64 < 4e-6, (worst, c.tol64)      # ... and inside the all-queries tolerance
