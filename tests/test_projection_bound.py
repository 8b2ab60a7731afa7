"""tests/projection_ref.py on the CPU: the per-entry bound that tests/test_gpu_projection.py holds segvlad_pca_apply to must pass a
healthy host emulation of the fp16 two-term split (fp16 rounding of f and f - h1, fp32 accumulation in 32-deep blocks, split-K
slices as launch_x3 cuts them) at every split-path shape of the device test -- and must FAIL each of three broken ones: a cross
product left out, the last 32-deep k-block of one slice skipped, the column scale applied twice.  That is the proof that the
bound can fail."""
import numpy as np
import pytest

import projection_ref as PR

DEEP = [(16, 6144, 12)]       # one deeper K than the device test's (the describe stage's descriptors are deeper still)


def test_plan_matches_the_documented_slices():
    assert PR.x3_plan(1, 32, 1) == (128, 32, 1)                 # one k-block, direct epilogue
    assert PR.x3_plan(5, 7, 64) == (128, 32, 2)                 # two slices
    assert PR.x3_plan(130, 129, 1056) == (128, 64, 17)          # 16 slices of 64 and a last one of 32
    assert PR.x3_plan(1300, 300, 32) == (256, 32, 1)
    assert PR.x3_plan(1025, 257, 96)[0] == 256 and PR.x3_plan(1025, 257, 96, tile=128)[0] == 128


@pytest.mark.parametrize("shape", PR.X3_SMALL_TILE + PR.X3_BIG_TILE + DEEP)
def test_healthy_emulation_is_inside_the_bound(shape):
    n, KD, P = shape
    for whiten, with_mean in ((True, True), (False, False)):
        X, mean, W, _, cs = PR.make_case(n, KD, P, whiten, with_mean)
        ref = PR.Ref(X, mean, W, cs)
        assert not ref.small_x.any() and not ref.small_w.any()          # reduced bound everywhere
        w = ref.check(f"emu {shape} whiten={whiten} mean={with_mean}", PR.emulate_x3(X, mean, W, cs))
        assert w < 0.5       # healthy arithmetic is nowhere near the bound (0.04 .. 0.2 here)


@pytest.mark.parametrize("side,e", PR.DYN_CASES + [("x", 24), ("w", 24)])
def test_healthy_emulation_dynamic_range(side, e):
    X, mean, W, _, cs = PR.make_dyn_case(side, e)
    ref = PR.Ref(X, mean, W, cs, all_reduced=(e == 12))      # scaled by 2^-12: the reduced bound, fp32 class per row
    small = ref.small_x if side == "x" else ref.small_w
    other = ref.small_w if side == "x" else ref.small_x
    assert not other.any()
    if e == 12:
        assert not small.any()
    else:
        assert small[len(small) // 2:].all() and not small[:len(small) // 2].any()
    y = PR.emulate_x3(X, mean, W, cs)
    ref.check(f"emu dyn {side} 2^-{e}", y)
    # the property itself: per-row relative error of the small rows beside a plain fp32 product's
    if side == "x":
        rr = ref.row_rel(y)[len(small) // 2:].max()
        rr_np = (ref.e_np / ref.row_ref_max)[len(small) // 2:].max()
        print(f"[projection] emu dyn x 2^-{e}: small rows rel err {rr:.1e}, numpy fp32 {rr_np:.1e}")
        if e == 12:
            assert rr < 4e-6
        if e == 24:
            assert rr > 10 * rr_np                   # the loss is real: the header must not promise fp32 class down there
    else:
        # a small row of W is a small output COLUMN: the row yardstick is blind to it, the transposed one is not
        refc = PR.Ref(X, mean, W, cs, all_reduced=(e == 12), yardstick="col")
        refc.check(f"emu dyn {side} 2^-{e} (column yardstick)", y)
        cr = refc.col_rel(y)[len(small) // 2:].max()
        cr_np = (refc.e_np_col / np.abs(refc.ref).max(axis=0))[len(small) // 2:].max()
        print(f"[projection] emu dyn w 2^-{e}: small columns rel err {cr:.1e}, numpy fp32 {cr_np:.1e}")
        if e == 12:
            assert cr < 4e-6
        if e == 24:
            assert cr > 10 * cr_np


BROKEN = [dict(drop="a1b2"), dict(drop="a2b1"), dict(skip_last_block_of_slice=0), dict(cs_twice=True)]


@pytest.mark.parametrize("shape", [(130, 1056, 129), (333, 2048, 200), (1025, 96, 257)])
@pytest.mark.parametrize("how", BROKEN, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_broken_emulations_are_outside_the_bound(shape, how):
    n, KD, P = shape
    X, mean, W, _, cs = PR.make_case(n, KD, P, whiten=True, with_mean=True)
    ref = PR.Ref(X, mean, W, cs)
    y = PR.emulate_x3(X, mean, W, cs, **how)
    w = ref.report(f"broken {how} {shape}", y)
    assert w > 4.0, w                                # (dropping a cross product overshoots 10 to 30 times)
    with pytest.raises(AssertionError):
        ref.check("broken", y)


def test_a_single_wrong_entry_or_a_nan_fails():
    X, mean, W, _, cs = PR.make_case(5, 64, 7)
    ref = PR.Ref(X, mean, W, cs)
    y = PR.emulate_x3(X, mean, W, cs)
    ref.check("ok", y)
    for bad in (np.float32(np.nan), y[3, 2] * np.float32(1.0 + 1e-4)):
        z = y.copy()
        z[3, 2] = bad
        with pytest.raises(AssertionError):
            ref.check("one entry", z)


def test_fp32_path_bound_is_the_first_line_only():
    X, mean, W, _, cs = PR.make_case(70, 180, 40)
    a, b = PR.Ref(X, mean, W, cs, "fp32"), PR.Ref(X, mean, W, cs, "x3")
    assert np.array_equal(a.bound, 4.0 * a.e_np[:, None] * np.ones_like(a.ref)) and (b.bound > a.bound).all()
