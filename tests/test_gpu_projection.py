"""segvlad_pca_apply -- the library's general "NT" GEMM (describe stage, device PCA fit, segvlad_images_pca's fall-back) -- per
output ENTRY against float64, across its dispatch: the fp16 two-term split kernel with 128 and 256 tiles, split-K with a short
last slice, direct and reducing epilogues, forced tiles, the XCD-aware tile order, and the fp32 kernel's fast / edge / ragged-K /
scalar-load loops.  Reference and bound: tests/projection_ref.py (derivation there; tests/test_projection_bound.py shows on the
CPU that the bound passes a healthy emulation of the split and fails three broken ones).  Every entry of every case is held to

    |y - ref| <= 4 e_np[m] + 3 2^-22 cs[j] sum_k |A[m,k]| |W[j,k]|  (+ the two sub-normal terms for rows below 2^-12 of the maximum)

(fp32 kernel: the first term alone), where e_np[m] is the worst error of numpy's fp32 product of the same operands in row m.
Three families are bit-for-bit identities: the tile ORDER (x3_gm) against the default order, l2norm=True against normalize_rows
of the l2norm=False result, and a used context against a fresh one.  Run with `-m gpu` on an MI355X; conftest.py's guard mode
(fenced, exact-size scratch) is what gives the "big call, then small call" cases their teeth.

Measured on an MI355X (max over entries of |err| / bound; worst row's max|err| / max|ref|):

    case                                                       err/bound   row rel err
    x3 (1, 32, 1) whiten=1 mean=1                               0.002    1.13e-08
    x3 (1, 32, 1) whiten=1 mean=0                               0.008    5.98e-08
    x3 (1, 32, 1) whiten=0 mean=1                               0.004    3.20e-08
    x3 (1, 32, 1) whiten=0 mean=0                               0.007    5.23e-08
    x3 (5, 64, 7) whiten=1 mean=1                               0.053    1.86e-07
    x3 (5, 64, 7) whiten=1 mean=0                               0.074    1.49e-07
    x3 (5, 64, 7) whiten=0 mean=1                               0.065    1.40e-07
    x3 (5, 64, 7) whiten=0 mean=0                               0.079    1.62e-07
    x3 (130, 1056, 129) whiten=1 mean=1                         0.036    3.06e-07
    x3 (130, 1056, 129) whiten=1 mean=0                         0.040    3.44e-07
    x3 (130, 1056, 129) whiten=0 mean=1                         0.035    3.08e-07
    x3 (130, 1056, 129) whiten=0 mean=0                         0.039    2.83e-07
    x3 (333, 2048, 200) whiten=1 mean=1                         0.034    3.34e-07
    x3 (333, 2048, 200) whiten=1 mean=0                         0.035    3.41e-07
    x3 (333, 2048, 200) whiten=0 mean=1                         0.039    3.72e-07
    x3 (333, 2048, 200) whiten=0 mean=0                         0.042    3.46e-07
    x3 (1024, 96, 256) whiten=1 mean=1                          0.077    2.41e-07
    x3 (1025, 96, 257) whiten=1 mean=1                          0.095    3.20e-07
    x3 (1300, 32, 300) whiten=1 mean=1                          0.147    2.96e-07
    x3 (130, 1056, 129) whiten=1 mean=1 x3_tile=256             0.036    3.06e-07
    x3 (1025, 96, 257) whiten=1 mean=1 x3_tile=128              0.095    3.20e-07
    fp32 (70, 180, 40)                                          0.250    7.15e-07
    fp32 (70, 250, 40)                                          0.250    8.54e-07
    fp32 (130, 1000, 129)                                       0.328    3.83e-07
    fp32 (130, 1001, 129)                                       0.270    3.34e-07
    fp32 (256, 1024, 128)                                       0.475    4.00e-07
    fp32 (130, 1024, 70)                                        0.305    4.14e-07
    dyn x 2^-12                                                 0.026    2.92e-07
      dyn x 2^-12: small rows rel err 2.5e-07, numpy fp32 8.2e-07
    dyn x 2^-20                                                 0.040    9.60e-06
      dyn x 2^-20: small rows rel err 9.6e-06, numpy fp32 8.2e-07
    dyn w 2^-12                                                 0.030    3.43e-07
    dyn w 2^-12 (column yardstick)                              0.035    3.43e-07
      dyn w 2^-12: small columns rel err 2.5e-07, numpy fp32 7.2e-07
    dyn w 2^-20                                                 0.030    3.43e-07
    dyn w 2^-20 (column yardstick)                              0.042    3.43e-07
      dyn w 2^-20: small columns rel err 9.5e-06, numpy fp32 7.2e-07
    nan row, batch x 2^0                                        0.023    2.80e-07
    nan row, batch x 2^-12                                      0.023    2.80e-07
    stale rows: (5, 32, 300) after (1300, 32, 300)              0.072    1.61e-07
    model change: (5, 64, 7) after P=300, KD=32                 0.053    1.86e-07

    normalize_rows, worst entry in ulp of the float64 quotient (d x n):
      1x1: 0.00   1x5: 0.00   3x1: 1.15   3x5: 1.01   4x1: 0.75   4x5: 0.77   63x1: 0.81
      63x5: 1.18   64x1: 0.96   64x5: 1.39   260x1: 0.56   260x5: 1.47   1024x1: 1.15   1024x5: 1.54
"""
import numpy as np
import pytest
from conftest import engine_scope

import projection_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope=engine_scope)
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def fresh_engine():
    from revisit_anything_amd.engine import SegVLADEngine

    return SegVLADEngine(0)


def set_model(eng, mean, W, var, whiten):
    eng.pca_set(mean, W, var if whiten else None, whiten=whiten)


def apply(eng, X, **kw):
    return eng.pca_apply(X, **kw).cpu().numpy()


def apply_into_nan(eng, X):
    """pca_apply into an output tensor pre-filled with NaN: an entry that no workgroup writes cannot pass by leftovers"""
    import torch

    out = torch.full((X.shape[0], eng.P), float("nan"), dtype=torch.float32, device=eng.device)
    return eng.pca_apply(X, out=out).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the split path
# ------------------------------------------------------------------------------------------------
def run_x3_case(eng, shape, whiten, with_mean, tag=""):
    n, KD, P = shape
    X, mean, W, var, cs = PR.make_case(n, KD, P, whiten, with_mean)
    ref = PR.Ref(X, mean, W, cs, "x3")
    assert not ref.small_x.any() and not ref.small_w.any()        # the reduced bound: fp32 class per row
    set_model(eng, mean, W, var, whiten)
    y = apply_into_nan(eng, X)
    ref.check(f"x3 {shape} whiten={int(whiten)} mean={int(with_mean)}{tag}", y)
    return X, y


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("shape", PR.X3_SMALL_TILE)
def test_x3_small_tile(eng, shape, whiten, with_mean):
    X, y = run_x3_case(eng, shape, whiten, with_mean)
    # l2norm=True normalises the projected rows IN PLACE: the same kernel on the same values -> the same bits
    yn = apply(eng, X, l2norm=True)
    assert np.array_equal(bits(yn), bits(eng.normalize_rows(y).cpu().numpy()))


@pytest.mark.parametrize("shape", PR.X3_BIG_TILE)
def test_x3_big_tile(eng, shape):
    X, y = run_x3_case(eng, shape, True, True)
    yn = apply(eng, X, l2norm=True)
    assert np.array_equal(bits(yn), bits(eng.normalize_rows(y).cpu().numpy()))


@pytest.mark.parametrize("shape,tile", [((130, 1056, 129), 256), ((1025, 96, 257), 128)])
def test_x3_forced_tile(eng, shape, tile):
    try:
        eng.set_option("x3_tile", tile)
        run_x3_case(eng, shape, True, True, tag=f" x3_tile={tile}")
    finally:
        eng.set_option("x3_tile", 0)


@pytest.mark.parametrize("shape", [(333, 2048, 200), (1025, 96, 257)])
def test_x3_tile_order_changes_no_bit(eng, shape):
    """x3_gm re-orders the tiles over the workgroups (blocks of gm x 32/gm tiles per XCD); slices and arithmetic stay, so every
    order must reproduce the default order's output bit for bit -- and cover every tile (NaN-filled output)."""
    _, y0 = run_x3_case(eng, shape, True, True)
    n, KD, P = shape
    X = PR.make_case(n, KD, P, True, True)[0]
    try:
        for gm in (1, 4, 32):
            eng.set_option("x3_gm", gm)
            y = apply_into_nan(eng, X)
            assert not np.isnan(y).any(), (gm, "entries never written:", int(np.isnan(y).sum()))
            assert np.array_equal(bits(y), bits(y0)), gm
    finally:
        eng.set_option("x3_gm", -1)


# ------------------------------------------------------------------------------------------------
# the fp32 kernel
# ------------------------------------------------------------------------------------------------
FP32_CASES = [((70, 180, 40), False), ((70, 250, 40), False), ((130, 1000, 129), False), ((130, 1001, 129), False),
              ((256, 1024, 128), True), ((130, 1024, 70), True)]          # True: KD % 32 == 0, reached with pca_arith=fp32


@pytest.mark.parametrize("shape,force", FP32_CASES)
def test_fp32_kernel(eng, shape, force):
    n, KD, P = shape
    assert force == (KD % 32 == 0)
    X, mean, W, var, cs = PR.make_case(n, KD, P, True, True)
    ref = PR.Ref(X, mean, W, cs, "fp32")
    try:
        if force:
            eng.set_option("pca_arith", "fp32")
        set_model(eng, mean, W, var, True)
        y = apply_into_nan(eng, X)
    finally:
        eng.set_option("pca_arith", "auto")
    ref.check(f"fp32 {shape}", y)


# ------------------------------------------------------------------------------------------------
# dynamic range: one scale per batch and one per model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,e", PR.DYN_CASES)
def test_x3_dynamic_range(eng, side, e):
    """Half of the rows of X (or of W: the PCA fit's X^T operand) scaled by 2^-12 and 2^-20.  At 2^-12 both fp16 terms of every
    significant element are still normal: the reduced bound, fp32 class per row.  At 2^-20 the second terms are sub-normal and the
    full bound holds (absolute error per element <= 2^-25 of the scaled unit); the small rows' relative error is recorded beside
    numpy's fp32 product's."""
    X, mean, W, var, cs = PR.make_dyn_case(side, e)
    ref = PR.Ref(X, mean, W, cs, "x3", all_reduced=(e == 12))
    small = ref.small_x if side == "x" else ref.small_w
    assert small[len(small) // 2:].all() == (e == 20) and not small[:len(small) // 2].any()
    set_model(eng, None, W, var, False)
    y = apply_into_nan(eng, X)
    ref.check(f"dyn {side} 2^-{e}", y)
    h = len(small) // 2
    if side == "x":
        rel, rel_np = ref.row_rel(y)[h:].max(), (ref.e_np / ref.row_ref_max)[h:].max()
    else:
        # a small row of W is a small output COLUMN, which the row yardstick cannot see: the transposed yardstick as well
        refc = PR.Ref(X, mean, W, cs, "x3", all_reduced=(e == 12), yardstick="col")
        refc.check(f"dyn {side} 2^-{e} (column yardstick)", y)
        rel, rel_np = refc.col_rel(y)[h:].max(), (refc.e_np_col / np.abs(refc.ref).max(axis=0))[h:].max()
    print(f"[projection] dyn {side} 2^-{e}: small {'rows' if side == 'x' else 'columns'} rel err {rel:.1e}, numpy fp32 {rel_np:.1e}")


# ------------------------------------------------------------------------------------------------
# isolation and context state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_scale", [0, -12])
def test_one_nan_row_stays_in_its_row(eng, log2_scale):
    """Row 7 of X is NaN: row 7 of the output is NaN, every other row is finite and inside the bound computed WITHOUT row 7 -- the
    batch scale must come from the finite entries.  (log2_scale = -12: the same batch at 2^-12 of the magnitude, where a scale
    of 1 instead of the batch's would put every first fp16 term into the sub-normals.)"""
    n, KD, P = 40, 2048, 48
    X, mean, W, var, cs = PR.make_case(n, KD, P, True, True)
    X = (X * np.float32(2.0 ** log2_scale)).astype(np.float32)
    mean = (mean * np.float32(2.0 ** log2_scale)).astype(np.float32)
    keep = np.arange(n) != 7
    ref = PR.Ref(X[keep], mean, W, cs, "x3")
    Xn = X.copy()
    Xn[7] = np.nan
    set_model(eng, mean, W, var, True)
    y = apply_into_nan(eng, Xn)
    assert np.isnan(y[7]).all()
    assert np.isfinite(y[keep]).all()
    ref.check(f"nan row, batch x 2^{log2_scale}", y[keep])


def test_stale_plane_rows_do_not_leak(eng):
    """The blocked fp16 planes are padded to whole 256-row tiles and only n rows are written.  A big call with rows of 6e4 (finite,
    near the top of the fp16 range after scaling) leaves such rows behind; the small call after it must equal, bit for bit, the
    same call on a fresh context."""
    mean, W, var = PR.make_case(1, 32, 300)[1:4]
    Xbig = PR.make_case(1300, 32, 300)[0] * np.float32(6e4 * np.sqrt(32) / 4)       # |x| up to ~6e4
    assert 3e4 < np.abs(Xbig).max() < 3e5
    m7, W7, var7 = PR.make_case(5, 32, 7)[1:4]
    Xs = PR.make_case(5, 32, 7)[0]
    set_model(eng, mean, W, var, True)
    ybig = apply_into_nan(eng, Xbig)
    assert np.isfinite(ybig).all()
    set_model(eng, m7, W7, var7, True)          # "the same model" for the small call on both contexts
    y_used = apply_into_nan(eng, Xs)
    # ... and with the big call's OWN model (P = 300), rows 5.. of the planes stale
    set_model(eng, mean, W, var, True)
    apply_into_nan(eng, Xbig)
    y_used_300 = apply_into_nan(eng, Xs)
    f = fresh_engine()
    try:
        set_model(f, m7, W7, var7, True)
        y_fresh = apply_into_nan(f, Xs)
        set_model(f, mean, W, var, True)
        y_fresh_300 = apply_into_nan(f, Xs)
    finally:
        f.close()
    assert np.array_equal(bits(y_used), bits(y_fresh))
    assert np.array_equal(bits(y_used_300), bits(y_fresh_300))
    PR.Ref(Xs, mean, W, PR.col_scale(var, True), "x3").check("stale rows: (5, 32, 300) after (1300, 32, 300)", y_used_300)


def test_model_change_leaves_nothing_behind(eng):
    """pca_set (P = 300, KD = 32), then pca_set (P = 7, KD = 64), then pca_apply: bitwise the fresh context's result."""
    mean, W, var = PR.make_case(1, 32, 300)[1:4]
    X, m7, W7, var7, cs7 = PR.make_case(5, 64, 7)
    set_model(eng, mean, W, var, True)
    set_model(eng, m7, W7, var7, True)
    y_used = apply_into_nan(eng, X)
    f = fresh_engine()
    try:
        set_model(f, m7, W7, var7, True)
        y_fresh = apply_into_nan(f, X)
    finally:
        f.close()
    assert np.array_equal(bits(y_used), bits(y_fresh))
    PR.Ref(X, m7, W7, cs7, "x3").check("model change: (5, 64, 7) after P=300, KD=32", y_used)


# ------------------------------------------------------------------------------------------------
# normalize_rows alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 260, 1024])
def test_normalize_rows(eng, d, n):
    """Scalar (d % 4 != 0) and float4 loads, one to four trips of the 64-lane loop, a last workgroup with one live wave (n = 5: four
    rows per workgroup).  Per entry within 2 ulp of the float64 quotient."""
    X = np.random.Generator(np.random.PCG64(100 + d + n)).standard_normal((n, d)).astype(np.float32)
    y = eng.normalize_rows(X).cpu().numpy()
    X64 = X.astype(np.float64)
    ref = X64 / np.linalg.norm(X64, axis=1, keepdims=True)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = (np.abs(y - ref) / ulp).max()
    print(f"[projection] normalize_rows d={d} n={n}: worst {worst:.2f} ulp")
    # 2 ulp: half an ulp for the quotient's rounding, up to one for the norm's (2^-24 relative is an ulp of an entry at the top of
    # its binade), and the fp32 sum of squares: a lane's chain of at most 16 fma (d = 1024) plus the 6-step butterfly, a random
    # walk of a few 2^-25 relative on the sum, HALF of which reaches the norm.  Not a worst-case bound (22 roundings could add up
    # to 11 ulp): for these seeded rows the exact host emulation of the device's sum (fp32_emu.row_sumsq) with correctly rounded
    # sqrt and division gives at most 1.54 ulp (d = 1024, n = 5), so d = 1024 needs no more than the others.
    assert (np.abs(y - ref) <= 2.0 * ulp).all(), worst


def test_normalize_rows_zero_row_is_nan_and_alone(eng):
    """r / ||r|| of a zero row is 0 / 0 = NaN, as in the reference; its neighbours in the same workgroup are untouched."""
    for d in (3, 64):
        X = np.random.Generator(np.random.PCG64(300 + d)).standard_normal((5, d)).astype(np.float32)
        want = eng.normalize_rows(X).cpu().numpy()
        X0 = X.copy()
        X0[1] = 0
        y = eng.normalize_rows(X0).cpu().numpy()
        assert np.isnan(y[1]).all()
        keep = np.arange(5) != 1
        assert np.array_equal(bits(y[keep]), bits(want[keep]))
