"""Reference, per-entry error bound and host emulation for segvlad_pca_apply (test infrastructure, pure numpy; used by
tests/test_gpu_projection.py on the device and by tests/test_projection_bound.py on the CPU).

For X [n, KD], mean [KD] or None, W [P, KD] and cs [P] (the column scale: 1/sqrt(var) as fp32, or 1), all taken as their fp32
values and evaluated in float64:

    A   = X - mean                          ref = (A W^T) * cs
    e_np[m] = max_j |fp32 numpy product of the same operands - ref|[m, j]     (the yardstick: independent of the code under test)
    B   = max|X| + max|mean|                Wm  = max|W|

    bound[m, j] = 4 e_np[m]
                + 3 2^-22 cs[j] sum_k |A[m,k]| |W[j,k]|          dropped terms of the two-term fp16 split, elementwise
                + 2^-25 (B  / 2^13) cs[j] sum_k |W[j,k]|         only where row m of A is "small": its second fp16 terms are sub-normal
                + 2^-25 (Wm / 2^13) cs[j] sum_k |A[m,k]|         only where row j of W is "small"

The factor 4 over numpy is a margin for another summation order (32-deep MFMA chunks and split-K slices added in index order
against the BLAS's blocking) on a random-walk error; it is not a measurement of the kernel.  The other terms are derived:

  * x s = h1 + h2 + e with |e| <= 2^-22 |x s| for an element whose two fp16 terms are normal; the three products kept are
    (h1 + h2)(g1 + g2) - h2 g2, so the entry loses at most (2^-22 + 2^-22 + 2^-22) |a| |w| per element.
  * The library scales a whole batch by ONE power of two s with B s in [2^13, 2^14) (and the model by one with Wm s_w in the same
    interval).  fp16 sub-normals step by 2^-24: an element whose second term h2 falls below 2^-14 carries an absolute error of up
    to 2^-25 in scaled units, which is 2^-25 / s <= 2^-25 B / 2^13 in the caller's.  A row whose max|.| is at least 2^-12 of B
    has its significant elements at >= 2 in scaled units, h2 >= 2^-11 |element| well inside the normal range for every element
    that matters at the 2^-22 level: such rows are "large" and get the REDUCED bound (the first two lines), i.e. the output is
    held to fp32 class per row.  Smaller rows get the full bound.
  * The fp32 kernel (pca_arith=fp32, or KD % 32 != 0) is held to the first line alone.

"Small" is decided on what the kernel splits: row m of A = X - mean against B, row j of W against Wm (without a mean that is
"row of X against the batch maximum").  Rows SCALED by 2^-12 have their own maximum a little below 2^-12 of the batch's (row
maxima of Gaussian rows differ by a factor < 2); the tests hold them to the reduced bound all the same (all_reduced=True): an
element of >= 2^-3 in scaled units loses at most 2^-25 <= 2^-22 of itself to a sub-normal second term, and the smaller
elements of such a row add up to a fraction of the second line.
"""
import numpy as np

SMALL_ROW = 2.0 ** -12      # rows below this fraction of the batch / model maximum get the sub-normal terms


def col_scale(var, whiten):
    """pca_scale_kernel: (float)(1 / sqrt((double)var[j])), or 1 without whitening."""
    if not whiten:
        return np.ones(len(var), np.float32)
    return (1.0 / np.sqrt(np.asarray(var, np.float32).astype(np.float64))).astype(np.float32)


class Ref:
    """ref [n, P] float64, e_np [n], bound [n, P] for one case (see the module docstring).  path: "x3" or "fp32"."""

    def __init__(self, X, mean, W, cs, path="x3", all_reduced=False, yardstick="row"):
        assert path in ("x3", "fp32") and yardstick in ("row", "col")
        X = np.ascontiguousarray(X, np.float32)
        W = np.ascontiguousarray(W, np.float32)
        cs = np.asarray(cs, np.float32)
        mean32 = np.zeros(X.shape[1], np.float32) if mean is None else np.asarray(mean, np.float32)
        assert np.isfinite(X).all() and np.isfinite(W).all() and np.isfinite(mean32).all() and np.isfinite(cs).all()
        A = X.astype(np.float64) - mean32.astype(np.float64)
        W64, cs64 = W.astype(np.float64), cs.astype(np.float64)
        self.ref = (A @ W64.T) * cs64
        y_np = ((X - mean32) @ W.T) * cs                                      # all-fp32 numpy product of the same operands
        assert y_np.dtype == np.float32
        e_all = np.abs(y_np.astype(np.float64) - self.ref)
        self.e_np = e_all.max(axis=1)
        self.e_np_col = e_all.max(axis=0)
        self.B = float(np.abs(X).max() + np.abs(mean32).max())
        self.Wm = float(np.abs(W).max())
        absA, absW = np.abs(A), np.abs(W64)
        self.small_x = absA.max(axis=1) < SMALL_ROW * self.B
        self.small_w = absW.max(axis=1) < SMALL_ROW * self.Wm
        if all_reduced:       # the caller holds every row to the reduced bound (never the other way round)
            self.small_x[:] = False
            self.small_w[:] = False
        # yardstick="col": numpy's worst error of the COLUMN instead of the row -- the same bound for the transposed product
        # (W^T is the "batch"), which is what holds a small row of W (a small output column) to its own magnitude
        bound = 4.0 * (self.e_np[:, None] if yardstick == "row" else self.e_np_col[None, :]) * np.ones_like(self.ref)
        if path == "x3":
            bound += 3.0 * 2.0 ** -22 * cs64 * (absA @ absW.T)
            sub_a = 2.0 ** -25 * (self.B / 2.0 ** 13) * cs64 * absW.sum(axis=1)            # [P]
            sub_w = 2.0 ** -25 * (self.Wm / 2.0 ** 13) * cs64[None, :] * absA.sum(axis=1)[:, None]   # [n, P]
            bound += np.where(self.small_x[:, None], sub_a[None, :], 0.0)
            bound += np.where(self.small_w[None, :], sub_w, 0.0)
        self.bound = bound
        self.row_ref_max = np.abs(self.ref).max(axis=1)

    def err(self, y):
        return np.abs(np.asarray(y).astype(np.float64) - self.ref)

    def worst(self, y):
        """max over entries of |err| / bound (an entry with bound 0 must have err 0)."""
        e = self.err(y)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(self.bound > 0, e / self.bound, np.where(e > 0, np.inf, 0.0))
        return float(q.max())

    def col_rel(self, y):
        """per column: max|err| / max|ref| of that column."""
        e, r = self.err(y).max(axis=0), np.abs(self.ref).max(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, e / r, np.where(e > 0, np.inf, 0.0))

    def row_rel(self, y):
        """per row: max|err| / max|ref| of that row."""
        e = self.err(y).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.row_ref_max > 0, e / self.row_ref_max, np.where(e > 0, np.inf, 0.0))

    def report(self, name, y):
        rr = self.row_rel(y)
        w = self.worst(y)
        print(f"[projection] {name}: max|err|/bound = {w:.3f}   worst row max|err|/max|ref| = {rr.max():.2e} (median {np.median(rr):.2e})")
        return w

    def check(self, name, y):
        """print the figures, then hold EVERY entry to its bound"""
        y = np.asarray(y)
        assert y.shape == self.ref.shape, (y.shape, self.ref.shape)
        w = self.report(name, y)
        bad = np.argwhere(~(self.err(y) <= self.bound))        # NaN fails too
        assert bad.size == 0, (name, "entries outside the bound:", len(bad), "first", bad[:5].tolist(), "worst err/bound", w)
        return w


# ------------------------------------------------------------------------------------------------
# host emulation of the split path (csrc/gemm_f16x3_kernels.hip), with the dispatch of launch_x3
# ------------------------------------------------------------------------------------------------
def x3_scale(maxabs):
    """the power of two s with maxabs * s in [2^13, 2^14) (api.hip: frexpf / ldexpf(1, 14 - e)); 1 for 0 / non-finite"""
    if not (maxabs > 0 and np.isfinite(maxabs)):
        return np.float32(1.0)
    _, e = np.frexp(np.float32(maxabs))
    return np.float32(np.ldexp(1.0, 14 - int(e)))


def x3_plan(M, N, Kd, tile=0):
    """(tile, k_per_split, splits) as launch_x3 chooses them"""
    bm = tile if tile else (256 if M >= 1024 else 128)
    tiles = -(-M // bm) * -(-N // bm)
    slots = 256 * (1 if bm == 256 else 2)
    best, splits = 1e30, 1
    for s in range(1, 33):
        rounds = (tiles * s + slots - 1) // slots
        cost = rounds / s + 0.004 * s * tiles / slots
        if cost < best - 1e-12:
            best, splits = cost, s
    kps = (-(-Kd // splits) + 31) // 32 * 32
    return bm, kps, -(-Kd // kps)


def split16(x32, scale):
    """split_f16x2_kernel: f = x * scale (fp32); h1 = fp16(f); h2 = fp16(f - h1)"""
    f = (np.asarray(x32, np.float32) * np.float32(scale)).astype(np.float32)
    h1 = f.astype(np.float16)
    h2 = (f - h1.astype(np.float32)).astype(np.float16)
    return h1.astype(np.float64), h2.astype(np.float64)


def emulate_x3(X, mean, W, cs, tile=0, drop=None, skip_last_block_of_slice=None, cs_twice=False):
    """The split projection on the host: fp16 rounding of f and f - h1, per 32-deep k-block the three products a2.b1, a1.b2,
    a1.b1 added to an fp32 accumulator (the block's 32 exact fp16 x fp16 products summed in float64 first), one accumulator per
    split-K slice, slices added in index order, then the scale.  The three keyword arguments each break it in one way:
    drop = "a2b1" | "a1b2" | "a1b1" leaves one product out, skip_last_block_of_slice = s skips the last k-block of slice s,
    cs_twice applies the column scale in the kernel epilogue AND in the reduction."""
    X = np.ascontiguousarray(X, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    cs = np.asarray(cs, np.float32)
    n, Kd = X.shape
    P = W.shape[0]
    assert Kd % 32 == 0
    mean32 = np.zeros(Kd, np.float32) if mean is None else np.asarray(mean, np.float32)
    sx = x3_scale(np.float32(np.abs(X).max()) + np.float32(np.abs(mean32).max()))
    sw = x3_scale(np.abs(W).max())
    a1, a2 = split16((X - mean32).astype(np.float32), sx)
    b1, b2 = split16(W, sw)
    _, kps, splits = x3_plan(n, P, Kd, tile)
    total = None
    for s in range(splits):
        kbeg, kend = s * kps, min(Kd, (s + 1) * kps)
        blocks = list(range(kbeg, kend, 32))
        if skip_last_block_of_slice == s:
            blocks = blocks[:-1]
        acc = np.zeros((n, P), np.float32)
        for k in blocks:
            sl = slice(k, k + 32)
            for name, (a, b) in (("a2b1", (a2, b1)), ("a1b2", (a1, b2)), ("a1b1", (a1, b1))):
                if name != drop:
                    acc = (acc.astype(np.float64) + a[:, sl] @ b[:, sl].T).astype(np.float32)
        total = acc if total is None else (total + acc).astype(np.float32)
    out_scale = np.float32(1.0) / (sx * sw)
    y = (total * (out_scale * cs)).astype(np.float32)
    if cs_twice:
        y = (y * cs).astype(np.float32)
    return y


# ------------------------------------------------------------------------------------------------
# the cases (shared by the device test and the CPU test of the bound)
# ------------------------------------------------------------------------------------------------
X3_SMALL_TILE = [(1, 32, 1), (5, 64, 7), (130, 1056, 129), (333, 2048, 200)]      # M < 1024: 128 x 128 tiles
X3_BIG_TILE = [(1024, 96, 256), (1025, 96, 257), (1300, 32, 300)]                 # M >= 1024: 256 x 256 tiles
DYN_SHAPE = (64, 2048, 48)
DYN_CASES = [("x", 12), ("x", 20), ("w", 12), ("w", 20)]                          # which operand's second half, scaled by 2^-e


def make_case(n, KD, P, whiten=True, with_mean=True, seed=None):
    """(X, mean or None, W, var, cs): a synth.make_pca_model model and seeded standard_normal / sqrt(KD) rows"""
    from revisit_anything_amd import synth

    seed = 7000 + (n * 31 + KD * 7 + P) % 1000 if seed is None else seed
    mean, W, var = synth.make_pca_model(KD, P, seed=seed)
    X = (np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((n, KD)) / np.sqrt(KD)).astype(np.float32)
    return X, (mean if with_mean else None), W, var, col_scale(var, whiten)


def make_dyn_case(side, e):
    """DYN_SHAPE without mean and whitening; the second half of the rows of X (side "x") or of W (side "w") scaled by 2^-e"""
    n, KD, P = DYN_SHAPE
    X, _, W, var, cs = make_case(n, KD, P, whiten=False, with_mean=False, seed=7700)
    X, W = X.copy(), W.copy()
    if side == "x":
        X[n // 2:] *= np.float32(2.0 ** -e)
    else:
        W[P // 2:] *= np.float32(2.0 ** -e)
    return X, None, W, var, cs
