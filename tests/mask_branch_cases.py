"""The mask branch's shape table: which tokens belong to which segment (segvlad_incidence, segvlad_incidence_centroids,
segvlad_mask_centroids) and which segments are pooled together (segvlad_adjacency, segvlad_adjacency_flagged) -- one case per
branch that sv_launch_incidence and sv_launch_adjacency (csrc/mask_kernels.hip) take from the shape alone.  A plain module (no
fixtures): tests/test_mask_branch_cases.py qualifies the table on the CPU with references only, tests/test_gpu_mask_branch.py runs
the kernels on it.  Every comparison made with this table is exact.

How the launchers decide (the facts `launch_facts` and `adjacency_facts` restate, and every case's `expect` quotes):
  sv_launch_incidence  dh = H // patch, dw = W // patch, N = dh dw, nw = ceil(N / 64); sh = fp32(Hm) / fp32(H), sw alike;
                       lds = Hm ceil(Wm / 32) 4 bytes of bitmap.
                       incidence_fused_kernel (one workgroup per mask, ceil(64 nw / 256) passes of 256 tokens) when Wm % 16 == 0,
                       the mask pointer is 16-byte aligned and lds <= 150 KiB; above 64 KiB the launch asks for the larger dynamic
                       block first.  Inside it `ranges = sh <= 1 and sw <= 1` picks the word-mask range test, else the pixel walk.
                       Otherwise incidence_kernel on a (S, ceil(nw / 4)) grid, and centroid_kernel when centroids are wanted.
  sv_launch_adjacency  S_max = the largest image, SW = ceil(S_max / 64) words per bit row,
                       lds = 16 S_max + 24 S_max SW + 16 (the coordinates, three bit matrices, the flag word; the kernel has no
                       static LDS), refused with SEGVLAD_ERR_LIMIT above 160 KiB (S_max = 639 is the last size that fits), the
                       larger dynamic block is asked for above 64 KiB (S_max >= 385); 1024 threads per image for B <= 64, else 256.

An incidence case is (S, Hm, Wm, H, W, patch): S blob masks with bytes in {1, 2, 128, 255}, FOLLOWED by the masks built for the
case (`build_masks` returns their rows by role):
  corner0..3   one pixel each: (0, 0), (0, Wm-1), (Hm-1, 0), (Hm-1, Wm-1)
  strip        only pixels whose every reader is a destination row >= dh patch or column >= dw patch (the ragged strip of the
               last token row / column) -- present when the image is ragged and such source pixels exist
  ones, zeros  every token set and the centroid ((Wm-1)/2, (Hm-1)/2); no token set and a NaN centroid
  unsampled    (sh > 1 or sw > 1) every pixel that nearest sampling never reads: no token set, the centroid that of the pixels
A case with `specials=False` (S = 1, S = 0) holds its blobs only.

An adjacency batch is a list of images (centroids [S_b, 2] fp64); `classify` puts each image into a class with the exact
empty-circle rule (`exact_delaunay`), and `adjacency_reference` gives what the kernel must write for it.
"""
import functools
import math
from fractions import Fraction

import numpy as np

KIB = 1024
ORDERS = (1, 2, 3, 6)
MARGIN = 100.0        # a generic image keeps |tmax - tmin| >= MARGIN (emin + emax) on every pair the kernel's flag looks at


# ---- incidence / centroid cases ---------------------------------------------------------------------------------------------
def _inc(name, shape, expect, specials=True, offset=0, seed=0):
    S, Hm, Wm, H, W, patch = shape
    return dict(name=name, S=S, Hm=Hm, Wm=Wm, H=H, W=W, patch=patch, expect=expect, specials=specials, offset=offset, seed=seed)


INCIDENCE_CASES = [
    # N = 9 * 10 = 90 tokens (nw = 2, 38 pad bits), W = 150 ragged by 10 columns; both axes up-sampled: the word-mask range test
    _inc("fused_ranges_small", (6, 64, 96, 126, 150, 14),
         dict(fused=True, why="fused", ranges=True, N=90, nw=2, ragged_w=10, ragged_h=0, lds=64 * 3 * 4, lds_class="le64k")),
    # 208 / 100 and 272 / 130 > 1: the pixel walk on both axes, and source rows / columns that no destination pixel reads
    _inc("fused_walk_down_down", (5, 208, 272, 100, 130, 14), dict(fused=True, ranges=False, scale=("down", "down"), wm_mod32=16)),
    _inc("fused_walk_up_down", (4, 48, 272, 100, 130, 14), dict(fused=True, ranges=False, scale=("up", "down"))),
    _inc("fused_walk_down_up", (4, 208, 80, 100, 130, 14), dict(fused=True, ranges=False, scale=("down", "up"), wm_mod32=16)),
    # the masks have the image's size: every source pixel is read exactly once; Wm = 112 = 3 * 32 + 16: the last bitmap word of a
    # row is half used; N = 4 * 8 = 32 < 64: one ballot word, half of it pad
    _inc("fused_scale_one", (4, 56, 112, 56, 112, 14), dict(fused=True, ranges=True, scale=("one", "one"), wm_mod32=16, N=32, nw=1)),
    # one 16-pixel chunk and one (half used) bitmap word per row; a single token row
    _inc("fused_wm16_dh1", (3, 16, 16, 14, 70, 14), dict(fused=True, wpr=1, cpr=1, dh=1, N=5, scale=("down", "up"), ranges=False)),
    _inc("fused_n64", (3, 64, 64, 112, 112, 14), dict(fused=True, N=64, nw=1, pad_bits=0, ranges=True)),
    # the bench's geometry: 34 * 45 = 1530 tokens, nw = 24 -> six passes of 256 tokens, the last one holding 250
    _inc("fused_n1530", (3, 240, 320, 480, 640, 14), dict(fused=True, N=1530, nw=24, passes=6, last_pass_tokens=250, ranges=True)),
    # the bitmap at the three sizes the launcher compares it with, and one step past the last
    _inc("fused_lds_64k", (2, 512, 1024, 224, 322, 14), dict(fused=True, lds=64 * KIB, lds_class="le64k", attr_call=False)),
    _inc("fused_lds_128k", (2, 1024, 1024, 224, 322, 14), dict(fused=True, lds=128 * KIB, lds_class="le150k", attr_call=True)),
    _inc("fused_lds_150k", (2, 1200, 1024, 224, 322, 14), dict(fused=True, lds=150 * KIB, lds_class="le150k", attr_call=True)),
    _inc("unfused_lds_152k", (2, 1216, 1024, 224, 322, 14), dict(fused=False, why="lds_over_150k", lds=152 * KIB, grid_y=2)),
    _inc("unfused_wm_up", (6, 50, 70, 126, 150, 14), dict(fused=False, why="wm_not_16", scale=("up", "up"), grid_y=1)),
    # N = 17 * 23 = 391 tokens, nw = 7: two workgroups per mask, the second with one idle wave
    _inc("unfused_wm_down_gridy2", (3, 250, 330, 238, 322, 14),
         dict(fused=False, why="wm_not_16", scale=("down", "down"), N=391, nw=7, grid_y=2)),
    # the first case's masks one byte into a device buffer: a contiguous view that the engine passes through as it is
    _inc("unfused_misaligned", (6, 64, 96, 126, 150, 14), dict(fused=False, why="misaligned", ranges=True), offset=1),
    _inc("patch16", (3, 48, 80, 100, 130, 16), dict(patch=16, N=48, ragged_h=4, ragged_w=2, fused=True)),
    _inc("patch8", (3, 64, 96, 57, 83, 8), dict(patch=8, N=70, ragged_h=1, ragged_w=3, fused=True, ranges=False)),
    _inc("s1", (1, 64, 96, 126, 150, 14), dict(S_total=1, fused=True), specials=False, seed=1),
    _inc("s0", (0, 64, 96, 126, 150, 14), dict(S_total=0), specials=False),
    # grid.x = 300 + the case's own masks
    _inc("s300", (300, 32, 48, 56, 84, 14), dict(S_blobs=300, fused=True, N=24)),
]
INC_BY_NAME = {c["name"]: c for c in INCIDENCE_CASES}
INC_NAMES = [c["name"] for c in INCIDENCE_CASES]

# every branch of sv_launch_incidence / the two kernels that the table must reach (tests/test_mask_branch_cases.py compares)
INCIDENCE_BRANCHES = {
    "fused", "unfused:wm_not_16", "unfused:misaligned", "unfused:lds_over_150k",
    "lds<64k", "lds==64k", "64k<lds<150k", "lds==150k", "lds>150k",
    "ranges", "walk:down,down", "walk:up,down", "walk:down,up", "scale:one,one", "unfused:up,up", "unfused:down,down",
    "wm%32==16", "wpr==1", "dh==1", "N<64", "N%64==0", "N%64!=0", "grid_y>1", "passes>1,last partial",
    "patch==8", "patch==16", "S==0", "S==1", "S>=300", "ragged_h", "ragged_w",
}


def nearest_src_index(out_size, in_size):
    from oracle import segvlad_oracle as O

    return O.nearest_src_index(out_size, in_size)


def _axis(scale):
    return "one" if scale == 1.0 else "up" if scale < 1.0 else "down"


def launch_facts(c):
    """What sv_launch_incidence and its kernels derive from the case's shape (and the pointer's alignment)."""
    Hm, Wm, H, W, patch = c["Hm"], c["Wm"], c["H"], c["W"], c["patch"]
    dh, dw = H // patch, W // patch
    N = dh * dw
    nw = (N + 63) // 64
    sh, sw = np.float32(Hm) / np.float32(H), np.float32(Wm) / np.float32(W)
    lds = Hm * ((Wm + 31) // 32) * 4
    aligned = c["offset"] % 16 == 0
    why = "wm_not_16" if Wm % 16 else "misaligned" if not aligned else "lds_over_150k" if lds > 150 * KIB else "fused"
    fused = why == "fused"
    passes = (nw * 64 + 255) // 256
    n_special = len(special_roles(c))
    return dict(fused=fused, why=why, lds=lds, lds_over_64k=lds > 64 * KIB, attr_call=fused and lds > 64 * KIB,
                lds_class="le64k" if lds <= 64 * KIB else "le150k" if lds <= 150 * KIB else "over150k",
                ranges=bool(sh <= 1 and sw <= 1), scale=(_axis(sh), _axis(sw)), dh=dh, dw=dw, N=N, nw=nw, pad_bits=nw * 64 - N,
                grid_y=(nw + 3) // 4, passes=passes, last_pass_tokens=N - 256 * (passes - 1), wpr=(Wm + 31) // 32, cpr=Wm // 16,
                wm_mod32=Wm % 32, patch=patch, ragged_h=H - dh * patch, ragged_w=W - dw * patch, S_blobs=c["S"],
                S_total=c["S"] + n_special)


def incidence_branches(c):
    """The names of INCIDENCE_BRANCHES that the case reaches"""
    f = launch_facts(c)
    b = set()
    if f["S_total"] == 0:
        return {"S==0"}          # (the launcher returns before it decides anything)
    b.add("fused" if f["fused"] else "unfused:" + f["why"])
    lds = f["lds"]
    b.add("lds<64k" if lds < 64 * KIB else "lds==64k" if lds == 64 * KIB else "64k<lds<150k" if lds < 150 * KIB else
          "lds==150k" if lds == 150 * KIB else "lds>150k")
    sc = ",".join(f["scale"])
    if f["fused"]:
        b.add("ranges" if f["ranges"] else "walk:" + sc)
        if sc == "one,one":
            b.add("scale:one,one")
        if f["wm_mod32"] == 16:
            b.add("wm%32==16")
        if f["wpr"] == 1:
            b.add("wpr==1")
        if f["passes"] > 1 and f["last_pass_tokens"] < 256:
            b.add("passes>1,last partial")
    else:
        b.add("unfused:" + sc)
        if f["grid_y"] > 1:
            b.add("grid_y>1")
    if f["dh"] == 1:
        b.add("dh==1")
    if f["N"] < 64:
        b.add("N<64")
    b.add("N%64==0" if f["N"] % 64 == 0 else "N%64!=0")
    if f["patch"] != 14:
        b.add("patch==%d" % f["patch"])
    if f["S_total"] == 1:
        b.add("S==1")
    if f["S_blobs"] >= 300:
        b.add("S>=300")
    if f["ragged_h"]:
        b.add("ragged_h")
    if f["ragged_w"]:
        b.add("ragged_w")
    return b


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


def _sampling(c):
    """Per axis: (source index of every destination pixel, the source indices read only from the ragged strip, the source
    indices never read)"""
    out = []
    for n_out, n_in, n_tok in ((c["H"], c["Hm"], c["H"] // c["patch"]), (c["W"], c["Wm"], c["W"] // c["patch"])):
        src = nearest_src_index(n_out, n_in)
        edge = n_tok * c["patch"]
        strip_only = np.setdiff1d(src[edge:], src[:edge])
        never = np.setdiff1d(np.arange(n_in), src)
        out.append((src, strip_only, never))
    return out


def special_roles(c):
    """The roles of the masks behind the case's blobs, in their order"""
    if not c["specials"]:
        return []
    (_, strip_r, never_r), (_, strip_c, never_c) = _sampling(c)
    roles = ["corner0", "corner1", "corner2", "corner3"]
    if len(strip_r) or len(strip_c):
        roles.append("strip")
    roles += ["ones", "zeros"]
    if len(never_r) or len(never_c):
        roles.append("unsampled")
    return roles


@functools.lru_cache(maxsize=None)
def build_masks(name):
    """(masks uint8 [S_total, Hm, Wm] -- never written to --, {role: row})"""
    from revisit_anything_amd import synth

    c = INC_BY_NAME[name]
    S, Hm, Wm = c["S"], c["Hm"], c["Wm"]
    seed = 9100 + 10 * c["seed"] + (0 if name == "unfused_misaligned" else INC_NAMES.index(name))
    rng = _rng(seed)
    roles = special_roles(c)
    m = np.zeros((S + len(roles), Hm, Wm), np.uint8)
    if S:
        blobs = synth.make_blob_masks(S, Hm, Wm, seed=seed + 1)
        m[:S] = blobs * rng.choice(np.array([1, 2, 128, 255], np.uint8), size=blobs.shape)
    (src_r, strip_r, never_r), (src_c, strip_c, never_c) = _sampling(c)
    where = {}
    for j, role in enumerate(roles):
        s = S + j
        where[role] = s
        if role.startswith("corner"):
            k = int(role[-1])
            m[s, (Hm - 1) * (k >> 1), (Wm - 1) * (k & 1)] = 255
        elif role == "strip":     # (rows read only from the strip) x (every column that is read), and the same transposed
            if len(strip_r):
                m[s][np.ix_(strip_r, np.unique(src_c))] = 1
            if len(strip_c):
                m[s][np.ix_(np.unique(src_r), strip_c)] = 1
        elif role == "ones":
            m[s] = 1
        elif role == "unsampled":
            m[s, never_r, :] = 3
            m[s, :, never_c] = 3
    m.setflags(write=False)
    return m, where


@functools.lru_cache(maxsize=None)
def incidence_reference(name):
    """(oracle.incidence bool [S_total, N], oracle.mask_centroids fp64 [S_total, 2] with NaN rows for empty masks)"""
    from oracle import segvlad_oracle as O

    c = INC_BY_NAME[name]
    m, _ = build_masks(name)
    N = (c["H"] // c["patch"]) * (c["W"] // c["patch"])
    if len(m) == 0:
        return np.zeros((0, N), bool), np.zeros((0, 2))
    inc = O.incidence(m, c["H"], c["W"], c["patch"])
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (the mean of an empty mask's coordinates: NaN, as in the reference)
            cent = O.mask_centroids(list(m))
    return inc, np.asarray(cent, np.float64).reshape(len(m), 2)


# ---- the exact Delaunay rule ------------------------------------------------------------------------------------------------
# For a pair (u, v) and every other point p:  a = p - u, b = p - v, e = v - u, num = a . b, den = e x a, tau = num / den.
# den > 0 bounds the circle parameter from above (tmin = min tau), den < 0 from below (tmax = max tau), den == 0 with num < 0 is a
# point inside the segment (blocked).  The edge exists iff not blocked and tmax <= tmin; tmax == tmin is an empty circle through four
# points.  Everything below is integer arithmetic on exact integer coordinates: fractions are compared by cross-multiplication.
def _exact_ints(c):
    """The fp64 coordinates as exact integers over one common power-of-two denominator (tau does not depend on the scale)"""
    fr = [[Fraction(float(x)) for x in row] for row in np.asarray(c, np.float64)]
    den = 1
    for row in fr:
        for f in row:
            den = max(den, f.denominator)
    return [[int(f * den) for f in row] for row in fr]


def _delaunay_python(P):
    """The rule on Python integers of any size: (A1, duplicate, rows (u, v, pmax, pmin, |tmax - tmin| as a Fraction) of the unblocked
    pairs with both bounds finite)"""
    S = len(P)
    A = np.eye(S, dtype=bool)
    dup = False
    both = []
    for u in range(S):
        ux, uy = P[u]
        for v in range(u + 1, S):
            vx, vy = P[v]
            ex, ey = vx - ux, vy - uy
            if ex == 0 and ey == 0:
                dup = True
            lo = hi = None      # hi = tmin as (num, den > 0, p), lo = tmax as (num, den < 0, p)
            blocked = False
            for p in range(S):
                if p == u or p == v:
                    continue
                ax, ay = P[p][0] - ux, P[p][1] - uy
                bx, by = P[p][0] - vx, P[p][1] - vy
                n, d = ax * bx + ay * by, ex * ay - ey * ax
                if d > 0:
                    if hi is None or n * hi[1] < hi[0] * d:      # n / d < hi: both dens positive
                        hi = (n, d, p)
                elif d < 0:
                    if lo is None or n * lo[1] > lo[0] * d:      # n / d > lo: both dens negative, their product positive
                        lo = (n, d, p)
                elif n < 0:
                    blocked = True
            if blocked:
                continue
            if lo is None or hi is None or lo[0] * hi[1] >= hi[0] * lo[1]:      # tmax <= tmin, times dmax dmin < 0
                A[u, v] = A[v, u] = True
            if lo is not None and hi is not None:
                both.append((u, v, lo[2], hi[2], abs(Fraction(lo[0], lo[1]) - Fraction(hi[0], hi[1]))))
    U, V, PL, PH = (np.array([r[k] for r in both], np.int64) for k in range(4))
    zero = np.array([r[4] == 0 for r in both], bool)
    return A, dup, U, V, PL, PH, np.array([float(r[4]) for r in both], np.float64), zero


def _delaunay_int64(P):
    """The same on an int64 array [S, 2] with |coordinates| < 2^13 (every product below stays under 2^56), vectorised over (v, p)"""
    P = np.asarray(P, np.int64)
    S = len(P)
    assert np.abs(P).max() < 2 ** 13
    A = np.eye(S, dtype=bool)
    dup = False
    cols = [[] for _ in range(6)]
    idx = np.arange(S)
    for u in range(S - 1):
        vs = idx[u + 1:]
        a = P - P[u]                                  # [p]
        e = P[vs] - P[u]                              # [v]
        dup = dup or bool(((e[:, 0] == 0) & (e[:, 1] == 0)).any())
        bx, by = a[None, :, 0] - e[:, None, 0], a[None, :, 1] - e[:, None, 1]
        num = a[None, :, 0] * bx + a[None, :, 1] * by
        den = e[:, None, 0] * a[None, :, 1] - e[:, None, 1] * a[None, :, 0]
        other = (idx[None, :] != u) & (idx[None, :] != vs[:, None])
        blocked = ((den == 0) & (num < 0) & other).any(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        rows = np.arange(len(vs))
        pick = []
        for side, sign in ((den > 0, 1.0), (den < 0, -1.0)):      # tmin: the least tau; tmax: the greatest = the least of -tau
            side = side & other
            has = side.any(1)
            j = np.where(side, sign * t, np.inf).argmin(1)
            while True:        # fp64 only proposes: whether p beats j is decided exactly
                nj, dj = num[rows, j][:, None], den[rows, j][:, None]
                # the dens of one side share a sign, so den_p den_j > 0 and num_p den_j - num_j den_p has the sign of tau_p - tau_j
                diff = num * dj - nj * den
                better = side & ((diff < 0) if sign > 0 else (diff > 0)) & has[:, None]
                if not better.any():
                    break
                j = np.where(better.any(1), np.where(better, sign * t, np.inf).argmin(1), j)
            pick.append((has, j))
        (has_hi, jh), (has_lo, jl) = pick
        nh, dh_, nl, dl = num[rows, jh], den[rows, jh], num[rows, jl], den[rows, jl]
        fin = has_hi & has_lo
        cross = nl * dh_ - nh * dl                    # (tmax - tmin) dmax dmin, dmax dmin < 0
        edge = ~blocked & (~fin | (cross >= 0))
        A[u, vs[edge]] = True
        A[vs[edge], u] = True
        k = fin & ~blocked
        for col, val in zip(cols, (np.full(k.sum(), u), vs[k], jl[k], jh[k], np.abs(cross[k]), np.abs(dl[k] * dh_[k]))):
            col.append(val)
    U, V, PL, PH, G, D = (np.concatenate(col) if col else np.zeros(0, np.int64) for col in cols)
    return A, dup, U, V, PL, PH, G.astype(np.float64) / np.maximum(D, 1).astype(np.float64), G == 0


def _kernel_err(c, U, V, Pp):
    """adjacency_kernel's rounding bound `err` of tau_p for the pairs (u, v), from its formula (plain fp64 products where the kernel
    fuses two of them: the bound moves by a rounding of itself)"""
    ux, uy, vx, vy, qx, qy = c[U, 0], c[U, 1], c[V, 0], c[V, 1], c[Pp, 0], c[Pp, 1]
    ex, ey = vx - ux, vy - uy
    ax, ay, bx, by = qx - ux, qy - uy, qx - vx, qy - vy
    den = ex * ay - ey * ax
    t = (ax * bx + ay * by) / den
    return 9e-16 * ((np.abs(ax * bx) + np.abs(ay * by)) + np.abs(t) * (np.abs(ex * ay) + np.abs(ey * ax))) / np.abs(den)


def exact_delaunay(c, force_python=False):
    """dict(A1 bool [S, S] with the diagonal, duplicate, cocircular: an unblocked pair with tmax == tmin exactly,
    margin: the least |tmax - tmin| / (emin + emax) over the unblocked pairs with both bounds finite and tmax != tmin -- inf
    without one) for S > 3 points without NaN"""
    c = np.asarray(c, np.float64)
    ints = _exact_ints(c)
    if not force_python and max(abs(x) for row in ints for x in row) < 2 ** 13:
        A, dup, U, V, PL, PH, gap, zero = _delaunay_int64(np.array(ints, np.int64))
    else:
        assert len(c) <= 64, "the Python-integer form is for small images"
        A, dup, U, V, PL, PH, gap, zero = _delaunay_python(ints)
    margin = math.inf
    if (~zero).any():
        k = ~zero
        margin = float((gap[k] / (_kernel_err(c, U[k], V[k], PL[k]) + _kernel_err(c, U[k], V[k], PH[k]))).min())
    return dict(A1=A, duplicate=dup, cocircular=bool(zero.any()), margin=margin)


def small_image_block(S):
    """S <= 3 (func_vpr.py:1339-1344): every row = e0 (+ e1), whatever the order"""
    A = np.zeros((S, S), bool)
    A[:, :min(S, 2)] = True
    return A


def closure(A1, order):
    """(A1 ^ order) > 0: order - 1 rounds of P <- (P A1) > 0 on integer matrices (a product's entries are counts <= S)"""
    A = A1.astype(np.int64)
    P = A.copy()
    for _ in range(order - 1):
        P = ((P.astype(np.float64) @ A.astype(np.float64)) > 0).astype(np.int64) if len(A) > 200 else ((P @ A) > 0).astype(np.int64)
    return P > 0


def classify(c):
    """('empty' | 'small' | 'nan' | 'generic' | 'degenerate' | 'unclassified', margin, exact dict or None).  'small' (S <= 3) images
    are not triangulated at all; 'unclassified' = no exact degeneracy, yet a pair whose |tmax - tmin| is within MARGIN times the
    kernel's rounding bound: what the kernel's flag says there is a matter of rounding, and the table must not hold such an image."""
    c = np.asarray(c, np.float64).reshape(-1, 2)
    if len(c) == 0:
        return "empty", math.inf, None
    if np.isnan(c).any():
        return "nan", math.nan, None
    if len(c) <= 3:
        return "small", math.inf, None
    ex = exact_delaunay(c)
    if ex["duplicate"] or ex["cocircular"]:
        return "degenerate", ex["margin"], ex
    return ("generic" if ex["margin"] >= MARGIN else "unclassified"), ex["margin"], ex


# ---- adjacency batches ------------------------------------------------------------------------------------------------------
def _dyadic_points(rng, S, span=512, step=16):
    """S distinct points k / step in [0, span)^2: fp64 holds them exactly, and step * span = 2^13 keeps the exact rule in int64"""
    seen, pts = set(), []
    while len(pts) < S:
        k = tuple(int(x) for x in rng.integers(0, span * step, size=2))
        if k not in seen:
            seen.add(k)
            pts.append((k[0] / step, k[1] / step))
    return np.array(pts, np.float64).reshape(S, 2)


def _int_points(rng, S, span=4096):
    seen, pts = set(), []
    while len(pts) < S:
        k = tuple(int(x) for x in rng.integers(0, span, size=2))
        if k not in seen:
            seen.add(k)
            pts.append(k)
    return np.array(pts, np.float64).reshape(S, 2)


LADDER = (0, 1, 2, 3, 4, 5, 0, 63, 64, 65, 3, 128, 129)
S_LDS_ATTR = 385            # the first S_max whose LDS block exceeds 64 KiB
S_LIMIT = 639               # the largest S_max that sv_launch_adjacency accepts; S_LIMIT + 1 is refused
GENERIC5 = np.array([[3.0, 4.0], [40.5, 7.25], [21.0, 33.0], [8.0, 29.5], [30.0, 18.0]])
RECT = np.array([[10.0, 10.0], [30.0, 10.0], [30.0, 22.0], [10.0, 22.0], [55.0, 60.0]])      # a lattice rectangle + one far point
# the rectangle (0,0) (50,0) (50,25) (0,25) turned by atan(3/4) -- an irrational angle whose sine and cosine are 3/5 and 4/5, so the
# turned corners are integers and exactly co-circular while no side is parallel to an axis
RECT_TURNED = np.array([[20.0, 10.0], [60.0, 40.0], [45.0, 60.0], [5.0, 30.0], [90.0, 95.0]])
DUPLICATE = np.array([[5.0, 5.0], [25.0, 6.0], [25.0, 6.0], [9.0, 31.0], [40.0, 28.0]])
# x^2 + y^2 = 25^2 through five lattice points (+ the centre (40, 40))
CIRCLE5 = np.array([[65.0, 40.0], [60.0, 55.0], [47.0, 64.0], [25.0, 60.0], [33.0, 16.0]])
LATTICE3 = np.array([[x, y] for y in (2.0, 9.0, 16.0) for x in (3.0, 10.0, 17.0)])
# (2, 3) (12, 8) (22, 13) on one line: the middle one blocks the outer pair, no four points share an empty circle
COLLINEAR = np.array([[2.0, 3.0], [12.0, 8.0], [22.0, 13.0], [7.0, 21.0], [19.0, 1.5]])
DEGENERATE_IMAGES = {"rect": RECT, "rect_turned": RECT_TURNED, "duplicate": DUPLICATE, "circle5": CIRCLE5, "lattice3": LATTICE3}


def _batch(name, images, expect, orders=ORDERS):
    return dict(name=name, images=[np.asarray(i, np.float64).reshape(-1, 2) for i in images], expect=expect, orders=orders)


@functools.lru_cache(maxsize=None)
def adjacency_batches():
    """{name: batch}; a batch's images are never written to"""
    out = []
    rng = _rng(4100)
    out.append(_batch("ladder", [_dyadic_points(rng, S) for S in LADDER],
                      dict(S_max=129, SW=3, threads=1024, B=13, lds_over_64k=False, mixed=True)))
    # centroids of the s300 case's blob masks: means of integer pixel coordinates
    cent = incidence_reference("s300")[1]
    out.append(_batch("mask_centroids", [cent[:30], cent[30:80]], dict(S_max=50, SW=1, threads=1024)))
    rng = _rng(4200)
    many = [_dyadic_points(rng, int(S)) for S in _rng(4201).integers(4, 41, size=65)]
    out.append(_batch("b65", many, dict(B=65, threads=256, SW=1)))
    out.append(_batch("b64", many[:64], dict(B=64, threads=1024, SW=1)))
    # 184 S_max > 64 KiB from S_max = 357 on -- with SW = 7, which needs S_max >= 385: at 357 (SW = 6, 57136 B) the launch still takes
    # the default block, 385 (70856 B) is the first size that asks for the larger one
    out.append(_batch("s357", [_dyadic_points(_rng(4300), 357)], dict(S_max=357, SW=6, lds=57136, lds_over_64k=False, threads=1024)))
    out.append(_batch("s385", [_dyadic_points(_rng(4301), S_LDS_ATTR)], dict(S_max=385, SW=7, lds=70856, lds_over_64k=True)))
    out.append(_batch("s_limit", [_int_points(_rng(4400), S_LIMIT)],
                      dict(S_max=S_LIMIT, SW=10, lds=163600, lds_over_64k=True, fits=True)))
    g = [GENERIC5 + 1.5 * k for k in range(len(DEGENERATE_IMAGES) + 2)]
    imgs = [g[0]]
    for k, d in enumerate(DEGENERATE_IMAGES.values()):
        imgs += [d, g[k + 1]]
    imgs += [COLLINEAR, g[-1]]
    out.append(_batch("degenerate", imgs, dict(B=13, threads=1024, SW=1)))
    nan = GENERIC5 + 2.0
    nan[2] = np.nan
    out.append(_batch("nan", [GENERIC5, nan, GENERIC5 + 0.5], dict(B=3, SW=1)))
    out.append(_batch("order6", [_dyadic_points(_rng(4500), 20), GENERIC5], dict(S_max=20, SW=1), orders=(6,)))
    for b in out:
        for i in b["images"]:
            i.setflags(write=False)
    return {b["name"]: b for b in out}


ADJ_NAMES = ["ladder", "mask_centroids", "b65", "b64", "s357", "s385", "s_limit", "degenerate", "nan", "order6"]
DEGENERATE_AT = {1: "rect", 3: "rect_turned", 5: "duplicate", 7: "circle5", 9: "lattice3"}       # image -> name, batch "degenerate"
ADJACENCY_BRANCHES = {"SW==1", "SW>1", "threads==1024", "threads==256", "lds>64k", "lds<=64k", "largest accepted", "order>3",
                      "S<=3 and S==0 and S>64 under one S_max", "degenerate", "nan"}


def adjacency_lds(S_max):
    """sv_adjacency_lds: every byte of LDS of adjacency_kernel (it has no static LDS)"""
    return 16 * S_max + 24 * S_max * ((S_max + 63) // 64) + 16


def adjacency_facts(batch):
    sizes = [len(i) for i in batch["images"]]
    S_max, B = max(sizes), len(sizes)
    lds = adjacency_lds(S_max)
    return dict(S_max=S_max, SW=(S_max + 63) // 64, lds=lds, lds_over_64k=lds > 64 * KIB, fits=lds <= 160 * KIB, B=B,
                threads=1024 if B <= 64 else 256,
                mixed=0 in sizes and any(0 < s <= 3 for s in sizes) and any(s > 64 for s in sizes))


def adjacency_branches(batch):
    f = adjacency_facts(batch)
    b = {"SW==1" if f["SW"] == 1 else "SW>1", "threads==%d" % f["threads"], "lds>64k" if f["lds_over_64k"] else "lds<=64k"}
    if f["fits"] and adjacency_lds(f["S_max"] + 1) > 160 * KIB:
        b.add("largest accepted")
    if max(batch["orders"]) > 3:
        b.add("order>3")
    if f["mixed"]:
        b.add("S<=3 and S==0 and S>64 under one S_max")
    classes = [cl for cl, _, _ in batch_classes(batch["name"])] if "name" in batch else []
    b |= {cl for cl in classes if cl in ("degenerate", "nan")}
    return b


def pack_centroids(images):
    """(centroids [S_tot, 2] fp64, seg_offsets int32 [B + 1], where each image's block starts in the adjacency buffer)"""
    sizes = np.array([len(i) for i in images], np.int64)
    cat = np.concatenate([np.asarray(i, np.float64).reshape(-1, 2) for i in images]) if len(images) else np.zeros((0, 2))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    blocks = np.concatenate([[0], np.cumsum(sizes * sizes)])
    return np.ascontiguousarray(cat), offs, blocks


@functools.lru_cache(maxsize=None)
def batch_classes(name):
    """[(class, margin, exact dict or None)] per image, computed once"""
    return [classify(i) for i in adjacency_batches()[name]["images"]]


@functools.lru_cache(maxsize=None)
def adjacency_reference(name, order):
    """Per image: the block the kernel must write (bool [S, S]), None for an image with a NaN centroid.  The table's degenerate
    images have integer coordinates below 128: every product, sum and comparison of the kernel is then exact (two different taus
    with denominators below 2^14 differ by far more than a rounding of their quotients), so it must write the exact rule's block
    with every tie kept -- both diagonals of four points on an empty circle, a link between two duplicates (tmax <= tmin)."""
    out = []
    for img, (cl, _, ex) in zip(adjacency_batches()[name]["images"], batch_classes(name)):
        if cl in ("empty", "small"):
            out.append(small_image_block(len(img)))
        elif cl in ("generic", "degenerate"):
            out.append(closure(ex["A1"], order))
        else:
            out.append(None)
    return out
