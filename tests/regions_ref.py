"""Small-region removal restated in NumPy + scipy, and the masks the tests run it on.

`clean(mask, min_area)` is the contract of segvlad_mask_regions (include/segvlad.h) for one mask: remove_small_regions in mode
"holes" and then in mode "islands" (sam/segment_anything/utils/amg.py:267-291), 8-connected, strictly `< min_area`, keep-largest
with the tie going to the component whose FIRST PIXEL in row-major order comes first -- stated here through the first pixels
themselves, not through a labeller's numbering.  tests/test_regions_host.py holds it to the reference's own function on
tests/golden/regions_cases.npz; tests/test_gpu_regions.py holds the kernels to it over the table below."""
import functools

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=np.uint8)
SHAPES = [(1, 1), (1, 130), (130, 1), (33, 65), (64, 64), (97, 131), (200, 300)]
PLANTED = 6          # a 3 x 2 block planted in the "planted" masks
HOLE = 16            # the 4 x 4 hole of the square ring


def components(working: np.ndarray):
    """(labels int [H, W] with 0 = outside, sizes [n], first pixel (row-major index) [n]) of the 8-connected components"""
    lab, n = ndimage.label(working, structure=EIGHT)
    flat = lab.ravel()
    sizes = np.bincount(flat, minlength=n + 1)[1:]
    _, first = np.unique(flat, return_index=True)
    first = first[1:] if (flat == 0).any() else first
    assert len(first) == n
    return lab, sizes, first


def fill_holes(mask: np.ndarray, min_area: int):
    lab, sizes, _ = components(~mask)
    small = np.nonzero(sizes < min_area)[0] + 1
    if len(small) == 0:
        return mask, False
    return mask | np.isin(lab, small), True


def strip_islands(mask: np.ndarray, min_area: int):
    lab, sizes, first = components(mask)
    if not (sizes < min_area).any():
        return mask, False
    keep = np.nonzero(sizes >= min_area)[0] + 1
    if len(keep) == 0:
        best = np.nonzero(sizes == sizes.max())[0]
        keep = np.array([best[np.argmin(first[best])] + 1])   # the tie: the earliest first pixel
    return np.isin(lab, keep), True


def box_of(mask: np.ndarray):
    ys, xs = np.nonzero(mask)
    return [0, 0, 0, 0] if len(ys) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def clean(mask: np.ndarray, min_area: int):
    """one mask (non-zero = set) -> (uint8 0 / 1 [H, W], changed bits, XYXY box, area)"""
    m = np.asarray(mask) != 0
    m, c0 = fill_holes(m, min_area)
    m, c1 = strip_islands(m, min_area)
    return m.astype(np.uint8), int(c0) | (int(c1) << 1), box_of(m), int(m.sum())


def clean_batch(masks: np.ndarray, min_area: int):
    """[S, H, W] -> (uint8 [S, H, W], changed int32 [S], boxes int32 [S, 4], area int64 [S])"""
    r = [clean(m, min_area) for m in masks]
    S = len(r)
    return (np.stack([x[0] for x in r]) if S else np.zeros(np.shape(masks), np.uint8), np.array([x[1] for x in r], dtype=np.int32),
            np.array([x[2] for x in r], dtype=np.int32).reshape(S, 4), np.array([x[3] for x in r], dtype=np.int64))


# ---- the masks -------------------------------------------------------------------------------------------------------------------
def _corner_pairs(H, W, T, anti):
    """two pixels touching only at a corner, on every corner of the tiles of T: (T-1, T-1), (T, T) or (T-1, T), (T, T-1)"""
    m = np.zeros((H, W), np.uint8)
    for y in range(T, H, T):
        for x in range(T, W, T):
            if anti:
                m[y - 1, x] = m[y, x - 1] = 1
            else:
                m[y - 1, x - 1] = m[y, x] = 1
    return m


def _serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def _paint(m, y0, y1, x0, x1, v):
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = v


def patterns(H: int, W: int):
    """[(name, uint8 [H, W])]: the same list at every shape (what does not fit is clipped by the slicing)"""
    P = H * W
    out = []
    z = lambda: np.zeros((H, W), np.uint8)   # noqa: E731
    out.append(("zero", z()))
    out.append(("ones", np.ones((H, W), np.uint8)))
    m = z(); m[H // 2, W // 2] = 1
    out.append(("single_pixel", m))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checkerboard", ((yy + xx) % 2).astype(np.uint8)))
    m = z(); i = np.arange(min(H, W)); m[i, i] = 1
    out.append(("diagonal", m))
    m = z(); m[i, W - 1 - i] = 1
    out.append(("anti_diagonal", m))
    m = z(); i = np.arange(H); m[i, (i * 3) % W] = 1                    # a scatter of lone pixels
    out.append(("scatter", m))
    for T in (16, 32, 64):
        out.append((f"corners_{T}", _corner_pairs(H, W, T, False)))
        out.append((f"corners_{T}_anti", _corner_pairs(H, W, T, True)))
    s = _serpentine(H, W)
    out.append(("serpentine", s))
    out.append(("serpentine_complement", (1 - s).astype(np.uint8)))
    out.append(("serpentine_columns", _serpentine(W, H).T.copy()))
    # a one-pixel diamond ring: its inside leaks out through the diagonals -- not a hole
    cy, cx, r = H // 2, W // 2, max(2, min(H, W) // 3)
    out.append(("diamond_ring", (np.abs(yy - cy) + np.abs(xx - cx) == r).astype(np.uint8)))
    # a square ring around a 4 x 4 hole
    m = z(); _paint(m, 2, 10, 3, 11, 1); _paint(m, 4, 8, 5, 9, 0)
    out.append(("square_ring", m))
    # island inside hole inside island
    m = z(); _paint(m, 1, 22, 1, 24, 1); _paint(m, 4, 19, 4, 21, 0); _paint(m, 8, 12, 9, 13, 1)
    out.append(("nested", m))
    # a hole that touches the image border (closed by it), and a mask whose outer background is small
    m = z(); _paint(m, 0, 9, 2, 14, 1); _paint(m, 0, 3, 6, 9, 0)
    out.append(("hole_at_border", m))
    m = np.ones((H, W), np.uint8); _paint(m, 0, 2, 0, 2, 0)
    out.append(("small_background", m))
    m = np.ones((H, W), np.uint8); _paint(m, 0, 2, 0, 2, 0); _paint(m, H - 1, H, W - 3, W, 0); m[H // 2, W // 2] = 0
    out.append(("small_backgrounds", m))
    # every island small: with a tie for the largest (3, 3, 2 -- the later 3 is drawn first in the array's columns), without (2, 3, 4)
    m = z(); _paint(m, 0, 1, 6, 9, 1); _paint(m, 3, 6, 0, 1, 1); _paint(m, 8, 9, 8, 10, 1)
    out.append(("small_islands_tie", m))
    m = z(); _paint(m, 0, 1, 0, 2, 1); _paint(m, 3, 4, 0, 3, 1); _paint(m, 6, 8, 4, 6, 1)
    out.append(("small_islands", m))
    m = z(); _paint(m, 5, 7, 5, 7, 1)
    out.append(("one_small_island", m))
    # a planted block of PLANTED pixels next to a large one
    m = z(); _paint(m, 0, 3, 0, 2, 1); _paint(m, 6, H, 5, W, 1)
    out.append(("planted", m))
    for k, d in enumerate((0.3, 0.5, 0.7)):
        rng = np.random.Generator(np.random.PCG64([4242, H, W, k]))
        out.append((f"random_{d}", (rng.random((H, W)) < d).astype(np.uint8)))
    rng = np.random.Generator(np.random.PCG64([4243, H, W]))
    out.append(("other_bytes", rng.choice(np.array([0, 0, 0, 2, 128, 255], np.uint8), size=(H, W))))
    rng = np.random.Generator(np.random.PCG64([4244, H, W]))               # blobs: what SAM's masks look like
    blob = ndimage.uniform_filter(rng.random((H, W)), size=7, mode="constant") > 0.5
    out.append(("blobs", blob.astype(np.uint8)))
    assert all(m.shape == (H, W) and m.dtype == np.uint8 for _, m in out)
    assert P == H * W
    return out


def min_areas(H: int, W: int):
    """1, 2, a planted component's size and that + 1 (the planted block, the square ring's hole), a value above P"""
    return [1, 2, 3, PLANTED, PLANTED + 1, HOLE, HOLE + 1, H * W + 1]


@functools.lru_cache(maxsize=None)
def table(H: int, W: int):
    """(names, masks uint8 [S, H, W]) of a shape; computed once"""
    p = patterns(H, W)
    return [n for n, _ in p], np.stack([m for _, m in p])


@functools.lru_cache(maxsize=None)
def expected(H: int, W: int, min_area: int):
    """clean_batch of the shape's table; computed once and shared -- treat as read-only"""
    return clean_batch(table(H, W)[1], min_area)


def isolation_batch():
    """At least 8 different masks of 40 x 70, an empty and a full one among them; mask 2's last row lies directly "above" mask 3's
    first row in memory: a leak across masks would join them"""
    H, W = 40, 70
    names, t = table(H, W)
    pick = ["zero", "ones", "blobs", "random_0.5", "nested", "checkerboard", "serpentine", "small_islands_tie", "square_ring", "corners_32"]
    b = np.stack([t[names.index(n)] for n in pick]).copy()
    b[2, H - 1, 10:20] = 1
    b[3, 0, 10:20] = 1
    b[3, 1:3, :] = 0          # so that the row of mask 3 is a small island of its own
    return b
