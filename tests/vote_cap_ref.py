"""Plain reference of the vote's per-image cap (SEGVLAD_VOTE_PER_IMAGE, include/segvlad.h) and the inputs that the cap's tests share.
NumPy and python only, written to be read; it never calls product code.

The cap is defined by equivalence: the capped vote over `matches` is the plain vote (tests/search_tail_ref.py) over
blank(matches, img_of_seg, m)."""
import functools

import numpy as np

import search_tail_ref as R


def blank(matches, img_of_seg, m):
    """A copy of matches [nq][k] in which every valid entry (0 <= id < n_ref) that has m earlier valid entries of its row on the same
    image is -1.  Image ids compare as 32-bit values.  Invalid entries stay what they are: the vote skips them anyway."""
    matches = np.asarray(matches, np.int64)
    img = np.asarray(img_of_seg).astype(np.int32)
    out = matches.copy()
    for q in range(matches.shape[0]):
        seen = {}
        for r in range(matches.shape[1]):
            i = int(matches[q, r])
            if i < 0 or i >= len(img):
                continue
            g = int(img[i])
            if seen.get(g, 0) >= m:
                out[q, r] = -1
            else:
                seen[g] = seen.get(g, 0) + 1
    return out


# the shapes of the GPU parity test: one per launch regime of the vote, and the benchmark's depth
SHAPES = list(R.REGIME_SHAPES) + ["bench_depth_50x200"]
CAPS = [1, 2]


@functools.lru_cache(maxsize=None)
def case(name, invalid):
    c = R.vote_case(name)
    return R.with_invalid_ids(c) if invalid else c


@functools.lru_cache(maxsize=None)
def blanked(name, invalid, m):
    c = case(name, invalid)
    return blank(c["matches"], c["img_of_seg"], m)


@functools.lru_cache(maxsize=None)
def chunk_case(segs, k):
    """One query image of `segs` segments at depth k beside a 3-segment image, concentrated ids: the chunk edges of the cap's kernel
    (64 ranks per step; 1024 ranks of a row kept on chip)."""
    rng = np.random.default_rng(1000 * segs + k)
    im = R.ref_map()
    counts = [segs, 3]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    matches, _ = R._concentrated(rng, off, k, im)
    sims = np.sort(rng.uniform(0.2, 1.9, size=matches.shape).astype(np.float32), axis=1)[:, ::-1].copy()
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)


# (segments, k): one rank past a chunk, the last rank kept on chip, and a row that goes on behind it
CHUNK_SHAPES = [(3, 65), (5, 1024), (2, 1100)]


def blanked_share(c, m):
    """Share of the valid entries that blank() removes."""
    valid = (c["matches"] >= 0) & (c["matches"] < len(c["img_of_seg"]))
    b = blank(c["matches"], c["img_of_seg"], m)
    return float(((b != c["matches"]) & valid).sum()) / float(valid.sum())


@functools.lru_cache(maxsize=None)
def revisit_index(n_places=40, visits=4, segs=3, d=64, seed=11):
    """A small planted index with revisits: reference image p shows place p and stores it `visits` times -- `visits` noisy copies of
    each of the place's `segs` rows, all under image id p -- so a query segment of the place finds several rows of ONE image.  The
    queries are the first places' rows with noise of their own.  Returns (rows [n][d], img_of_seg [n], queries [nq][d],
    qseg_offsets) -- unit rows, fp32, the index rows shuffled."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n_places, segs, d)).astype(np.float32)

    def unit(x):
        return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)

    rows = np.concatenate([unit(base + 0.05 * rng.standard_normal(base.shape).astype(np.float32)).reshape(-1, d) for _ in range(visits)])
    img = np.tile(np.repeat(np.arange(n_places, dtype=np.int32), segs), visits)
    perm = rng.permutation(len(rows))
    n_q = 6
    q = unit(base[:n_q] + 0.05 * rng.standard_normal(base[:n_q].shape).astype(np.float32)).reshape(-1, d)
    off = (np.arange(n_q + 1) * segs).astype(np.int32)
    return rows[perm].copy(), img[perm].copy(), q, off
