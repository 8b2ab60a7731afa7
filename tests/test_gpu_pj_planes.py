"""Option pj_planes (fused segment-VLAD -> PCA, "project" form): the grouped projection GEMM stores every element of Z as the fp16
pair of z * zscale (h | l << 16 where the fp32 z stood) and the P-space aggregation feeds those words to its MFMAs from registers,
three tiles in flight, instead of staging fp32 tiles in LDS and splitting every element again.  Same operands in the same order:
pj_planes = 1 must give the BITS of pj_planes = 0, with cover_rows 0 and 1, and -- so that both cannot be wrong alike -- the fp64
oracle's values within 3e-5 of max |reference| (the bound tests/test_gpu_cover_rows.py holds this form to).

Calls go through the C ABI (segvlad_images_pca) with pca_path=project forced.  The labels are chosen, not drawn: a token is its
centre plus a little noise, and the case asserts that the oracle assigns it there.  What the cases cover:
  grid      B in {1, 3} x D in {32, 96} x P in {4, 36, 260} (fewer columns than a wave's 32 | a partial 256-column block | a second
            column block) x K in {1, 3, 5} (K > 1: one cluster that no token takes); clusters of one image of 33 / 32 / 17 / 16 / 1
            positions in rotation; one cluster of image 0 that no segment covers (a tile of zero rows, nothing loaded); an image
            without a segment where B = 3; S_b from {1, 3, 33, 65} (the small cases, both 32-segment halves, a second 64-segment chunk)
  sizes     K = 6: one image with clusters of 0, 1, 16, 17, 32 and 33 positions (the last is two tiles)
  tiles     images of 1, 2, 3 and 4 tiles in all (three register sets / fragment slots: fill, steady state, drain).  An image of
            no tile does not exist: tiles are made of positions and every image has N of them; the image without a segment is the
            case in which a workgroup has nothing to do
  zscale0   a centre whose norm overflows fp32 switches the 16-bit form off (zscale = 0): pj_planes must change nothing and the
            result is the fp32-MFMA form's (pj_f16 = 0).  No oracle here: a centre of that size takes the fp16 planes' whole range
  twice     two batches with other labels and masks alternate in one context (stale words of Z, of the zero row, of the tables)"""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_GRID = 99
S_POOL = (1, 3, 33, 65)
GRID = [(B, D, P, K) for B, D, P, K in itertools.product((1, 3), (32, 96), (4, 36, 260), (1, 3, 5))]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _tokens(C, labels, seed):
    """[D][N] unit columns: centre of the wanted cluster + noise well inside the gap to the next centre."""
    r = np.random.default_rng(seed)
    x = C[labels].astype(np.float64)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) + 0.02 * r.standard_normal(x.shape) / np.sqrt(x.shape[1])
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.T.astype(np.float32))


def _labels_from_sizes(sizes, N, seed):
    """sizes[k] positions of cluster k, shuffled over the image (the kernels group them by label themselves)."""
    assert sum(sizes) == N, (sizes, N)
    lab = np.concatenate([np.full(n, k, dtype=np.int64) for k, n in enumerate(sizes)])
    return np.random.default_rng(seed).permutation(lab)


def _incidence(S, labels, seed, bare=None):
    """bool [S][N]: about a third of the tokens per segment, the first segment at least one token; no token of cluster `bare`."""
    r = np.random.default_rng(seed)
    inc = r.random((S, labels.size)) < 0.35
    if S:
        inc[0, int(np.argmax(labels != bare))] = True
    if bare is not None:
        inc[:, labels == bare] = False
    return inc


def _case(K, D, P, sizes_per_image, S_per_image, seed, bare0=None, vocab=None):
    from oracle import segvlad_oracle as O
    from revisit_anything_amd import synth

    C = synth.make_vocab(K, D, seed=1000 + K) if vocab is None else vocab
    N = sum(sizes_per_image[0])
    labs = [_labels_from_sizes(sz, N, seed + 10 * b) for b, sz in enumerate(sizes_per_image)]
    tok = np.stack([_tokens(C, lab, seed + 100 + b) for b, lab in enumerate(labs)])
    incs = [_incidence(S, lab, seed + 200 + b, bare0 if b == 0 else None) for b, (S, lab) in enumerate(zip(S_per_image, labs))]
    off = np.concatenate([[0], np.cumsum(S_per_image)]).astype(np.int32)
    bits = np.concatenate([O.pack_bits_u64(i) for i in incs if len(i)] or [np.zeros((0, (N + 63) // 64), dtype="<u8")])
    for b, lab in enumerate(labs):   # the case is what it says: the oracle puts every token where the sizes want it
        got, gap = O.assign_labels(O.normalize_tokens_f32(tok[b]), C)
        assert np.array_equal(got, lab) and gap.min() > 1e-3, (b, float(gap.min()))
    return dict(K=K, D=D, P=P, N=N, C=C, tok=tok, incs=incs, off=off, bits=bits.view(np.int64), labs=labs,
                pca=synth.make_pca_model(K * D, P, seed=5000 + P))


def _sizes(K, b, N=N_GRID):
    """Cluster sizes of image b: K > 1 leaves the last cluster empty; the others take 33 / 32 / 17 / 16 / 1 in rotation, the last
    used one the rest."""
    used = max(1, K - 1)
    pool = (33, 32, 17, 16, 1)
    sz = [pool[(b + k) % len(pool)] for k in range(used - 1)]
    return sz + [N - sum(sz)] + [0] * (K - used)


@functools.lru_cache(maxsize=None)
def _grid_case(B, D, P, K):
    j = GRID.index((B, D, P, K))
    S = [S_POOL[(j + b) % 4] for b in range(B)]
    if B == 3:
        S[1] = 0   # an image without a segment
    return _case(K, D, P, [_sizes(K, b) for b in range(B)], S, seed=7 * j, bare0=0 if K > 1 else None)


@functools.lru_cache(maxsize=None)
def _sizes_case():
    return _case(6, 32, 36, [[0, 1, 16, 17, 32, 33], [33, 0, 32, 1, 17, 16], [16, 17, 0, 33, 1, 32]], [33, 3, 1], seed=901, bare0=3)


@functools.lru_cache(maxsize=None)
def _tiles_case(which):
    # N = 20, K = 5 with cluster 4 unused: 1, 2, 3 and 4 tiles per image
    per = {"a": [[20, 0, 0, 0, 0], [10, 10, 0, 0, 0], [7, 7, 6, 0, 0]], "b": [[5, 5, 5, 5, 0], [0, 12, 8, 0, 0], [0, 0, 20, 0, 0]]}[which]
    return _case(5, 32, 36, per, [3, 33, 1] if which == "a" else [65, 1, 3], seed=950 + ord(which))


@functools.lru_cache(maxsize=None)
def _reference(key):
    from oracle import segvlad_oracle as O

    d = key()
    mean, comps, var = d["pca"]
    rows = [O.seg_vlad(d["tok"][b], inc, d["C"]) for b, inc in enumerate(d["incs"]) if len(inc)]
    ref = O.pca_transform(np.concatenate(rows), mean, comps, var, True)
    ref.setflags(write=False)
    return ref


def _engine(d):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    eng.set_vocab(d["C"])
    eng.pca_set(*d["pca"], whiten=True)
    eng.set_option("pca_path", "project")
    return eng


def _run(eng, d, planes, cover, l2norm=False):
    eng.set_option("pj_planes", planes)
    eng.set_option("cover_rows", cover)
    y = eng.seg_vlad_pca(torch.from_numpy(d["tok"]).cuda(), torch.from_numpy(d["bits"]).cuda(), d["off"], None, l2norm=l2norm)["out"]
    return y.cpu().numpy()


def _check(d, ref, tag):
    eng = _engine(d)
    try:
        base = _run(eng, d, 0, 0)
        assert base.shape == (int(d["off"][-1]), d["P"]) and np.isfinite(base).all()
        for planes, cover in ((1, 0), (1, 1), (0, 1)):
            y = _run(eng, d, planes, cover)
            assert _bits_equal(y, base), (tag, planes, cover, float(np.abs(y - base).max()))
        err, bound = float(np.abs(base - ref).max()), 3e-5 * float(np.abs(ref).max())
        print(f"{tag}: max|err| = {err:.3e}, bound = {bound:.3e}")
        assert err <= bound, tag
        yn = _run(eng, d, 1, 1, l2norm=True)
        assert _bits_equal(yn, _run(eng, d, 0, 1, l2norm=True)), tag
    finally:
        eng.close()


@pytest.mark.parametrize("B,D,P,K", GRID)
def test_pj_planes_bits_and_oracle_over_the_grid(B, D, P, K):
    key = functools.partial(_grid_case, B, D, P, K)
    d = key()
    if K > 1:   # cluster 0 of image 0 holds positions and no segment covers one of them
        assert (d["labs"][0] == 0).any() and not d["incs"][0][:, d["labs"][0] == 0].any()
    _check(d, _reference(_HashablePartial(key)), f"B{B} D{D} P{P} K{K}")


class _HashablePartial:
    """functools.partial with value equality, so that the shared reference is computed once per case."""

    def __init__(self, p):
        self.p = p

    def __call__(self):
        return self.p()

    def __hash__(self):
        return hash((self.p.func, self.p.args))

    def __eq__(self, o):
        return (self.p.func, self.p.args) == (o.p.func, o.p.args)


def test_pj_planes_cluster_sizes_around_the_tile():
    d = _sizes_case()
    assert sorted(np.bincount(d["labs"][0], minlength=6).tolist()) == [0, 1, 16, 17, 32, 33]
    _check(d, _reference(_sizes_case), "sizes")


@pytest.mark.parametrize("which", ["a", "b"])
def test_pj_planes_images_of_one_to_four_tiles(which):
    key = _HashablePartial(functools.partial(_tiles_case, which))
    d = key()
    tiles = sorted(int(np.ceil(np.bincount(lab, minlength=5) / 32).sum()) for lab in d["labs"])
    assert tiles == ([1, 2, 3] if which == "a" else [1, 2, 4])
    _check(d, _reference(key), f"tiles {which}")


def test_pj_planes_changes_nothing_where_the_16_bit_form_is_off():
    """The unused centre's norm overflows fp32 -> the plan's bound on |z| is not finite -> zscale = 0, fp32-MFMA aggregation over fp32 Z."""
    from revisit_anything_amd import synth

    C = synth.make_vocab(3, 32, seed=1003).copy()
    C[2] = 4e18
    d = _case(3, 32, 36, [[33, 66, 0], [50, 49, 0], [1, 98, 0]], [3, 33, 1], seed=977, vocab=C)
    eng = _engine(d)
    try:
        base = _run(eng, d, 0, 1)
        assert np.isfinite(base).all()
        assert _bits_equal(_run(eng, d, 1, 1), base) and _bits_equal(_run(eng, d, 1, 0), base)
        eng.set_option("pj_f16", 0)
        assert _bits_equal(_run(eng, d, 1, 1), base)
    finally:
        eng.close()


def test_pj_planes_twice_in_one_context_with_other_masks():
    da, db = _tiles_case("a"), _tiles_case("b")
    dc = _grid_case(3, 32, 36, 5)   # same K, D, P: one vocabulary and one model serve the three batches
    assert np.array_equal(da["C"], dc["C"]) and all(np.array_equal(x, y) for x, y in zip(da["pca"], dc["pca"]))
    eng = _engine(da)
    try:
        got = {}
        for w, planes, cover in (("c", 1, 1), ("a", 1, 1), ("b", 1, 1), ("c", 1, 0), ("a", 0, 1), ("b", 0, 0), ("c", 0, 1), ("a", 1, 0), ("b", 1, 1)):
            d = {"a": da, "b": db, "c": dc}[w]
            y = _run(eng, d, planes, cover, l2norm=True)
            assert np.isfinite(y).all()
            assert _bits_equal(y, got.setdefault(w, y)), (w, planes, cover)
    finally:
        eng.close()
