"""Option cover_rows (fused segment-VLAD -> PCA, "project" form): only the tokens that some segment covers -- after the
adjacency union -- get a row of the grouped residual planes and of the projected tokens Z; the others are left out of the
projection GEMM.  Every kernel keeps its LOGICAL positions (task sizes, Gram tiles, 32-row aggregation tiles), only the
physical row of a token moves, so cover_rows = 1 must give the bits of cover_rows = 0: checked for the four task-size
classes of the token kernels (a task = the tokens of one image in one cluster), with and without the adjacency union and
the final normalisation, through the fused describe entry, across calls of one context (stale row maps), and -- so that
both settings cannot be wrong alike -- against the fp64 oracle.

Oracle tolerance: 3e-5 of max |reference|, the bound tests/test_gpu_parity.py holds this form to against the same oracle
(tests/test_gpu_describe.py compares entry points bit for bit and has no oracle bound of its own)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, P, B = 64, 32, 4
# (K, H, W): tokens of one image in one cluster
SHAPES = {
    "k32_le32": (32, 126, 154),      # N = 99: <= 32 per task (one Gram tile), empty clusters, clusters without a covered token
    "k2_33to64": (2, 126, 154),      # 33 .. 64 (two Gram tiles)
    "k1_65to255": (1, 126, 154),     # 99: the block-sum kernel, lists in LDS
    "k1_big": (1, 210, 280),         # N = 300 >= 256: the block-sum kernel's BIG instantiation
}


def _rect(Hm, Wm, y0, x0, h, w):
    m = np.zeros((Hm, Wm), dtype=bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def _mask_set(Hm, Wm, which):
    """Per-image mask lists.  Set 0: image 0 a few small rectangles (most tokens uncovered), image 1 one full-frame mask,
    image 2 no segment, image 3 several masks with an empty one.  Set 1: other counts and coverage per image."""
    from revisit_anything_amd import synth

    small = [_rect(Hm, Wm, 3, 5, 10, 12), _rect(Hm, Wm, Hm // 2, Wm // 2, 9, 15), _rect(Hm, Wm, Hm - 14, 2, 8, 8)]
    if which == 0:
        several = synth.make_masks(5, Hm, Wm, seed=77, hmin=6, hmax=30, wmin=6, wmax=40)
        several[2] = False
        per = [np.stack(small), np.ones((1, Hm, Wm), dtype=bool), np.zeros((0, Hm, Wm), dtype=bool), several]
    else:
        per = [np.ones((1, Hm, Wm), dtype=bool), np.stack(small + [_rect(Hm, Wm, 20, 30, 7, 7)]),
               synth.make_masks(6, Hm, Wm, seed=78, hmin=6, hmax=30, wmin=6, wmax=40), np.zeros((0, Hm, Wm), dtype=bool)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    return per, off


@functools.lru_cache(maxsize=None)
def _data(shape, which=0):
    from revisit_anything_amd import synth

    K, H, W = SHAPES[shape]
    N = (H // 14) * (W // 14)
    C = synth.make_vocab(K, D, seed=1000)
    used = C[:28] if K == 32 else C              # K = 32: clusters 28 .. 31 stay empty
    tok = np.stack([synth.make_tokens(used, N, seed=40 + b, noise=0.1) for b in range(B)])
    per, off = _mask_set(H // 2, W // 2, which)
    mean, comps, var = synth.make_pca_model(K * D, P, seed=5000)
    return dict(K=K, H=H, W=W, N=N, C=C, tok=tok, per=per, off=off, masks=np.concatenate(per).astype(np.uint8), pca=(mean, comps, var))


def _engine(d):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    eng.set_vocab(d["C"])
    eng.pca_set(*d["pca"], whiten=True)
    eng.set_option("pca_path", "project")
    return eng


def _inputs(eng, d, order):
    masks = torch.from_numpy(d["masks"]).cuda()
    bits, cent = eng.incidence_centroids(masks, d["H"], d["W"], 14)
    adj = eng.adjacency_flagged(cent, d["off"], order, device_flags=True)[0] if order else None
    return torch.from_numpy(d["tok"]).cuda(), bits, adj


def _run(eng, cover, tok, bits, off, adj, l2norm):
    eng.set_option("cover_rows", cover)
    return eng.seg_vlad_pca(tok, bits, off, adj, l2norm=l2norm)["out"].cpu().numpy()


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_shape_class(eng, d, shape, tok, bits, adj):
    """The case is what its name says: task sizes, and the coverage the mask set was built for."""
    from oracle import segvlad_oracle as O

    lab = eng.seg_vlad(tok, bits, d["off"], adj, want_labels=True)["labels"].cpu().numpy()
    cnt = np.stack([np.bincount(lab[b], minlength=d["K"]) for b in range(B)])
    lo, hi = {"k32_le32": (0, 32), "k2_33to64": (33, 64), "k1_65to255": (65, 255), "k1_big": (256, 10 ** 9)}[shape]
    assert cnt.min() >= lo and cnt.max() <= hi, (shape, cnt.min(), cnt.max())
    cov0 = O.incidence(d["per"][0], d["H"], d["W"]).any(0)
    assert cov0.sum() > 0 and 2 * cov0.sum() < d["N"]                      # image 0: more than half uncovered
    assert O.incidence(d["per"][1], d["H"], d["W"]).all()                  # image 1: every token covered
    if shape == "k32_le32":
        assert (cnt == 0).any()                                            # empty clusters
        held = cnt[0] > 0
        n_cov = np.bincount(lab[0][cov0], minlength=d["K"])
        assert (held & (n_cov == 0)).any() and (held & (n_cov > 0) & (n_cov < cnt[0])).any()   # all / some tokens uncovered


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cover_rows_on_equals_off_bit_for_bit(shape):
    d = _data(shape)
    eng = _engine(d)
    try:
        for order in (0, 2):
            tok, bits, adj = _inputs(eng, d, order)
            if order == 0:
                _check_shape_class(eng, d, shape, tok, bits, adj)
            for l2norm in (True, False):
                on = _run(eng, 1, tok, bits, d["off"], adj, l2norm)
                off = _run(eng, 0, tok, bits, d["off"], adj, l2norm)
                assert np.isfinite(off).all() and off.shape == (int(d["off"][-1]), P)
                assert _bits_equal(on, off), (shape, order, l2norm, float(np.abs(on - off).max()))
    finally:
        eng.close()


def test_cover_rows_through_the_fused_describe_entry():
    d = _data("k32_le32")
    eng = _engine(d)
    try:
        masks, tok = torch.from_numpy(d["masks"]).cuda(), torch.from_numpy(d["tok"]).cuda()
        outs = {}
        for cover in (1, 0, 1):
            eng.set_option("cover_rows", cover)
            r = eng.describe(masks, tok, d["off"], d["H"], d["W"], 14, 2, pca=True, l2norm=True)
            y = r["out"].cpu().numpy()
            assert _bits_equal(y, outs.setdefault(cover, y))
        assert _bits_equal(outs[1], outs[0])
        # ... and the fused entry's rows are the separate calls'
        _, bits, adj = _inputs(eng, d, 2)
        assert _bits_equal(outs[1], _run(eng, 1, tok, bits, d["off"], adj, True))
    finally:
        eng.close()


@pytest.mark.parametrize("shape", ["k32_le32", "k1_65to255"])
def test_cover_rows_against_the_oracle(shape):
    from oracle import segvlad_oracle as O

    d = _data(shape)
    eng = _engine(d)
    try:
        mean, comps, var = d["pca"]
        for order in (0, 2):
            tok, bits, adj = _inputs(eng, d, order)
            y = _run(eng, 1, tok, bits, d["off"], adj, False)
            adj_h = adj.cpu().numpy() if order else None
            refs, a0 = [], 0
            for b in range(B):
                S = len(d["per"][b])
                if S:
                    a = adj_h[a0:a0 + S * S].reshape(S, S).astype(bool) if order else None
                    refs.append(O.seg_vlad_from_masks(d["tok"][b], d["per"][b], d["C"], d["H"], d["W"], a))
                a0 += S * S
            ref = O.pca_transform(np.concatenate(refs), mean, comps, var, True)
            err = float(np.abs(y - ref).max())
            print(f"{shape} order {order}: max|err| = {err:.3e}, bound = {3e-5 * np.abs(ref).max():.3e}")
            assert err <= 3e-5 * np.abs(ref).max(), (shape, order)
        eng.set_option("pca_path", "planes")     # the option is the project form's: the other form runs other kernels
        y_planes = eng.seg_vlad_pca(tok, bits, d["off"], adj, l2norm=False)["out"].cpu().numpy()
        assert not _bits_equal(y, y_planes) and np.abs(y - y_planes).max() <= 1e-5 * np.abs(ref).max()
    finally:
        eng.close()


def test_cover_rows_twice_in_one_context_with_other_masks():
    """The row map and the GEMM's tile list are per call: a second batch with other coverage (more covered rows in some
    clusters, fewer in others, another image without segments) must not meet entries of the first."""
    da, db = _data("k32_le32", 0), _data("k32_le32", 1)
    eng = _engine(da)
    try:
        ins = {w: _inputs(eng, d, 2) for w, d in (("a", da), ("b", db))}
        seq = [("a", 1), ("b", 1), ("a", 1), ("b", 0), ("a", 0), ("b", 1)]
        got = {}
        for w, cover in seq:
            d = da if w == "a" else db
            tok, bits, adj = ins[w]
            y = _run(eng, cover, tok, bits, d["off"], adj, True)
            assert np.isfinite(y).all()
            assert _bits_equal(y, got.setdefault(w, y)), (w, cover)
        assert not _bits_equal(got["a"][:1], got["b"][:1])
    finally:
        eng.close()
