"""Soft-assignment VLAD on the device (option vlad_assign=soft:<T>, include/segvlad.h) against its fp64 restatement
(tests/soft_vlad_ref.py) over the describe stage's shape table, imported unchanged from tests/describe_shape_cases.py.

Bounds (none of them new):
  descriptor   max |out - ref| < 1e-6 and 1 - cos < 1e-6 per row; block norms rtol 1e-5 / atol 1e-6 (tests/test_gpu_parity.py's
               hard path); labels and gap EQUAL to the hard call's; image 3 bit-equal to image 0; the uncovered segment's row 0
  projected    3e-5 of max |ref| against the restatement pushed through the fp64 PCA -- the planes form's bound of
               tests/test_gpu_describe_shapes.py at these shapes
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import describe_shape_cases as T
import soft_vlad_ref as SR

pytestmark = pytest.mark.gpu

DESC_TOL, COS_TOL, PCA_RTOL = 1e-6, 1e-6, 3e-5


def _engine(C, pca=None, guard=None):
    if guard is None:
        from revisit_anything_amd.engine import SegVLADEngine

        eng = SegVLADEngine(0)
    else:
        import async_order as A

        eng = A.make_engine(guard)
    eng.set_vocab(C)
    if pca is not None:
        eng.pca_set(*pca, whiten=True)
    return eng


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _images(eng, d, with_adj):
    return _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"] if with_adj else None, want_labels=True, want_gap=True,
                            want_block_norms=True))


def _row_errors(out, ref):
    err = float(np.abs(out - ref).max())
    nz = np.sqrt((ref * ref).sum(1)) > 0
    o = out[nz].astype(np.float64)
    cos = (o * ref[nz]).sum(1) / (np.sqrt((o * o).sum(1)) * np.sqrt((ref[nz] * ref[nz]).sum(1)))
    return err, float((1.0 - cos).max()) if nz.any() else 0.0


def _check_soft(tag, r, ref, hard, offs, bn_rtol=1e-5):
    err, cos_err = _row_errors(r["out"], ref["out"])
    bn_err = float(np.abs(r["block_norms"] - ref["block_norms"]).max())
    print(f"{tag}: max|out-ref| {err:.3e} (bound {DESC_TOL:.0e}), max 1-cos {cos_err:.3e} (bound {COS_TOL:.0e}), block-norm err {bn_err:.3e}")
    assert r["out"].shape == ref["out"].shape and err < DESC_TOL, tag
    assert cos_err < COS_TOL, tag
    assert np.allclose(r["block_norms"], ref["block_norms"], rtol=bn_rtol, atol=1e-6), tag
    assert _bits_equal(r["labels"], hard["labels"]) and _bits_equal(r["gap"], hard["gap"]), tag      # the audit outputs stay the hard ones
    assert ref["zero_rows"].any() and np.all(r["out"][ref["zero_rows"]] == 0), tag
    assert np.all(r["block_norms"][ref["zero_rows"]] == 0), tag
    s0, s3 = slice(offs[0], offs[1]), slice(offs[3], offs[4])
    for key in ("out", "block_norms"):
        assert _bits_equal(r[key][s0], r[key][s3]), (tag, key)                                        # image 3 is image 0


# ---- 1. the shape table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_adj", (True, False), ids=("adj", "noadj"))
@pytest.mark.parametrize("name", SR.CASES)
def test_shape_table_against_the_restatement(name, with_adj):
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        hard = _images(eng, d, with_adj)
        for temp in SR.TEMPS:
            eng.set_vlad_assign("soft", temp)
            r = _images(eng, d, with_adj)
            _check_soft(f"{name} adj={int(with_adj)} T={temp:g}", r, SR.reference(name, with_adj, temp), hard, d["offs"])
            if d["K"] == 1:      # every weight is exactly 1: the hard call's blocks, whatever the temperature
                assert np.allclose(r["block_norms"], hard["block_norms"], rtol=1e-5, atol=1e-6)
                assert np.abs(r["out"] - hard["out"]).max() < DESC_TOL
        assert eng.vlad_assign == "soft:1.0e+02"
    finally:
        eng.close()


# ---- 1b. soft_pooled: the reference's blocks, every one against all centres ------------------------------------------------------
POOLED_CASES = ["k1_d32_n130", "k31_d64_n257", "k65_d200_n333", "k128_d64_n513_s129"]   # K = 1; a padded centre; D % 32 != 0; SC = 3


@pytest.mark.parametrize("with_adj", (True, False), ids=("adj", "noadj"))
@pytest.mark.parametrize("name", POOLED_CASES)
def test_shape_table_pooled_against_the_restatement(name, with_adj):
    """vlad_assign=soft_pooled:<T>: the descriptor at the bounds of soft:<T>.

    The block norms, ||K sum w x^ - (sum w) sum_c c_c||, get a relative bound worked out from the number format, not the hard path's
    1e-5 alone.  A pooled block is K sum_n w[n][k] (x^_n - m) with |x^_n - m| of order 1 for EVERY cluster, so a far cluster's norm is
    carried by a few small weights and inherits their relative error undamped (under soft:<T> such a block is small and the atol of
    1e-6 covers it).  An fp32 softmax weight has the relative error T x (the error of two fp32 scores); a score is a D-term fp32 dot
    product of unit vectors, sqrt(D) 2^-24 by the usual probabilistic bound.  Hence rtol = 1e-5 + 2 T sqrt(D) 2^-24: 1.2e-5 at T = 1
    and 1.8e-4 at T = 100 for D = 200.  (fp32 torch, the reference's own arithmetic, puts 1.7e-5 on a weight at T = 100 there.)"""
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        hard = _images(eng, d, with_adj)
        for temp in SR.TEMPS:
            eng.set_vlad_assign("soft", temp)
            own = _images(eng, d, with_adj)
            eng.set_vlad_assign("soft_pooled", temp)
            r = _images(eng, d, with_adj)
            ref = SR.reference(name, with_adj, temp, True)
            s0 = slice(d["offs"][0], d["offs"][1])
            bn32 = SR.pooled_block_norms_fp32(d["toks"][0], d["C"], d["incs"][0], d["adjs"][0] if with_adj else None, temp)
            print(f"{name} pooled adj={int(with_adj)} T={temp:g}: block norms need rtol {SR.needed_rtol(r['block_norms'], ref['block_norms']):.3e} "
                  f"on the device (image 0: {SR.needed_rtol(r['block_norms'][s0], ref['block_norms'][s0]):.3e}), "
                  f"{SR.needed_rtol(bn32, ref['block_norms'][s0]):.3e} in fp32 torch (image 0); "
                  f"bound {1e-5 + 2.0 * temp * np.sqrt(d['D']) * 2.0 ** -24:.3e}")
            _check_soft(f"{name} pooled adj={int(with_adj)} T={temp:g}", r, ref, hard, d["offs"],
                        bn_rtol=1e-5 + 2.0 * temp * np.sqrt(d["D"]) * 2.0 ** -24)
            if d["K"] == 1:      # one centre: all centres are that centre
                assert np.abs(r["out"] - own["out"]).max() < DESC_TOL
            else:
                assert np.abs(r["out"] - own["out"]).max() > 1e-3
        assert eng.vlad_assign == "soft_pooled:1.0e+02"
    finally:
        eng.close()


def test_pooled_projected_and_launches():
    """soft_pooled through segvlad_images_pca (planes form; project refused), twice the same bytes, one launch more than soft"""
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    name, temp = "k33_d96_n129", 10.0
    d = T.build(name)
    eng = _engine(d["C"], T.pca_model(name))
    try:
        eng.set_vlad_assign("soft_pooled", temp)
        desc = SR.reference(name, True, temp, True)["out"]
        from oracle import segvlad_oracle as O

        ref = O.normalize_feat(O.pca_transform(desc, *T.pca_model(name), True))
        y = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=True)["out"].cpu().numpy()
        _check_y(f"{name} pooled images_pca", y, ref, d["offs"])
        r = _np(eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=True, want_desc=True))
        _check_y(f"{name} pooled images_pca + desc", r["out"], ref, d["offs"])
        err, cos_err = _row_errors(r["desc"], desc)
        print(f"{name} pooled images_pca desc_out: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
        assert err < DESC_TOL and cos_err < COS_TOL
        s1, s2 = _images(eng, d, True), _images(eng, d, True)
        assert all(_bits_equal(s1[k], s2[k]) for k in s1)
        assert _launches(eng, d) == {"assign": 2, "prep": 1, "aggregate": 3}
        eng.set_option("pca_path", "project")
        with pytest.raises(SegVLADError) as ei:
            eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])
        assert ei.value.code == SEGVLAD_ERR_LIMIT and "vlad_assign=soft_pooled:10" in str(ei.value), ei.value
        eng.set_option("pca_path", "auto")
        eng.set_vlad_assign("hard")
        assert _launches(eng, d) == HARD_LAUNCHES
    finally:
        eng.close()


# ---- 2. the projected forms ----------------------------------------------------------------------------------------------------
def _check_y(tag, y, ref, offs, twin=True):
    err, bound = float(np.abs(y - ref).max()), PCA_RTOL * float(np.abs(ref).max())
    print(f"{tag}: max|y-ref| {err:.3e} (bound {bound:.3e})")
    assert y.shape == ref.shape and err <= bound, tag
    assert not twin or _bits_equal(y[offs[0]:offs[1]], y[offs[3]:offs[4]]), tag


@pytest.mark.parametrize("name", SR.PCA_CASES)
def test_images_pca_with_and_without_the_descriptor(name):
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d, temp = T.build(name), 10.0
    eng = _engine(d["C"], T.pca_model(name))
    try:
        eng.set_vlad_assign("soft", temp)
        for l2norm in (True, False):
            ref = SR.pca_reference(name, True, temp, l2norm)
            y = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm)["out"].cpu().numpy()
            _check_y(f"{name} images_pca l2norm={int(l2norm)}", y, ref, d["offs"])
            r = _np(eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm, want_desc=True))
            _check_y(f"{name} images_pca + desc l2norm={int(l2norm)}", r["out"], ref, d["offs"])
            err, cos_err = _row_errors(r["desc"], SR.reference(name, True, temp)["out"])
            print(f"{name} images_pca desc_out: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
            assert err < DESC_TOL and cos_err < COS_TOL
        # the project form presupposes one cluster per token: refused, the context stays usable, auto takes the planes form
        eng.set_option("pca_path", "project")
        with pytest.raises(SegVLADError) as ei:
            eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])
        assert ei.value.code == SEGVLAD_ERR_LIMIT and "pca_path" in str(ei.value) and "vlad_assign" in str(ei.value), ei.value
        eng.set_option("pca_path", "auto")
        y = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=True)["out"].cpu().numpy()
        _check_y(f"{name} images_pca after the refusal", y, SR.pca_reference(name, True, temp, True), d["offs"])
    finally:
        eng.close()


@pytest.mark.parametrize("name", SR.PCA_CASES)
def test_describe_and_begin_flags_end_with_a_patched_adjacency(name):
    """From masks: the device's own incidence and adjacency feed the restatement, so only the soft kernels are under test"""
    from oracle import segvlad_oracle as O
    from revisit_anything_amd import synth
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d, temp = T.build(name), 10.0
    h, w = T.image_grid(d["N"])
    H, W = 14 * h, 14 * w
    Hm, Wm = H // 2, W // 2
    segs, offs = d["case"]["segs"], d["offs"]
    masks = np.concatenate([synth.make_masks(S, Hm, Wm, seed=300 + b, hmin=4, hmax=max(Hm // 2, 5), wmin=4, wmax=max(Wm // 2, 5))
                            for b, S in enumerate(segs)]).astype(np.uint8)
    eng = _engine(d["C"], T.pca_model(name))

    def restated(bits, adj, l2norm=True):
        inc = O.unpack_bits_u64(bits.cpu().numpy().view(np.uint64), d["N"])
        adj = adj.cpu().numpy()
        incs, adjs, pos = [], [], 0
        for b in range(T.B):
            n = int(offs[b + 1] - offs[b])
            incs.append(inc[offs[b]:offs[b + 1]]), adjs.append(adj[pos:pos + n * n].reshape(n, n).astype(bool))
            pos += n * n
        desc = np.concatenate([SR.soft_vlad(d["toks"][b], d["C"], incs[b], adjs[b], temp)["out"] for b in range(T.B)])   # (image 3 has masks of its own)
        y = O.pca_transform(desc, *T.pca_model(name), True)
        return desc, (O.normalize_feat(y) if l2norm else y)

    try:
        eng.set_vlad_assign("soft", temp)
        masks_d, tok_d = torch.from_numpy(masks).cuda(), torch.from_numpy(d["tok"]).cuda()
        r = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True, l2norm=True, want_desc=True)
        desc, y = restated(r["bits"], r["adj"])
        _check_y(f"{name} describe", r["out"].cpu().numpy(), y, offs, twin=False)
        err, cos_err = _row_errors(r["desc"].cpu().numpy(), desc)
        print(f"{name} describe desc: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
        assert err < DESC_TOL and cos_err < COS_TOL
        raw = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=False)
        assert torch.equal(raw["out"], r["desc"])                      # the same kernels: the same bytes
        # begin / flags / end, image 2's adjacency replaced by a host block
        hnd = eng.describe_begin(masks_d, tok_d, offs, H, W, 14, 2, pca=True)
        eng.describe_flags(hnd)
        n2 = int(offs[3] - offs[2])
        blk = (np.random.Generator(np.random.PCG64(41)).random((n2, n2)) < 0.3).astype(np.uint8)
        blk[np.arange(n2), np.arange(n2)] = 1
        e = eng.describe_end(hnd, patch_images=np.array([2], np.int32), patch_blocks=[blk], l2norm=True, want_desc=True)
        adj_p = r["adj"].clone()
        a2 = int(sum(int(offs[b + 1] - offs[b]) ** 2 for b in range(2)))
        adj_p[a2:a2 + n2 * n2] = torch.from_numpy(blk.reshape(-1)).to(adj_p.device)
        desc_p, y_p = restated(r["bits"], adj_p)
        _check_y(f"{name} begin/flags/end patched", e["out"].cpu().numpy(), y_p, offs, twin=False)
        err, _ = _row_errors(e["desc"].cpu().numpy(), desc_p)
        assert err < DESC_TOL and np.abs(desc_p - desc).max() > 1e-3    # (the patch changed the answer)
        # explicit project: refused by describe and by describe_begin, nothing left open
        eng.set_option("pca_path", "project")
        for call in (lambda: eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True),
                     lambda: eng.describe_begin(masks_d, tok_d, offs, H, W, 14, 2, pca=True)):
            with pytest.raises(SegVLADError) as ei:
                call()
            assert ei.value.code == SEGVLAD_ERR_LIMIT, ei.value
        eng.set_option("pca_path", "auto")
        again = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True, l2norm=True)
        assert torch.equal(again["out"], r["out"])
    finally:
        eng.close()


# ---- 3. saturation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_adj", [("k2_d36_n65", False), ("k31_d64_n257", True), ("k65_d200_n333", True), ("k128_d64_n513_s129", False)])
def test_a_saturating_temperature_is_the_hard_assignment(name, with_adj):
    """SATURATING_TEMP x (the gap the table's qualification guarantees) = 120: every weight but the arg-max's is 0 in fp32"""
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        hard = _images(eng, d, with_adj)
        assert hard["gap"].min() >= SR.MIN_GAP * 0.99
        eng.set_vlad_assign("soft", SR.SATURATING_TEMP)
        soft = _images(eng, d, with_adj)
        err = float(np.abs(soft["out"] - hard["out"]).max())
        bn_err = float(np.abs(soft["block_norms"] - hard["block_norms"]).max())
        print(f"{name} adj={int(with_adj)} T={SR.SATURATING_TEMP:g}: max|soft-hard| {err:.3e} (bound {DESC_TOL:.0e}), block norms {bn_err:.3e}")
        assert err < DESC_TOL
        assert np.allclose(soft["block_norms"], hard["block_norms"], rtol=1e-5, atol=1e-6)
    finally:
        eng.close()


# ---- 4. the option's life ------------------------------------------------------------------------------------------------------
REFUSED = ("soft", "soft:", "Soft:1", "SOFT:1", "soft:0", "soft:-1", "soft:nan", "soft:inf", "soft:1e50", "soft:1e-50", "soft:1x", "soft:1 ",
           "soft: 1", "soft:0x10", "soft:1,5", "softmax", "", "Hard", "hard:1",
           "soft_pooled", "soft_pooled:", "soft_pooled:0", "soft_pooled:nan", "soft_pooled:1x", "Soft_pooled:1", "soft_pooled 1", "soft_pool:1")
HARD_LAUNCHES = {"assign": 1, "prep": 1, "aggregate": 1}      # what segvlad_images issues without the option


def _launches(eng, d, pca=False):
    eng.set_profiling(True)
    eng.profile_reset()
    if pca:
        eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])
    else:
        eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"])
    eng.synchronize()
    n = {s: eng.stage_ms(s)[1] for s in ("assign", "prep", "aggregate") + (("pca",) if pca else ())}
    eng.set_profiling(False)
    return n


def test_the_options_life():
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    name = "k33_d96_n129"
    d = T.build(name)
    fresh = _engine(d["C"], T.pca_model(name))
    eng = _engine(d["C"], T.pca_model(name))
    plain = _engine(d["C"], T.pca_model(name), guard=False)
    try:
        hard0 = _images(fresh, d, True)
        y0 = fresh.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy()
        n_hard0, n_pca0 = _launches(fresh, d), _launches(fresh, d, pca=True)
        assert n_hard0 == HARD_LAUNCHES, n_hard0
        # soft, twice: the same bytes; the plain (unguarded) library: the same bytes
        eng.set_vlad_assign("soft", 10.0)
        s1, s2 = _images(eng, d, True), _images(eng, d, True)
        assert all(_bits_equal(s1[k], s2[k]) for k in s1)
        ys = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy()
        plain.set_vlad_assign("soft", 10.0)
        sp = _images(plain, d, True)
        assert all(_bits_equal(s1[k], sp[k]) for k in s1)
        assert _bits_equal(ys, plain.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy())
        assert not _bits_equal(s1["out"], hard0["out"])
        n_soft = _launches(eng, d)
        assert n_soft == {"assign": 2, "prep": 1, "aggregate": 2}, n_soft
        # every refusal leaves soft:10 in force
        for value in REFUSED:
            with pytest.raises(SegVLADError) as ei:
                eng.set_option("vlad_assign", value)
            assert ei.value.code == SEGVLAD_ERR_ARG, (value, ei.value)
            assert eng.vlad_assign == "soft:1.0e+01"
        assert all(_bits_equal(s1[k], v) for k, v in _images(eng, d, True).items())
        # back to hard: the fresh context's bytes and launches
        assert eng.set_vlad_assign("hard") == "soft:1.0e+01"
        h1 = _images(eng, d, True)
        assert all(_bits_equal(hard0[k], h1[k]) for k in hard0)
        assert _bits_equal(y0, eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy())
        assert _launches(eng, d) == n_hard0 and _launches(eng, d, pca=True) == n_pca0
        # a refusal under hard leaves hard
        with pytest.raises(SegVLADError):
            eng.set_option("vlad_assign", "soft:")
        assert all(_bits_equal(hard0[k], v) for k, v in _images(eng, d, True).items())
    finally:
        for e in (fresh, eng, plain):
            e.close()


# ---- 5. the entries out of the option's reach ----------------------------------------------------------------------------------
def test_kmeans_step_and_cluster_aggregate_ignore_the_option():
    from oracle import segvlad_oracle as O

    name = "k33_d96_n129"
    d = T.build(name)
    K, D, N = d["K"], d["D"], d["N"]
    xn = O.normalize_tokens_f32(d["toks"][0])
    labels, _ = O.assign_labels(xn, d["C"])
    res = (xn - d["C"][labels]).astype(np.float32)
    bits0 = d["bits"][d["offs"][0]:d["offs"][1]]
    eng = _engine(d["C"])

    def both():
        sums = torch.zeros((K, D), dtype=torch.float64, device="cuda")
        counts = torch.zeros(K, dtype=torch.int64, device="cuda")
        lab = eng.kmeans_step(d["tok"], sums, counts, want_labels=True)
        ca = eng.cluster_aggregate(K, res, labels.astype(np.uint8), bits0, d["adjs"][0].astype(np.uint8).reshape(-1))
        return {"sums": sums.cpu().numpy(), "counts": counts.cpu().numpy(), "labels": lab.cpu().numpy(), "ca": ca.cpu().numpy()}

    try:
        hard = both()
        eng.set_vlad_assign("soft", 10.0)
        soft = both()
        for k in hard:
            assert _bits_equal(hard[k], soft[k]), k
    finally:
        eng.close()


# ---- 7. the drop-in surface ----------------------------------------------------------------------------------------------------
def test_aggFt_with_a_soft_vlad_object_on_the_fixtures_inputs():
    """func_vpr.aggFt(vlad=VLAD(vlad_mode='soft', soft_temp=T)) against tests/golden/vlad_soft.npz, the reference's VLAD.generate
    (an fp32 torch result), at 1e-6.  aggFt sets soft_pooled for such an object: utilities.py:883-884 sums, for cluster k, the
    weighted residuals against ALL centres ("q c d -> (q c) d")."""
    import os
    import types

    import revisit_anything_amd.func_vpr as fv

    voc, toks = SR.golden_inputs()
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vlad_soft.npz"))
    Gm = SR.golden_projection(voc)
    h5 = {f"img_{j}.jpg": {"ift_dino": t.reshape(1, 1536, 34, 45)} for j, t in enumerate(toks)}
    eng = fv.engine()
    before = eng.vlad_assign
    worst_sub = worst_proj = 0.0
    for temp in SR.GOLDEN_TEMPS:
        vlad = types.SimpleNamespace(c_centers=torch.from_numpy(voc), num_clusters=32, desc_dim=1536, intra_norm=True, norm_descs=True,
                                     mode="cosine", vlad_mode="soft", soft_temp=temp)
        out = fv.aggFt(h5, None, None, {"desired_height": 480, "desired_width": 640}, "vlad", vlad)
        assert eng.vlad_assign == before                                 # the option is put back
        for j in range(2):
            ref = SR.soft_vlad(toks[j], voc, np.ones((1, 34 * 45), bool), None, temp, pooled=True)["out"][0]
            err = float(np.abs(out[j] - ref).max())
            fix = float(np.abs(out[j][::37] - z[f"vlad{j}_t{int(temp)}_sub"]).max())
            print(f"aggFt soft T={temp:g} image {j}: against the pooled restatement {err:.3e}, against the fixture {fix:.3e}")
            assert err < DESC_TOL
            worst_sub = max(worst_sub, fix)
            worst_proj = max(worst_proj, float(np.abs(out[j].astype(np.float64) @ Gm - z[f"vlad{j}_t{int(temp)}_proj"]).max()))
    hard = fv.aggFt(h5, None, None, {}, "vlad", torch.from_numpy(voc))    # bare centres: hard, as before
    assert np.abs(hard[0] - out[0]).max() > 1e-3
    assert worst_sub < 1e-6 and worst_proj < 2e-4, (worst_sub, worst_proj)     # (tests/test_gpu_shim.py's bounds of the hard fixture)
