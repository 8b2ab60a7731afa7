"""Burst-discounted VLAD on the device (option vlad_burst=<a>:<b>:<p>, include/segvlad.h) against its fp64 restatement
(tests/burst_ref.py) over the soft kernels' shape table and a probe table that reaches the Gram kernel's tile edges.

Bounds:
  weights      a discounted weight, read through block_norms of single-token segments: rtol = 1e-5 + 2 p a sqrt(D) 2^-24, atol 0
               (|dg| <= g max|dz| since sigmoid' <= sigmoid, |dz| = 2 a |dcos|, an fp32 D-term dot product of unit vectors is off by
               sqrt(D) 2^-24 -- the bound tests/test_gpu_soft_vlad.py uses for 2 T sqrt(D) 2^-24); the other block exactly 0
  descriptor   max |out - ref| < 1e-6 + 4 E_u and 1 - cos < 1e-6 per row, E_u = the move of the fp64 descriptor when its u is
               replaced by the sequential-fp32 restatement's (the device's rounding is another draw of the same noise: factor 4);
               block norms rtol = 1e-5 + 2 (p a + T) sqrt(D) 2^-24, atol 1e-6
  projected    3e-5 of max |ref| (tests/test_gpu_soft_vlad.py's PCA_RTOL)
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import burst_ref as BR
import describe_shape_cases as T
import soft_vlad_ref as SR

pytestmark = pytest.mark.gpu

DESC_TOL, COS_TOL, PCA_RTOL = 1e-6, 1e-6, 3e-5
MAIN = BR.PARAMS[0]


def _engine(C, pca=None):
    import async_order as A

    eng = A.make_engine(True)      # the guarded library: every scratch buffer fenced at the request's exact size
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


def _set(eng, assign, params):
    eng.set_vlad_assign(*assign)       # ("hard", None) | ("soft", T) | ("soft_pooled", T)
    eng.set_vlad_burst(params)


# ---- 1. the weights, through single-token segments ---------------------------------------------------------------------------
@pytest.mark.parametrize("nd", BR.PROBES, ids=BR.probe_id)
def test_weights_on_the_probe_table(nd):
    N, D = nd
    d = BR.probe(N, D)
    eng = _engine(d["C"])
    try:
        for params in BR.PARAMS:
            eng.set_vlad_burst(params)
            bn = eng.seg_vlad(d["tok"], d["bits"], d["offs"], None, want_block_norms=True)["block_norms"].cpu().numpy()
            ref = BR.probe_block_norms(N, D, params)
            on = ref > 0
            rel = float((np.abs(bn[on] - ref[on]) / ref[on]).max())
            bound = BR.weight_rtol(D, params)
            print(f"{BR.probe_id(nd)} {params}: label block off by {rel:.3e} relative (bound {bound:.3e}); other block max {np.abs(bn[~on]).max():.1e}")
            assert bn.shape == ref.shape == (N, 2) and on.sum() == N
            assert np.allclose(bn[on], ref[on], rtol=bound, atol=0.0)
            assert np.all(bn[~on] == 0)
    finally:
        eng.close()


# ---- 2. a = 0: a constant discount cancels in the normalisations --------------------------------------------------------------
@pytest.mark.parametrize("name", BR.CASES)
def test_a_constant_discount_is_the_plain_hard_descriptor(name):
    """0:7:1: g = N sigmoid(7) for every token.  A tile edge that drops or double-counts a column changes g by 1 / N at the least,
    and the block norms with it, orders of magnitude above rtol 1e-5 (the atol is the hard path's 1e-6 times the same constant)."""
    d = T.build(name)
    c = 1.0 / (d["N"] / (1.0 + np.exp(-7.0)))
    eng = _engine(d["C"])
    try:
        eng.set_vlad_burst((0.0, 7.0, 1.0))
        for with_adj in (True, False):
            ref = T.reference(name, with_adj)
            r = _images(eng, d, with_adj)
            err, cos_err = _row_errors(r["out"], ref["out"])
            bn_rel = SR.needed_rtol(r["block_norms"], ref["block_norms"] * c, atol=1e-6 * c)
            print(f"{name} adj={int(with_adj)} 0:7:1: max|out-hard| {err:.3e}, max 1-cos {cos_err:.3e}, block norms need rtol {bn_rel:.3e} (bound 1e-5)")
            assert err < DESC_TOL and cos_err < COS_TOL
            assert np.allclose(r["block_norms"], ref["block_norms"] * c, rtol=1e-5, atol=1e-6 * c)
    finally:
        eng.close()


# ---- 3. p = 0: u is exactly 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k2_d36_n65", "k33_d96_n129", "k65_d200_n333"))
def test_p_zero_is_no_discount(name):
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        eng.set_vlad_assign("soft", 10.0)
        soft = _images(eng, d, True)
        eng.set_vlad_burst((8.0, 7.0, 0.0))
        r = _images(eng, d, True)
        assert all(_bits_equal(soft[k], r[k]) for k in soft)
        eng.set_vlad_assign("hard")
        r = _images(eng, d, True)
        ref = T.reference(name, True)
        err, cos_err = _row_errors(r["out"], ref["out"])
        print(f"{name} hard 8:7:0: max|out-hard| {err:.3e}, max 1-cos {cos_err:.3e}")
        assert err < DESC_TOL and cos_err < COS_TOL
        assert np.allclose(r["block_norms"], ref["block_norms"], rtol=1e-5, atol=1e-6)
    finally:
        eng.close()


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------
def _check(tag, r, ref, eu, bn_rtol, hard, offs):
    err, cos_err = _row_errors(r["out"], ref["out"])
    print(f"{tag}: max|out-ref| {err:.3e} (bound {DESC_TOL + 4 * eu:.3e}, E_u {eu:.3e}), max 1-cos {cos_err:.3e}, "
          f"block norms need rtol {SR.needed_rtol(r['block_norms'], ref['block_norms']):.3e} (bound {bn_rtol:.3e})")
    assert r["out"].shape == ref["out"].shape and np.isfinite(r["out"]).all() and err < DESC_TOL + 4 * eu, tag
    assert cos_err < COS_TOL, tag
    assert np.allclose(r["block_norms"], ref["block_norms"], rtol=bn_rtol, atol=1e-6), tag
    if hard is not None:       # the audit outputs stay the hard arg-max and gap
        assert _bits_equal(r["labels"], hard["labels"]) and _bits_equal(r["gap"], hard["gap"]), tag
    assert np.all(r["out"][ref["zero_rows"]] == 0) and np.all(r["block_norms"][ref["zero_rows"]] == 0), tag
    if offs is not None:       # image 3 is image 0: g depends on the image alone
        s0, s3 = slice(offs[0], offs[1]), slice(offs[3], offs[4])
        for key in ("out", "block_norms"):
            assert _bits_equal(r[key][s0], r[key][s3]), (tag, key)


@pytest.mark.parametrize("with_adj", (True, False), ids=("adj", "noadj"))
@pytest.mark.parametrize("name", BR.CASES)
def test_shape_table_against_the_restatement(name, with_adj):
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        hard = _images(eng, d, with_adj)
        for params in BR.PARAMS:
            for assign in BR.ASSIGNS:
                _set(eng, assign, params)
                r = _images(eng, d, with_adj)
                ref = BR.reference(name, with_adj, assign, params)
                assert ref["zero_rows"].any()
                _check(f"{name} adj={int(with_adj)} {assign[0]} {params}", r, ref, BR.e_u(name, with_adj, assign, params),
                       BR.weight_rtol(d["D"], params, assign[1] or 0.0), hard, d["offs"])
                again = _images(eng, d, with_adj)
                assert all(_bits_equal(r[k], again[k]) for k in r), (name, assign, params)
    finally:
        eng.close()


def test_a_batch_of_eleven_images():
    """B >= 8: the Gram kernel deals its workgroups so that an image's tiles share an XCD (grid padded to a multiple of 8 images; 11
    is none).  Every image's rows are the bytes it has in the table's batch of 4."""
    name, order = "k33_d96_n129", (0, 2, 1, 0, 2, 2, 0, 1, 2, 0, 2)
    d = T.build(name)
    toks, incs, adjs = [d["toks"][b] for b in order], [d["incs"][b] for b in order], [d["adjs"][b] for b in order]
    tok, bits, offs, adj = T.pack_batch(toks, incs, adjs)
    us = BR.case_u_fp32(name, MAIN)
    eng = _engine(d["C"])
    try:
        for assign in BR.ASSIGNS[:2]:
            _set(eng, assign, MAIN)
            r = _np(eng.seg_vlad(tok, bits, offs, adj, want_labels=True, want_gap=True, want_block_norms=True))
            four = _images(eng, d, True)
            ref = BR.batch(toks, incs, adjs, d["C"], True, assign, MAIN)
            alt = BR.batch(toks, incs, adjs, d["C"], True, assign, MAIN, us=[us[b] for b in order])
            _check(f"{name} x 11 {assign[0]}", r, ref, float(np.abs(alt["out"] - ref["out"]).max()),
                   BR.weight_rtol(d["D"], MAIN, assign[1] or 0.0), None, None)
            for j, b in enumerate(order):
                for key in ("out", "block_norms"):
                    assert _bits_equal(r[key][offs[j]:offs[j + 1]], four[key][d["offs"][b]:d["offs"][b + 1]]), (assign, j, key)
    finally:
        eng.close()


# ---- 5. the other entries -----------------------------------------------------------------------------------------------------
def _check_y(tag, y, ref):
    err, bound = float(np.abs(y - ref).max()), PCA_RTOL * float(np.abs(ref).max())
    print(f"{tag}: max|y-ref| {err:.3e} (bound {bound:.3e})")
    assert y.shape == ref.shape and err <= bound, tag


@pytest.mark.parametrize("assign", (("hard", None), ("soft", 10.0)), ids=("hard", "soft10"))
@pytest.mark.parametrize("name", SR.PCA_CASES)
def test_images_pca_takes_the_planes_form_and_refuses_project(name, assign):
    from oracle import segvlad_oracle as O
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d = T.build(name)
    eng = _engine(d["C"], T.pca_model(name))
    try:
        _set(eng, assign, MAIN)
        desc = BR.reference(name, True, assign, MAIN)["out"]
        for l2norm in (True, False):
            y = O.pca_transform(desc, *T.pca_model(name), True)
            ref = O.normalize_feat(y) if l2norm else y
            got = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm)["out"].cpu().numpy()
            _check_y(f"{name} {assign[0]} images_pca l2norm={int(l2norm)}", got, ref)
            r = _np(eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm, want_desc=True))
            _check_y(f"{name} {assign[0]} images_pca + desc l2norm={int(l2norm)}", r["out"], ref)
            err, cos_err = _row_errors(r["desc"], desc)
            print(f"{name} {assign[0]} images_pca desc_out: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
            assert err < DESC_TOL + 4 * BR.e_u(name, True, assign, MAIN) and cos_err < COS_TOL
        eng.set_option("pca_path", "project")
        with pytest.raises(SegVLADError) as ei:
            eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])
        assert ei.value.code == SEGVLAD_ERR_LIMIT and "pca_path" in str(ei.value), ei.value
        if assign[0] == "hard":
            assert "vlad_burst" in str(ei.value), ei.value
        eng.set_option("pca_path", "auto")
        y = O.normalize_feat(O.pca_transform(desc, *T.pca_model(name), True))
        _check_y(f"{name} {assign[0]} images_pca after the refusal",
                 eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=True)["out"].cpu().numpy(), y)
    finally:
        eng.close()


@pytest.mark.parametrize("name", SR.PCA_CASES)
def test_describe_and_begin_flags_end(name):
    """From masks: the device's own incidence and adjacency feed the restatement, so only the weights are under test"""
    from oracle import segvlad_oracle as O
    from revisit_anything_amd import synth
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d, assign = T.build(name), ("hard", None)
    h, w = T.image_grid(d["N"])
    H, W = 14 * h, 14 * w
    Hm, Wm = H // 2, W // 2
    segs, offs = d["case"]["segs"], d["offs"]
    masks = np.concatenate([synth.make_masks(S, Hm, Wm, seed=300 + b, hmin=4, hmax=max(Hm // 2, 5), wmin=4, wmax=max(Wm // 2, 5))
                            for b, S in enumerate(segs)]).astype(np.uint8)
    eng = _engine(d["C"], T.pca_model(name))

    def restated(bits, adj):
        inc = O.unpack_bits_u64(bits.cpu().numpy().view(np.uint64), d["N"])
        adj = adj.cpu().numpy()
        descs, pos = [], 0
        for b in range(T.B):
            n = int(offs[b + 1] - offs[b])
            descs.append(BR.burst_vlad(d["toks"][b], d["C"], inc[offs[b]:offs[b + 1]], adj[pos:pos + n * n].reshape(n, n).astype(bool), assign,
                                       MAIN)["out"])
            pos += n * n
        desc = np.concatenate(descs)
        return desc, O.normalize_feat(O.pca_transform(desc, *T.pca_model(name), True))

    try:
        _set(eng, assign, MAIN)
        masks_d, tok_d = torch.from_numpy(masks).cuda(), torch.from_numpy(d["tok"]).cuda()
        r = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True, l2norm=True, want_desc=True)
        desc, y = restated(r["bits"], r["adj"])
        _check_y(f"{name} describe", r["out"].cpu().numpy(), y)
        err, cos_err = _row_errors(r["desc"].cpu().numpy(), desc)
        print(f"{name} describe desc: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
        assert err < DESC_TOL + 4 * BR.e_u(name, True, assign, MAIN) and cos_err < COS_TOL
        raw = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=False)
        assert torch.equal(raw["out"], r["desc"])                      # the same kernels: the same bytes
        hnd = eng.describe_begin(masks_d, tok_d, offs, H, W, 14, 2, pca=True)
        eng.describe_flags(hnd)
        e = eng.describe_end(hnd, l2norm=True, want_desc=True)
        assert torch.equal(e["out"], r["out"]) and torch.equal(e["desc"], r["desc"])
        eng.set_vlad_burst(None)
        plain = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=False)
        assert float((plain["out"] - raw["out"]).abs().max()) > 1e-4    # (the option changed the answer)
        eng.set_vlad_burst(MAIN)
        eng.set_option("pca_path", "project")
        for call in (lambda: eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True),
                     lambda: eng.describe_begin(masks_d, tok_d, offs, H, W, 14, 2, pca=True)):
            with pytest.raises(SegVLADError) as ei:
                call()
            assert ei.value.code == SEGVLAD_ERR_LIMIT and "vlad_burst" in str(ei.value), ei.value
        eng.set_option("pca_path", "auto")
        again = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True, l2norm=True)
        assert torch.equal(again["out"], r["out"])
    finally:
        eng.close()


# ---- 6. an all-zero token -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D", T.EXTRA_SHAPES)
def test_zero_token_and_unnormalised_magnitudes(K, D):
    """x^ = 0 takes part with cosine 0 against every token, itself included; columns scaled over six decades count as their unit vectors"""
    d = T.zero_column_batch(K, D)
    us = [BR.burst_u_fp32(t, *MAIN) for t in d["toks"]]
    eng = _engine(d["C"])
    try:
        for assign in BR.ASSIGNS[:2]:
            _set(eng, assign, MAIN)
            r = _images(eng, d, True)
            ref = BR.batch(d["toks"], d["incs"], d["adjs"], d["C"], True, assign, MAIN)
            alt = BR.batch(d["toks"], d["incs"], d["adjs"], d["C"], True, assign, MAIN, us=us)
            eu = float(np.abs(alt["out"] - ref["out"]).max())
            assert np.isfinite(r["out"]).all() and np.isfinite(r["block_norms"]).all()
            _check(f"zero token K={K} D={D} {assign[0]}", r, ref, eu, BR.weight_rtol(D, MAIN, assign[1] or 0.0), None, None)
    finally:
        eng.close()


# ---- 7. off is off; the entries out of the option's reach ----------------------------------------------------------------------
def _launches(eng, d):
    from revisit_anything_amd._lib import SegVLADError

    eng.set_profiling(True)
    eng.profile_reset()
    eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"])
    eng.synchronize()
    n = {s: eng.stage_ms(s)[1] for s in ("assign", "prep", "aggregate")}
    try:
        n["burst"] = eng.stage_ms("burst")[1]
    except SegVLADError:       # a stage that has not run since the reset has no timer to read
        n["burst"] = 0
    eng.set_profiling(False)
    return n


def test_off_is_off():
    from oracle import segvlad_oracle as O

    name = "k33_d96_n129"
    d = T.build(name)
    K, D = d["K"], d["D"]
    fresh, eng = _engine(d["C"], T.pca_model(name)), _engine(d["C"], T.pca_model(name))
    xn = O.normalize_tokens_f32(d["toks"][0])
    labels, _ = O.assign_labels(xn, d["C"])
    res = (xn - d["C"][labels]).astype(np.float32)
    bits0 = d["bits"][d["offs"][0]:d["offs"][1]]

    def both(e):
        sums = torch.zeros((K, D), dtype=torch.float64, device="cuda")
        counts = torch.zeros(K, dtype=torch.int64, device="cuda")
        lab = e.kmeans_step(d["tok"], sums, counts, want_labels=True)
        ca = e.cluster_aggregate(K, res, labels.astype(np.uint8), bits0, d["adjs"][0].astype(np.uint8).reshape(-1))
        return {"sums": sums.cpu().numpy(), "counts": counts.cpu().numpy(), "labels": lab.cpu().numpy(), "ca": ca.cpu().numpy()}

    try:
        hard0 = _images(fresh, d, True)
        y0 = fresh.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy()
        n0, other0 = _launches(fresh, d), both(fresh)
        assert n0 == {"assign": 1, "prep": 1, "burst": 0, "aggregate": 1}, n0
        assert eng.vlad_burst == "off" and eng.set_vlad_burst(MAIN) == "off" and eng.vlad_burst == "8.0e+00:7.0e+00:1.0e+00"
        on = _images(eng, d, True)
        assert not _bits_equal(on["out"], hard0["out"])
        assert _bits_equal(on["labels"], hard0["labels"]) and _bits_equal(on["gap"], hard0["gap"])
        assert _launches(eng, d) == {"assign": 1, "prep": 1, "burst": 2, "aggregate": 2}
        other = both(eng)
        assert all(_bits_equal(other0[k], other[k]) for k in other0)           # kmeans_step and cluster_aggregate ignore the option
        assert eng.set_vlad_burst(None) == "8.0e+00:7.0e+00:1.0e+00" and eng.vlad_burst == "off"
        off = _images(eng, d, True)
        assert all(_bits_equal(hard0[k], off[k]) for k in hard0)
        assert _bits_equal(y0, eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy())
        assert _launches(eng, d) == n0
        # the same under soft assignment
        fresh.set_vlad_assign("soft", 10.0), eng.set_vlad_assign("soft", 10.0)
        soft0 = _images(fresh, d, True)
        eng.set_vlad_burst(MAIN)
        assert not _bits_equal(_images(eng, d, True)["out"], soft0["out"])
        eng.set_option("vlad_burst", "off")
        assert all(_bits_equal(soft0[k], v) for k, v in _images(eng, d, True).items())
    finally:
        fresh.close(), eng.close()


# ---- 8. the option's parser ---------------------------------------------------------------------------------------------------
REFUSED = ("8:7", "8:7:1:0", "8:7:x", "nan:7:1", "-1:7:1", "65:7:1", "8:-9:1", "8:17:1", "8:7:2.5", "8:7:1 ", "Off", "",
           "8::1", ":7:1", "8:7:", "inf:7:1", "8:7:-0.5", "8:7:0x1", " 8:7:1", "8,7,1", "on", "OFF", "8:7:1e")
ACCEPTED = ("8:7:1", "0:-8:0", "64:16:2", "8.0e+00:7.0e+00:1.0e+00", ".5:-.5:.5", "2:0:0.5")


def test_refusals_leave_the_value_in_force():
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    name = "k2_d36_n65"
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        plain = _images(eng, d, True)
        eng.set_vlad_burst(MAIN)
        on = _images(eng, d, True)
        assert not _bits_equal(on["out"], plain["out"])
        for value in REFUSED:
            with pytest.raises(SegVLADError) as ei:
                eng.set_option("vlad_burst", value)
            assert ei.value.code == SEGVLAD_ERR_ARG, (value, ei.value)
            assert eng.vlad_burst == "8.0e+00:7.0e+00:1.0e+00"
        assert all(_bits_equal(on[k], v) for k, v in _images(eng, d, True).items())      # "left in force", by results
        eng.set_vlad_burst(None)
        for value in REFUSED[:4]:
            with pytest.raises(SegVLADError):
                eng.set_option("vlad_burst", value)
        assert all(_bits_equal(plain[k], v) for k, v in _images(eng, d, True).items())   # a refusal under off leaves off
        for value in ACCEPTED:
            eng.set_option("vlad_burst", value)
            assert eng.vlad_burst == value
        eng.set_option("vlad_burst", "8.0e+00:7.0e+00:1.0e+00")
        assert all(_bits_equal(on[k], v) for k, v in _images(eng, d, True).items())
    finally:
        eng.close()


def test_the_pipeline_sets_the_option():
    from revisit_anything_amd.pipeline import SegVLADPipeline

    d = T.build("k2_d36_n65")
    eng = _engine(d["C"])
    try:
        SegVLADPipeline(eng, 112, 140, use_pca=False)
        assert eng.vlad_burst == "off"
        SegVLADPipeline(eng, 112, 140, use_pca=False, vlad_burst=MAIN)
        assert eng.vlad_burst == "8.0e+00:7.0e+00:1.0e+00"
        with pytest.raises(ValueError):
            SegVLADPipeline(eng, 112, 140, use_pca=False, vlad_burst=(8, 7, 3))
        assert eng.vlad_burst == "8.0e+00:7.0e+00:1.0e+00"
    finally:
        eng.close()
