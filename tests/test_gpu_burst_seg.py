"""Burst discount over a segment's own tokens on the device (options vlad_burst=<a>:<b>:<p> with vlad_burst_scope=segment,
include/segvlad.h) against its fp64 restatement (tests/burst_seg_ref.py) over the soft kernels' shape table.

Bounds (tests/test_gpu_burst.py's, with E_u recomputed for the per-segment sums):
  descriptor   max |out - ref| < 1e-6 + 4 e_u_seg and 1 - cos < 1e-6 per row, e_u_seg = the move of the fp64 descriptor when its u is
               replaced by the sequential-fp32 restatement's (tests/test_burst_seg_cases.py holds 4 e_u_seg <= 1e-6);
               block norms rtol = 1e-5 + 2 (p a + T) sqrt(D) 2^-24, atol 1e-6; zero rows equal
  projected    3e-5 of max |ref| (tests/test_gpu_soft_vlad.py's PCA_RTOL)
Launches under segment scope, as built: "burst" 1 (the Gram kernel writes the weights itself), "aggregate" 2 (the masked aggregation
and the finalize; + 1 for soft_pooled's mean centre), "assign" 1 under hard assignment and 2 under soft.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import burst_ref as BR
import burst_seg_ref as BS
import describe_shape_cases as T
import soft_vlad_ref as SR

pytestmark = pytest.mark.gpu

DESC_TOL, COS_TOL, PCA_RTOL = 1e-6, 1e-6, 3e-5
MAIN = BS.PARAMS[0]
MAIN_VALUE = "8.0e+00:7.0e+00:1.0e+00"
HARD, SOFT = BS.ASSIGNS[0], BS.ASSIGNS[1]


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


def _call(eng, tok, bits, offs, adj):
    return _np(eng.seg_vlad(tok, bits, offs, adj, want_labels=True, want_gap=True, want_block_norms=True))


def _images(eng, d, with_adj):
    return _call(eng, d["tok"], d["bits"], d["offs"], d["adj"] if with_adj else None)


def _row_errors(out, ref):
    err = float(np.abs(out - ref).max()) if out.size else 0.0
    nz = np.sqrt((ref * ref).sum(1)) > 0
    o = out[nz].astype(np.float64)
    cos = (o * ref[nz]).sum(1) / (np.sqrt((o * o).sum(1)) * np.sqrt((ref[nz] * ref[nz]).sum(1)))
    return err, float((1.0 - cos).max()) if nz.any() else 0.0


def _set(eng, assign, params, scope="segment"):
    eng.set_vlad_assign(*assign)       # ("hard", None) | ("soft", T) | ("soft_pooled", T)
    eng.set_vlad_burst(params)
    eng.set_vlad_burst_scope(scope)


def _check(tag, r, ref, eu, bn_rtol, hard=None):
    err, cos_err = _row_errors(r["out"], ref["out"])
    print(f"{tag}: max|out-ref| {err:.3e} (bound {DESC_TOL + 4 * eu:.3e}, e_u_seg {eu:.3e}), max 1-cos {cos_err:.3e}, "
          f"block norms need rtol {SR.needed_rtol(r['block_norms'], ref['block_norms']):.3e} (bound {bn_rtol:.3e})")
    assert r["out"].shape == ref["out"].shape and np.isfinite(r["out"]).all() and err < DESC_TOL + 4 * eu, tag
    assert cos_err < COS_TOL, tag
    assert np.allclose(r["block_norms"], ref["block_norms"], rtol=bn_rtol, atol=1e-6), tag
    if hard is not None:       # the audit outputs stay the hard arg-max and gap
        assert _bits_equal(r["labels"], hard["labels"]) and _bits_equal(r["gap"], hard["gap"]), tag
    assert np.all(r["out"][ref["zero_rows"]] == 0) and np.all(r["block_norms"][ref["zero_rows"]] == 0), tag


# ---- 1. against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_adj", (True, False), ids=("adj", "noadj"))
@pytest.mark.parametrize("name", BS.CASES)
def test_shape_table_against_the_restatement(name, with_adj):
    d = T.build(name)
    offs = d["offs"]
    eng = _engine(d["C"])
    try:
        hard = _images(eng, d, with_adj)
        for params in BS.PARAMS:
            for assign in BS.ASSIGNS:
                _set(eng, assign, params)
                r = _images(eng, d, with_adj)
                ref = BS.reference(name, with_adj, assign, params)
                assert ref["zero_rows"].any()
                _check(f"{name} adj={int(with_adj)} {assign[0]} {params}", r, ref, BS.e_u_seg(name, assign, params, with_adj),
                       BR.weight_rtol(d["D"], params, assign[1] or 0.0), hard)
                for key in ("out", "block_norms"):      # image 3 is image 0
                    assert _bits_equal(r[key][offs[0]:offs[1]], r[key][offs[3]:offs[4]]), (name, assign, params, key)
    finally:
        eng.close()


# ---- 2. a = 0: a constant discount per segment cancels in the normalisations ------------------------------------------------------
@pytest.mark.parametrize("name", BS.CASES)
def test_a_constant_discount_is_the_plain_hard_descriptor(name):
    """0:7:1: g[s][n] = |U(s)| sigmoid(7) on U(s).  A mask product or a tile edge that drops or double-counts one token moves a block
    norm by 1 / |U(s)| at the least, orders of magnitude above rtol 1e-5 (the atol is the hard path's 1e-6 times the same constant)."""
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        _set(eng, HARD, (0.0, 7.0, 1.0))
        for with_adj in (True, False):
            ref = T.reference(name, with_adj)
            size = BS.union_sizes(name, with_adj).astype(np.float64)
            c = np.where(size > 0, 1.0 / (np.maximum(size, 1.0) / (1.0 + np.exp(-7.0))), 0.0)[:, None]
            r = _images(eng, d, with_adj)
            err, cos_err = _row_errors(r["out"], ref["out"])
            want = ref["block_norms"] * c
            dev = np.abs(r["block_norms"] - want) - 1e-6 * c
            on = want > 0
            bn_rel = float(max(0.0, (dev[on] / want[on]).max()))
            print(f"{name} adj={int(with_adj)} 0:7:1: max|out-hard| {err:.3e}, max 1-cos {cos_err:.3e}, block norms need rtol {bn_rel:.3e} "
                  f"(bound 1e-5); |U(s)| from {int(size[size > 0].min())} to {int(size.max())}")
            assert err < DESC_TOL and cos_err < COS_TOL
            assert np.all(np.abs(r["block_norms"] - want) <= 1e-6 * c + 1e-5 * want)
    finally:
        eng.close()


# ---- 3. one all-token segment per image, order 0: the image scope ----------------------------------------------------------------
@pytest.mark.parametrize("name", BS.CASES)
def test_one_all_token_segment_is_the_image_scope(name):
    d = T.build(name)
    incs = [np.ones((1, d["N"]), dtype=bool)] * 3
    tok, bits, offs, _ = T.pack_batch(d["toks"][:3], incs, [np.ones((1, 1), np.uint8)] * 3)
    us = BR.case_u_fp32(name, MAIN)
    eng = _engine(d["C"])
    try:
        for assign in BS.ASSIGNS:
            ref = BR.batch(d["toks"][:3], incs, [None] * 3, d["C"], False, assign, MAIN)
            alt = BR.batch(d["toks"][:3], incs, [None] * 3, d["C"], False, assign, MAIN, us=us[:3])
            eu = float(np.abs(alt["out"] - ref["out"]).max())
            _set(eng, assign, MAIN, "image")
            img = _call(eng, tok, bits, offs, None)
            _set(eng, assign, MAIN, "segment")
            seg = _call(eng, tok, bits, offs, None)
            err, cos_err = _row_errors(seg["out"], img["out"].astype(np.float64))
            bn_rtol = BR.weight_rtol(d["D"], MAIN, assign[1] or 0.0)
            print(f"{name} {assign[0]}: max|segment - image| {err:.3e} (bound {DESC_TOL + 4 * eu:.3e}), max 1-cos {cos_err:.3e}, block norms "
                  f"need rtol {SR.needed_rtol(seg['block_norms'], img['block_norms'].astype(np.float64)):.3e} (bound {bn_rtol:.3e})")
            assert err < DESC_TOL + 4 * eu and cos_err < COS_TOL
            assert np.allclose(seg["block_norms"], img["block_norms"], rtol=bn_rtol, atol=1e-6)
            _check(f"{name} {assign[0]} all-token vs fp64", seg, dict(ref, zero_rows=np.zeros(3, bool)), eu, bn_rtol)
    finally:
        eng.close()


# ---- 4. p = 0: u is exactly 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k2_d36_n65", "k33_d96_n129", "k65_d200_n333", "k128_d64_n513_s129"))
def test_p_zero_is_no_discount(name):
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        for assign in (HARD, SOFT):
            _set(eng, assign, None)
            off = _images(eng, d, True)
            _set(eng, assign, (8.0, 7.0, 0.0))
            r = _images(eng, d, True)
            err, cos_err = _row_errors(r["out"], off["out"].astype(np.float64))
            print(f"{name} {assign[0]} 8:7:0: max|out-off| {err:.3e}, max 1-cos {cos_err:.3e}")
            assert err < DESC_TOL and cos_err < COS_TOL
            assert np.allclose(r["block_norms"], off["block_norms"], rtol=1e-5, atol=1e-6)
    finally:
        eng.close()


# ---- 5. independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k33_d96_n129", "k128_d64_n513_s129"))
def test_rows_depend_on_the_image_and_the_segment_alone(name):
    d = T.build(name)
    offs = d["offs"]
    eng = _engine(d["C"])
    try:
        for assign in (HARD, SOFT):
            _set(eng, assign, MAIN)
            full = _images(eng, d, True)
            again = _images(eng, d, True)
            assert all(_bits_equal(full[k], again[k]) for k in full), (name, assign)           # two calls: the same bytes
            for b in (0, 2):      # a B = 1 call
                tok, bits, o1, adj = T.pack_batch([d["toks"][b]], [d["incs"][b]], [d["adjs"][b]])
                one = _call(eng, tok, bits, o1, adj)
                for key in ("out", "block_norms"):
                    assert _bits_equal(one[key], full[key][offs[b]:offs[b + 1]]), (name, assign, b, key)
            # identity adjacency: a segment's rows with and without the other segments of its image
            b, S = 2, int(offs[3] - offs[2])
            tok, bits, o1, _ = T.pack_batch([d["toks"][b]], [d["incs"][b]], [np.eye(S, dtype=np.uint8)])
            alone_all = _call(eng, tok, bits, o1, None)
            for s in sorted({0, 2, 33, S - 1}):
                tok, bits, o1, _ = T.pack_batch([d["toks"][b]], [d["incs"][b][s:s + 1]], [np.ones((1, 1), np.uint8)])
                alone = _call(eng, tok, bits, o1, None)
                for key in ("out", "block_norms"):
                    assert _bits_equal(alone[key][0], alone_all[key][s]), (name, assign, s, key)
    finally:
        eng.close()


def test_a_batch_of_eleven_images():
    """B >= 8: the Gram kernel deals its workgroups so that an image's tiles share an XCD (grid padded to a multiple of 8 images; 11
    is none).  Every image's rows are the bytes it has in the table's batch of 4."""
    name, order = "k33_d96_n129", (0, 2, 1, 0, 2, 2, 0, 1, 2, 0, 2)
    d = T.build(name)
    toks, incs, adjs = [d["toks"][b] for b in order], [d["incs"][b] for b in order], [d["adjs"][b] for b in order]
    tok, bits, offs, adj = T.pack_batch(toks, incs, adjs)
    eng = _engine(d["C"])
    try:
        for assign in (HARD, SOFT):
            _set(eng, assign, MAIN)
            r = _call(eng, tok, bits, offs, adj)
            four = _images(eng, d, True)
            for j, b in enumerate(order):
                for key in ("out", "block_norms"):
                    assert _bits_equal(r[key][offs[j]:offs[j + 1]], four[key][d["offs"][b]:d["offs"][b + 1]]), (assign, j, key)
    finally:
        eng.close()


# ---- 6. the other entries -----------------------------------------------------------------------------------------------------
def _check_y(tag, y, ref):
    err, bound = float(np.abs(y - ref).max()), PCA_RTOL * float(np.abs(ref).max())
    print(f"{tag}: max|y-ref| {err:.3e} (bound {bound:.3e})")
    assert y.shape == ref.shape and err <= bound, tag


@pytest.mark.parametrize("assign", (HARD, SOFT), ids=("hard", "soft10"))
@pytest.mark.parametrize("name", SR.PCA_CASES)
def test_images_pca_takes_the_planes_form_and_refuses_project(name, assign):
    from oracle import segvlad_oracle as O
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d = T.build(name)
    eng = _engine(d["C"], T.pca_model(name))
    try:
        _set(eng, assign, MAIN)
        desc = BS.reference(name, True, assign, MAIN)["out"]
        for l2norm in (True, False):
            y = O.pca_transform(desc, *T.pca_model(name), True)
            ref = O.normalize_feat(y) if l2norm else y
            got = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm)["out"].cpu().numpy()
            _check_y(f"{name} {assign[0]} images_pca l2norm={int(l2norm)}", got, ref)
            r = _np(eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm, want_desc=True))
            _check_y(f"{name} {assign[0]} images_pca + desc l2norm={int(l2norm)}", r["out"], ref)
            err, cos_err = _row_errors(r["desc"], desc)
            print(f"{name} {assign[0]} images_pca desc_out: max|desc-ref| {err:.3e}, max 1-cos {cos_err:.3e}")
            assert err < DESC_TOL + 4 * BS.e_u_seg(name, assign, MAIN, True) and cos_err < COS_TOL
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

    d, assign = T.build(name), HARD
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
        descs, alts, pos = [], [], 0
        for b in range(T.B):
            n = int(offs[b + 1] - offs[b])
            inc_b, adj_b = inc[offs[b]:offs[b + 1]], adj[pos:pos + n * n].reshape(n, n).astype(bool)
            descs.append(BS.seg_vlad(d["toks"][b], d["C"], inc_b, adj_b, assign, MAIN)["out"])
            u32 = BS.burst_seg_u_fp32(BS._sigmoid_fp32(name, b % 3, MAIN), inc_b, adj_b, MAIN[2])
            alts.append(BS.seg_vlad(d["toks"][b], d["C"], inc_b, adj_b, assign, MAIN, u=u32)["out"])
            pos += n * n
        desc = np.concatenate(descs)
        return desc, O.normalize_feat(O.pca_transform(desc, *T.pca_model(name), True)), float(np.abs(np.concatenate(alts) - desc).max())

    try:
        _set(eng, assign, MAIN)
        masks_d, tok_d = torch.from_numpy(masks).cuda(), torch.from_numpy(d["tok"]).cuda()
        r = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=True, l2norm=True, want_desc=True)
        desc, y, eu = restated(r["bits"], r["adj"])
        _check_y(f"{name} describe", r["out"].cpu().numpy(), y)
        err, cos_err = _row_errors(r["desc"].cpu().numpy(), desc)
        print(f"{name} describe desc: max|desc-ref| {err:.3e} (bound {DESC_TOL + 4 * eu:.3e}), max 1-cos {cos_err:.3e}")
        assert err < DESC_TOL + 4 * eu and cos_err < COS_TOL
        raw = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=False)
        assert torch.equal(raw["out"], r["desc"])                      # the same kernels: the same bytes
        hnd = eng.describe_begin(masks_d, tok_d, offs, H, W, 14, 2, pca=True)
        eng.describe_flags(hnd)
        e = eng.describe_end(hnd, l2norm=True, want_desc=True)
        assert torch.equal(e["out"], r["out"]) and torch.equal(e["desc"], r["desc"])
        eng.set_vlad_burst_scope("image")
        image = eng.describe(masks_d, tok_d, offs, H, W, 14, 2, pca=False)
        assert float((image["out"] - raw["out"]).abs().max()) > 1e-4    # (the option changed the answer)
        eng.set_vlad_burst_scope("segment")
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
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

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
        # vlad_burst=off: the scope is stored and changes nothing
        assert eng.vlad_burst_scope == "image" and eng.set_vlad_burst_scope("segment") == "image" and eng.vlad_burst_scope == "segment"
        off = _images(eng, d, True)
        assert all(_bits_equal(hard0[k], off[k]) for k in hard0)
        assert _bits_equal(y0, eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"])["out"].cpu().numpy())
        assert _launches(eng, d) == n0
        # a junk value is refused and leaves the scope as it was
        for junk in ("Segment", "", "seg", "segment ", "image,segment", "1"):
            with pytest.raises(SegVLADError) as ei:
                eng.set_option("vlad_burst_scope", junk)
            assert ei.value.code == SEGVLAD_ERR_ARG and eng.vlad_burst_scope == "segment", (junk, ei.value)
        # on: segment + hard
        eng.set_vlad_burst(MAIN)
        seg = _images(eng, d, True)
        assert not _bits_equal(seg["out"], hard0["out"])
        assert _bits_equal(seg["labels"], hard0["labels"]) and _bits_equal(seg["gap"], hard0["gap"])
        assert _launches(eng, d) == {"assign": 1, "prep": 1, "burst": 1, "aggregate": 2}
        other = both(eng)
        assert all(_bits_equal(other0[k], other[k]) for k in other0)           # kmeans_step and cluster_aggregate ignore the options
        eng.set_vlad_assign("soft", 10.0)
        assert _launches(eng, d) == {"assign": 2, "prep": 1, "burst": 1, "aggregate": 2}
        eng.set_vlad_assign("soft_pooled", 10.0)
        assert _launches(eng, d) == {"assign": 2, "prep": 1, "burst": 1, "aggregate": 3}
        eng.set_vlad_assign("hard")
        # the image scope after a round trip through segment: its launches and its bytes
        fresh.set_vlad_burst(MAIN)
        img0 = _images(fresh, d, True)
        assert eng.set_vlad_burst_scope("image") == "segment"
        img = _images(eng, d, True)
        assert all(_bits_equal(img0[k], img[k]) for k in img0) and not _bits_equal(img["out"], seg["out"])
        assert _launches(eng, d) == {"assign": 1, "prep": 1, "burst": 2, "aggregate": 2}
        eng.set_vlad_burst_scope("segment")
        assert all(_bits_equal(seg[k], v) for k, v in _images(eng, d, True).items())
        eng.set_vlad_burst(None)
        assert all(_bits_equal(hard0[k], v) for k, v in _images(eng, d, True).items()) and _launches(eng, d) == n0
    finally:
        fresh.close(), eng.close()


def test_the_weights_buffer_is_fenced():
    """Segment scope keeps its weights in a scratch buffer of its own, s_bseg [B][N][64 SC] fp32, an entry of the context's buffer list:
    the guard fences it at the request's size (every call of this file runs under those fences), and with its back fence put 4 bytes
    early a correct call lands in it and names the buffer.  (Under segment + hard reserve_scratch asks for neither s_softw nor s_burst;
    a call's scratch cannot be read from outside, what shows is the launch counts of test_off_is_off.)"""
    from revisit_anything_amd._lib import SEGVLAD_ERR_STATE, SegVLADError

    d = T.build("k33_d96_n129")
    eng = _engine(d["C"])
    try:
        _set(eng, HARD, MAIN, "segment")
        _images(eng, d, True)
        eng.synchronize()                          # quiet at the exact size
        eng.set_option("guard_undersize", "s_bseg:4")
        with pytest.raises(SegVLADError) as ei:
            _images(eng, d, True)
        assert ei.value.code == SEGVLAD_ERR_STATE and "guard" in str(ei.value) and "s_bseg" in str(ei.value), ei.value
    finally:
        eng.close()


def test_the_pipeline_sets_the_option():
    from revisit_anything_amd.pipeline import SegVLADPipeline

    d = T.build("k2_d36_n65")
    eng = _engine(d["C"])
    try:
        SegVLADPipeline(eng, 112, 140, use_pca=False)
        assert eng.vlad_burst_scope == "image"
        SegVLADPipeline(eng, 112, 140, use_pca=False, vlad_burst=MAIN, vlad_burst_scope="segment")
        assert eng.vlad_burst == MAIN_VALUE and eng.vlad_burst_scope == "segment"
        with pytest.raises(ValueError):
            SegVLADPipeline(eng, 112, 140, use_pca=False, vlad_burst_scope="both")
        assert eng.vlad_burst_scope == "segment"
    finally:
        eng.close()
