"""The describe stage against the fp64 oracle over the shape table of tests/describe_shape_cases.py: every case reaches a
branch that the launchers take from (K, D, N, S) alone -- narrow / wide assignment and their padded centres, partial 128-column
slabs and the last workgroup of the aggregation, staged / non-staged neighbour union, the words of segment columns, the forms
of the fused projection, the task-size classes of the project form's token kernels.  tests/test_describe_shape_cases.py has
shown with the oracle alone that no case holds a near-tie (gap >= 1e-4) or a tiny block (norm >= 1e-2), so nothing is left
out of a comparison here.

Bounds (none of them new):
  descriptor form   labels equal; gap within 2e-6; max |out - ref| < 2e-6; block norms rtol 1e-5, atol 1e-6; rows of segments
                    without a token in their neighbourhood exactly 0 -- what tests/test_gpu_parity.py holds this form to
  projected forms   3e-5 of max |ref| against oracle.pca_transform (+ normalize_feat) of the oracle's descriptor -- the bound of
                    test_images_pca_fused_equals_two_calls_and_oracle and tests/test_gpu_cover_rows.py against the same oracle
Every figure is printed before it is asserted.

Measured on an MI355X (max over both adjacency settings; pairs are "with l2norm, without"; |out| and gap are held to 2e-6):
  case                     |out|    gap      bound            planes           fp32             project          plain (K D % 32 != 0)
  k1_d32_n130              1.5e-07  0.0e+00  2.5e-05 1.1e-02  4.4e-07 9.5e-05  3.2e-07 7.2e-05  2.2e-07 6.1e-05  -
  k2_d36_n65               1.8e-07  2.4e-07  2.5e-05 7.2e-03  -                -                -                3.4e-07 8.3e-05
  k5_d36_n200              6.2e-08  3.2e-07  2.3e-05 4.3e-03  -                -                -                3.3e-07 8.0e-05
  k8_d36_n99               7.0e-08  2.8e-07  2.4e-05 4.7e-03  2.7e-07 3.5e-05  1.8e-07 2.8e-05  -                -
  k31_d64_n257             1.8e-08  3.4e-07  2.5e-05 1.9e-03  2.0e-07 1.3e-05  5.2e-07 1.6e-05  2.1e-07 8.5e-06  -
  k33_d96_n129             2.4e-08  3.0e-07  2.3e-05 1.2e-03  3.1e-07 1.5e-05  4.4e-07 1.6e-05  2.9e-07 1.1e-05  -
  k64_d160_n300            1.0e-08  3.6e-07  2.6e-05 6.3e-04  3.3e-07 7.3e-06  9.4e-07 1.4e-05  3.3e-07 7.4e-06  -
  k65_d200_n333            8.6e-09  1.6e-07  2.5e-05 5.8e-04  -                -                -                8.4e-07 1.2e-05
  k97_d384_n260            7.2e-09  1.5e-07  2.5e-05 4.5e-04  7.5e-07 8.6e-06  1.3e-06 1.1e-05  5.1e-07 7.1e-06  -
  k128_d64_n513_s129       1.2e-08  3.5e-07  2.4e-05 1.1e-03  2.7e-07 6.4e-06  4.2e-07 1.0e-05  3.2e-07 7.7e-06  -
  k128_d1536_n130          5.7e-09  3.7e-07  2.1e-05 1.5e-04  1.1e-06 6.4e-06  1.6e-06 1.3e-05  5.5e-07 3.3e-06  -
  k32_d32_n1530_s400       7.6e-08  3.5e-07  2.4e-05 2.4e-03  2.4e-07 1.9e-05  3.2e-07 2.4e-05  2.4e-07 1.7e-05  -
  cls_le32_k32_d96_n99     1.9e-08  2.9e-07  2.5e-05 1.4e-03  2.2e-07 1.1e-05  5.0e-07 1.5e-05  2.3e-07 9.1e-06  -
  cls_33to64_k3_d96_n99    6.8e-08  3.2e-07  2.5e-05 4.7e-03  1.6e-07 3.5e-05  1.7e-07 3.1e-05  1.5e-07 2.5e-05  -
  cls_65to255_k2_d96_n130  1.0e-07  5.0e-07  2.1e-05 3.2e-03  2.6e-07 4.2e-05  4.7e-07 8.0e-05  2.1e-07 2.6e-05  -
  cls_ge256_k2_d96_n300    1.2e-07  4.2e-07  2.0e-05 2.4e-03  3.9e-07 4.3e-05  3.9e-07 5.3e-05  8.8e-08 2.2e-05  -
  (project with tnk_gram=0 on the two Gram-sized classes: 2.3e-07 8.7e-06 and 1.5e-07 2.5e-05; assign_narrow=1, the negative-score
  and the zero-token batches: |out| <= 1.3e-07, gap <= 3.6e-07)"""
import numpy as np
import pytest
import torch

import describe_shape_cases as T

pytestmark = pytest.mark.gpu

DESC_TOL, GAP_TOL, PCA_RTOL = 2e-6, 2e-6, 3e-5


def _oracle():
    from oracle import segvlad_oracle as O

    return O


def _engine(C, pca=None):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    eng.set_vocab(C)
    if pca is not None:
        eng.pca_set(*pca, whiten=True)
    return eng


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_descriptor(tag, r, ref, K, zero_row=True):
    """One descriptor-form result (labels, gap, out, block_norms as NumPy) against the oracle's, every token and every block"""
    lab = r["labels"]
    assert lab.dtype == np.uint8 and lab.max() < K, tag
    n_bad = int((lab != ref["labels"]).sum())
    finite = np.isfinite(ref["gap"])
    gap_err = float(np.abs(r["gap"][finite] - ref["gap"][finite]).max()) if finite.any() else 0.0
    err = float(np.abs(r["out"] - ref["out"]).max())
    bn_err = float(np.abs(r["block_norms"] - ref["block_norms"]).max())
    print(f"{tag}: labels differing {n_bad}, gap err {gap_err:.3e} (bound {GAP_TOL:.0e}), max|out-ref| {err:.3e} (bound {DESC_TOL:.0e}), "
          f"block-norm err {bn_err:.3e}")
    assert n_bad == 0, tag
    assert np.array_equal(np.isposinf(r["gap"]), ~finite), tag       # K = 1: +inf, like the oracle
    assert gap_err <= GAP_TOL, tag
    assert r["out"].shape == ref["out"].shape and err < DESC_TOL, tag
    assert np.allclose(r["block_norms"], ref["block_norms"], rtol=1e-5, atol=1e-6), tag
    assert (ref["zero_rows"].any() or not zero_row) and np.all(r["out"][ref["zero_rows"]] == 0), tag


def _check_twin_image(tag, offs, N, **arrays):
    """Image 3 is image 0: bit-equal rows, whatever the batch position"""
    s0, s3 = slice(offs[0], offs[1]), slice(offs[3], offs[4])
    for key, a in arrays.items():
        per_image = a.shape[0] == T.B and a.ndim == 2 and a.shape[1] == N
        x, y = (a[0], a[3]) if per_image else (a[s0], a[s3])
        assert _bits_equal(x, y), (tag, key)


def _pca_ref(name, l2norm):
    O = _oracle()
    ref = O.pca_transform(T.reference(name, True)["out"], *T.pca_model(name), True)
    return O.normalize_feat(ref) if l2norm else ref


@pytest.mark.parametrize("name", T.NAMES)
def test_descriptor_form_against_the_oracle(name):
    d = T.build(name)
    facts = T.launch_facts(d["case"])
    assert all(facts[key] == want for key, want in d["case"]["expect"].items() if key in facts), name     # the branch it is named for
    if not facts["staged"]:        # the non-staged neighbour union: too large to stage beside the rest, small enough to run
        assert facts["prep_lds_staged"] > 150 * 1024 and facts["prep_lds"] < 160 * 1024
    eng = _engine(d["C"])
    try:
        for with_adj in (True, False):
            r = _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"] if with_adj else None, want_labels=True, want_gap=True,
                                 want_block_norms=True))
            tag = f"{name} descriptor adj={int(with_adj)}"
            _check_descriptor(tag, r, T.reference(name, with_adj), d["K"])
            _check_twin_image(tag, d["offs"], d["N"], **r)
            if "task_class" in d["case"]["expect"]:      # the label histogram lands in the class the case is named for
                lo, hi = T.TASK_CLASSES[d["case"]["expect"]["task_class"]]
                cnt = T.task_sizes(r["labels"], d["K"])
                assert cnt[cnt > 0].min() >= lo and cnt.max() <= hi, (name, cnt.min(), cnt.max())
            if "top_label" in d["case"]["expect"]:
                assert r["labels"].max() == d["case"]["expect"]["top_label"]
    finally:
        eng.close()


def _pca_forms(case):
    """(name, {option: (value, value afterwards)}) of every projected form the shape admits"""
    facts = T.launch_facts(case)
    if not facts["x3"]:
        return [("fallback", {})]          # K D % 32 != 0: no planes -- the call takes the plain projection by itself
    forms = [("planes", {"pca_path": ("planes", "auto")}), ("fp32", {"pca_arith": ("fp32", "auto")})]
    if facts["project"]:
        forms.append(("project", {"pca_path": ("project", "auto")}))
        if case["expect"].get("task_class") in ("le32", "33to64"):     # tasks the Gram kernels take: also through the block sums
            forms.append(("project tnk_gram=0", {"pca_path": ("project", "auto"), "tnk_gram": (0, 1)}))
    return forms


@pytest.mark.parametrize("name", T.NAMES)
def test_projected_forms_against_the_oracle(name):
    d = T.build(name)
    eng = _engine(d["C"], T.pca_model(name))
    try:
        for form, opts in _pca_forms(d["case"]):
            for key, (value, _) in opts.items():
                eng.set_option(key, value)
            for l2norm in (True, False):
                y = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=l2norm)["out"].cpu().numpy()
                ref = _pca_ref(name, l2norm)
                err, bound = float(np.abs(y - ref).max()), PCA_RTOL * float(np.abs(ref).max())
                tag = f"{name} {form} l2norm={int(l2norm)}"
                print(f"{tag}: max|y-ref| {err:.3e} (bound {bound:.3e})")
                assert y.shape == ref.shape == (int(d["offs"][-1]), T.P) and err <= bound, tag
                _check_twin_image(tag, d["offs"], d["N"], y=y)
            for key, (_, after) in opts.items():
                eng.set_option(key, after)
    finally:
        eng.close()


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if c["D"] % 32 == 0])
def test_fused_entry_equals_the_separate_calls_bit_for_bit(name):
    """segvlad_describe from masks at the case's (K, D, N) and segment counts: the kernels of the separate entry points, so their bits"""
    from revisit_anything_amd import synth

    d = T.build(name)
    h, w = T.image_grid(d["N"])
    H, W = 14 * h, 14 * w
    Hm, Wm = (H // 2 if h >= 4 else 2 * H), W // 2          # (a grid of one or three token rows: masks finer than the image)
    segs = d["case"]["segs"]
    masks = np.concatenate([synth.make_masks(S, Hm, Wm, seed=300 + b, hmin=4, hmax=max(Hm // 2, 5), wmin=4, wmax=max(Wm // 2, 5))
                            for b, S in enumerate(segs)]).astype(np.uint8)
    eng = _engine(d["C"], T.pca_model(name))
    try:
        masks_d, tok_d = torch.from_numpy(masks).cuda(), torch.from_numpy(d["tok"]).cuda()
        for pca in (True, False):
            r = eng.describe(masks_d, tok_d, d["offs"], H, W, 14, 2, pca=pca, l2norm=True)
            bits, cent = eng.incidence_centroids(masks_d, H, W, 14)
            adj, flags = eng.adjacency_flagged(cent, d["offs"], 2, device_flags=True)
            assert torch.equal(r["bits"], bits) and torch.equal(r["adj"], adj) and torch.equal(r["flags"], flags)
            sep = (eng.seg_vlad_pca(tok_d, bits, d["offs"], adj, l2norm=True) if pca else eng.seg_vlad(tok_d, bits, d["offs"], adj))["out"]
            assert r["out"].shape[0] == int(d["offs"][-1]) and torch.isfinite(sep).all()
            assert torch.equal(r["out"], sep), (name, pca)
    finally:
        eng.close()


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if T.launch_facts(c)["assign"].startswith("wide")])
def test_narrow_assignment_on_the_wide_kernels_shapes(name):
    """Option assign_narrow=1 on the cases that take assign_wide_kernel by default: assign_kernel<1> / <2> at D % 32 == 0"""
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        eng.set_option("assign_narrow", 1)
        r = _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"], want_labels=True, want_gap=True, want_block_norms=True))
        _check_descriptor(f"{name} descriptor assign_narrow=1", r, T.reference(name, True), d["K"])
    finally:
        eng.close()


# ---- inputs of another kind, at a padded K (33) and at K = 70 -----------------------------------------------------------------
@pytest.mark.parametrize("K,D", T.EXTRA_SHAPES)
def test_all_scores_negative_never_selects_a_padded_centre(K, D):
    """Every real centre scores below -0.05 (tests/test_describe_shape_cases.py), a padded all-zero centre scores exactly 0: a
    maximum taken over Kpad columns instead of K would pick it."""
    d = T.negative_scores_batch(K, D)
    ref = T.oracle_batch(d["toks"], d["incs"], d["adjs"], d["C"], True)
    eng = _engine(d["C"])
    try:
        for narrow in ((0, 1) if K <= 64 and D % 32 == 0 else (0,)):
            eng.set_option("assign_narrow", narrow)
            r = _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"], want_labels=True, want_gap=True, want_block_norms=True))
            _check_descriptor(f"negative scores K={K} D={D} assign_narrow={narrow}", r, ref, K, zero_row=False)
    finally:
        eng.close()


@pytest.mark.parametrize("K,D", T.EXTRA_SHAPES)
def test_zero_token_and_unnormalised_magnitudes(K, D):
    """An all-zero token takes label 0 (first maximum of K equal scores) and the residual -C[0] (x^ = 0 by max(norm, EPS)); columns
    scaled over six decades give the descriptor of their unit vectors."""
    d = T.zero_column_batch(K, D)
    ref = T.oracle_batch(d["toks"], d["incs"], d["adjs"], d["C"], True)
    eng = _engine(d["C"])
    try:
        r = _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"], want_labels=True, want_gap=True, want_block_norms=True))
        assert r["labels"][0, T.ZERO_TOKEN] == 0 and r["gap"][0, T.ZERO_TOKEN] == 0
        _check_descriptor(f"zero token K={K} D={D}", r, ref, K, zero_row=False)
    finally:
        eng.close()


def test_refusals_leave_the_context_usable():
    """K > 128 and D > 1536 are limits of the build (SEGVLAD_ERR_LIMIT), D % 4 != 0 is an argument error; after each refusal the
    same context describes a batch within the oracle's bound."""
    from revisit_anything_amd import synth
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_LIMIT, SegVLADError
    from revisit_anything_amd.engine import SegVLADEngine

    name = "k5_d36_n200"
    d, ref = T.build(name), T.reference(name, True)

    def describes_again(after):
        eng.set_vocab(d["C"])
        r = _np(eng.seg_vlad(d["tok"], d["bits"], d["offs"], d["adj"], want_labels=True, want_gap=True, want_block_norms=True))
        _check_descriptor(f"after {after}", r, ref, d["K"])
        eng.pca_set(*T.pca_model(name), whiten=True)
        y = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=False)["out"].cpu().numpy()
        assert np.abs(y - _pca_ref(name, False)).max() <= PCA_RTOL * np.abs(_pca_ref(name, False)).max(), after

    def refused(code, call):
        with pytest.raises(SegVLADError) as ei:
            call()
        assert ei.value.code == code, ei.value

    eng = SegVLADEngine(0)
    try:
        refused(SEGVLAD_ERR_LIMIT, lambda: eng.set_vocab(synth.make_vocab(129, 32, seed=1)))
        describes_again("set_vocab K=129")
        refused(SEGVLAD_ERR_ARG, lambda: eng.set_vocab(synth.make_vocab(8, 38, seed=2)))
        describes_again("set_vocab D=38")
        # K = 8, D = 1540: the vocabulary is taken (D % 4 == 0), the aggregation's 12-wave workgroup ends at D = 1536
        K, D, N = 8, 1540, 65
        C = synth.make_vocab(K, D, seed=3)
        tok = synth.make_tokens(C, N, seed=4, noise=0.02)[None]
        inc, adj = T.draw_segments(np.random.Generator(np.random.PCG64(5)), 5, N, 0.3, False)
        tok, bits, offs, adj = T.pack_batch([tok[0]], [inc], [adj])
        for fused in (False, True):
            eng.set_vocab(C)
            if fused:
                eng.pca_set(*synth.make_pca_model(K * D, T.P, seed=6), whiten=True)
                refused(SEGVLAD_ERR_LIMIT, lambda: eng.seg_vlad_pca(tok, bits, offs, adj))
            else:
                refused(SEGVLAD_ERR_LIMIT, lambda: eng.seg_vlad(tok, bits, offs, adj))
            describes_again("D=1540 " + ("images_pca" if fused else "images"))
    finally:
        eng.close()
