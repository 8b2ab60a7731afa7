"""segvlad_kmeans_step against an fp64 reference over the shape table of tests/kmeans_shape_cases.py: every case reaches a branch
that sv_launch_centroid_sums and centroid_sums_kernel (csrc/kmeans_kernels.hip) take from (K, D, N, B) alone -- CH = 256 / 128,
the 64 KiB + 1 KiB of LDS at K = 64 and K = 128, D below / at / past CH with a 4-column tail, a last round of 8 tokens with
padding lanes, one to three strided histogram rounds, one to three accumulating calls.  tests/test_kmeans_shape_cases.py has
shown with the oracle alone that no token holds a near-tie (gap >= 1e-4), so no token is left out here, and that each way in
which the kernel could be subtly wrong moves an entry by 10 times or more of the bound below.

Reference: from the fp32 tokens in fp64, x^ = x / ||x||, labels = the oracle's arg-max, sums[k] = sum of x^, counts = bincount.
Exact: labels, counts, the sums rows of empty clusters (0), a second pass doubles the counts, two runs give the same bits.

The bound on sums[k][c], read off the code (u = 2^-24):
  * centroid_sums_kernel: thread c walks the image's tokens in order, acc[label_t][c] += x[t][c] * rnorm[t].  The build's flags
    (-O3, no fast-math option: the compiler's defaults) contract this to one v_fmac_f32 -- one rounding per token; without the
    contraction the product and the sum round once each and the first sum (onto 0) is exact.  Either way a token's term passes
    through at most (n_bk - 1) + 1 roundings, n_bk = the tokens of image b in cluster k; one more u covers the second order of
    (1 + u)^m, m <= 513 + 1 + rho (m^2 u / 2 <= 1 for m <= 5792): n_bk - 1 + 2.
  * rnorm[t] = 1.0f / fmaxf(sqrtf(s2), 1e-12f) (SV_ASSIGN_TOKEN, csrc/assign_dev.h: assign_kernel and assign_wide_kernel).  s2: every square
    enters an fmaf chain (ss = fmaf(x, x, ss): the square itself is not rounded) of at most D / 2 terms -- the half-waves kk = 0, 1
    split D, the narrow kernel's four waves split it again -- and then one add across the half-waves and, in the narrow kernel,
    three across the waves: at most D / 2 + 3 roundings of non-negative terms, relative error (D / 2 + 3) u.  The square root
    halves it.  sqrtf and the division are correctly rounded: HIP's default (-fhip-fp32-correctly-rounded-divide-sqrt, which no
    flag of the build switches off) lowers them to v_sqrt_f32 with its one-ulp correction and to the v_div_scale / v_div_fmas /
    v_div_fixup sequence -- u each; fmaxf is exact.  rho = (D / 2 + 3) / 2 + 2, in units of u.
  * centroid_reduce_kernel adds the images' partials in fp64: nothing at this scale.
  So  |sums[k][c] - ref| <= u sum_b (n_bk - 1 + 2 + rho) sum_{t in image b, label k} |x^_tc|   (kmeans_shape_cases.bound).
  The accumulators are pre-filled here (sums with a non-zero pattern P, subtracted afterwards), which adds the fp64 roundings of
  P + s, one per call and one for the subtraction: (calls + 1) 2^-53 (|P| + sum |x^|), some 1e-9 of the bound.
The project's earlier figure, 1e-6 max|ref[k]| max(1, sqrt(n_k)) per cluster (tests/test_gpu_frows.py), is a measurement; both
ratios are printed for every case before anything is asserted.

The whole GPU run is in guard mode (tests/conftest.py): a write past the partial sums s_km_part or the partial counts s_km_cnt
fails the API call that made it.  These tests rely on that and add no check of their own.

Measured on an MI355X (the contiguous tensor and the strided view give the same figures; ratios of the worst entry to its bound):
  case                 max |err|  derived   earlier   second pass (2 x derived)
  k1_d32_n7_b1         1.1e-07    0.071     0.021     0.071
  k2_d36_n9_b3         4.0e-07    0.040     0.010     0.040
  k33_d96_n513_b2      1.2e-06    0.065     0.066     0.065
  k64_d256_n300_b2     1.7e-07    0.045     0.123     0.045
  k64_d260_n64_b2      3.9e-08    0.039     0.109     0.039
  k65_d128_n130_b2     8.6e-08    0.064     0.084     0.064
  k97_d384_n260_b3     5.9e-08    0.022     0.061     0.022
  k128_d132_n257_b5    2.4e-07    0.043     0.065     0.043
  k128_d1536_n130_b2   2.7e-08    0.010     0.137     0.010
The launch at K = 64 and at K = 128 -- 65536 B of dynamic LDS beside the kernel's 1024 B of static LDS, 66560 B in all, with no
call of sv_max_dyn_lds -- is accepted by the runtime as it stands (no SEGVLAD_ERR_HIP) and computes the figures above, the counts
out of s_cnt among them.  The earlier figure holds at every case as well and is asserted beside the derived bound.
"""
import numpy as np
import pytest
import torch

import kmeans_shape_cases as T

pytestmark = pytest.mark.gpu


def _prefill(K, D):
    """A known non-zero pattern (multiples of 2^-6 up to 1/2 in size) for sums, and one for counts"""
    k, c = np.arange(K)[:, None], np.arange(D)[None, :]
    return ((7 * k + 3 * c) % 65 - 32.5) / 64.0, (1000 + 3 * np.arange(K)).astype(np.int64)


def _run(eng, c, tok_of_call, sums, counts):
    """One pass over the case's images in its calls; returns the labels [B, N]"""
    labels = [eng.kmeans_step(tok_of_call(b0, nb), sums, counts, want_labels=True).cpu().numpy() for b0, nb in T.calls(c)]
    return np.concatenate(labels)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", T.NAMES)
def test_kmeans_step_against_the_fp64_reference(name):
    from revisit_anything_amd.engine import SegVLADEngine

    d, ref = T.build(name), T.reference(name)
    c, K, D, N, B = d["case"], d["K"], d["D"], d["N"], d["B"]
    facts = T.launch_facts(c)
    assert all(facts[key] == want for key, want in c["expect"].items()), name            # the branch it is named for
    dev = torch.device("cuda:0")
    tok = torch.from_numpy(d["tok"]).to(dev)                                            # [B, D, N], contiguous
    wide = torch.empty((B, D, 2 * N), dtype=torch.float32, device=dev).fill_(float("nan"))
    wide[:, :, ::2] = tok                                                               # every other column: a non-contiguous view
    inputs = {"contiguous": lambda b0, nb: tok[b0:b0 + nb], "strided view": lambda b0, nb: wide[b0:b0 + nb, :, ::2]}
    assert not inputs["strided view"](0, 1).is_contiguous()
    P, PC = _prefill(K, D)
    assert (P != 0).all()
    bound = T.bound(name) + (facts["calls"] + 1) * 2.0 ** -53 * (np.abs(P) + ref["apart"].sum(0))
    old = T.existing_figure(name)
    empty = ref["counts"] == 0
    assert K < 2 or empty[T.EMPTY_CLUSTER]
    eng = SegVLADEngine(0)
    try:
        eng.set_vocab(d["C"])
        for what, tok_of_call in inputs.items():
            sums, counts = torch.from_numpy(P).to(dev), torch.from_numpy(PC).to(dev)
            labels = _run(eng, c, tok_of_call, sums, counts)
            got, got_cnt = sums.cpu().numpy() - P, counts.cpu().numpy() - PC
            err = np.abs(got - ref["sums"])
            with np.errstate(divide="ignore", invalid="ignore"):
                r_new = float(np.where(err > 0, err / bound, 0.0).max())
                r_old = float(np.where(err > 0, err / old, 0.0).max())
            print(f"{name} {what}: labels differing {int((labels != ref['labels']).sum())}, counts differing "
                  f"{int((got_cnt != ref['counts']).sum())}, worst |err| {err.max():.3e}, worst err / derived bound {r_new:.3e}, "
                  f"worst err / (1e-6 max|ref[k]| max(1, sqrt n_k)) {r_old:.3e}")
            assert labels.dtype == np.uint8 and np.array_equal(labels, ref["labels"]), (name, what)
            assert np.array_equal(got_cnt, ref["counts"]), (name, what)
            assert np.all(got[empty] == 0), (name, what)                                # P + 0 - P: exactly 0
            assert np.all(err <= bound), (name, what, r_new)
            assert np.all(err <= old), (name, what, r_old)                              # the earlier figure holds at every case too
        # from zeroed accumulators: two runs with the same bits, then a second pass into the first run's
        runs = []
        for _ in range(2):
            sums = torch.zeros((K, D), dtype=torch.float64, device=dev)
            counts = torch.zeros(K, dtype=torch.int64, device=dev)
            _run(eng, c, inputs["contiguous"], sums, counts)
            runs.append((sums, counts))
        s0, s1 = runs[0][0].cpu().numpy(), runs[1][0].cpu().numpy()
        assert _bits_equal(s0, s1) and torch.equal(runs[0][1], runs[1][1]), name
        assert np.all(np.abs(s0 - ref["sums"]) <= T.bound(name)) and np.all(s0[empty] == 0), name
        _run(eng, c, inputs["contiguous"], *runs[0])
        s2 = runs[0][0].cpu().numpy()
        err2 = np.abs(s2 - 2 * ref["sums"])
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"{name} second pass: worst err / (2 x derived bound) {float(np.where(err2 > 0, err2 / T.bound(name, 2), 0.0).max()):.3e}")
        assert np.array_equal(runs[0][1].cpu().numpy(), 2 * ref["counts"]), name
        assert np.all(err2 <= T.bound(name, 2)) and np.all(s2[empty] == 0), name
    finally:
        eng.close()
