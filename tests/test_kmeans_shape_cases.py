"""Preconditions of tests/test_gpu_kmeans_shapes.py, decided by the fp64 oracle and NumPy alone (no GPU): every case of
tests/kmeans_shape_cases.py reaches the branch it is named for, has a top-2 cosine gap >= 1e-4 at every token -- so the GPU
test leaves no token out -- and an error bound with teeth: each way in which centroid_sums_kernel could be subtly wrong moves
some entry of the sums or counts by 10 times or more of what the GPU test allows that entry."""
import numpy as np
import pytest

import kmeans_shape_cases as T

MIN_GAP, TEETH = 1e-4, 10.0


def test_the_table_holds_the_shapes_the_launcher_branches_on():
    facts = {c["name"]: T.launch_facts(c) for c in T.CASES}
    assert len(set(T.NAMES)) == len(T.NAMES)
    assert {f["CH"] for f in facts.values()} == {256, 128}
    assert {(c["K"], facts[c["name"]]["lds"]) for c in T.CASES} >= {(64, 66560), (128, 66560)}     # 64 KiB + s_cnt at both CH
    assert {(c["K"], facts[c["name"]]["CH"]) for c in T.CASES} >= {(64, 256), (65, 128)}            # either side of the switch
    assert {1, 2, 3, 12} <= {f["chunks"] for f in facts.values()}
    assert any(c["D"] < f["CH"] for c, f in zip(T.CASES, facts.values()))                           # idle threads, cw < CH
    assert sum(c["D"] == f["CH"] for c, f in zip(T.CASES, facts.values())) >= 2                     # at CH = 256 and at 128
    assert sum(f["chunks"] > 1 and f["last_cw"] == 4 for f in facts.values()) >= 2                  # a 4-column tail at both CH
    assert {0, 1, 7} <= {f["pad_lanes"] for f in facts.values()}
    assert any(c["N"] < 8 for c in T.CASES) and any(c["N"] % 8 == 1 and c["N"] > 8 for c in T.CASES)
    assert {1, 2, 3} <= {f["hist_rounds"] for f in facts.values()}
    assert {1, 2, 3} <= {f["calls"] for f in facts.values()}
    assert {c["K"] for c in T.CASES} >= {1, 2, 64, 65, 128} and any(c["B"] == 1 for c in T.CASES)
    for c in T.CASES:
        assert c["K"] <= 128 and c["D"] % 4 == 0 and c["D"] <= 1536 and c["N"] <= 600 and c["B"] <= 5


@pytest.mark.parametrize("name", T.NAMES)
def test_case_qualifies(name):
    d, r = T.build(name), T.reference(name)
    c, K, N, B = d["case"], d["K"], d["N"], d["B"]
    facts = T.launch_facts(c)
    for key, want in c["expect"].items():
        assert facts[key] == want, (name, key, facts[key], want)
    gap = r["gap"].min()
    print(f"{name}: min top-2 gap {gap:.3e}")
    assert gap >= MIN_GAP and (K > 1 or np.isposinf(r["gap"]).all()), (name, gap)
    print(f"{name}: {(r['labels'] != d['drawn']).mean():.3f} of the tokens left the centre they were drawn around")
    assert np.array_equal(r["cnt"].sum(1), [N] * B)
    assert K == 2 or (r["labels"][:, -1] == K - 1).all()                # the top label, in every image (at K = 2 it is the empty one)
    if K >= 2:
        assert (r["cnt"][:, T.EMPTY_CLUSTER] == 0).all() and not r["sums"][T.EMPTY_CLUSTER].any()
    if K >= 3:
        one = np.zeros(B, np.int64)
        one[T.single_image(B)] = 1
        assert np.array_equal(r["cnt"][:, T.SINGLE_CLUSTER], one)       # one token, in one image
    norms = np.linalg.norm(d["tok"].astype(np.float64), axis=1)
    assert norms.min() < 0.7 * norms.max()                              # un-normalised: the kernel has to normalise
    cn = np.linalg.norm(d["C"].astype(np.float64), axis=1)
    assert 0.4 - 1e-6 <= cn.min() and cn.max() <= 1 + 1e-6


@pytest.mark.parametrize("name", T.NAMES)
def test_the_bound_has_teeth(name):
    c, r = T.BY_NAME[name], T.reference(name)
    bound = T.bound(name)
    assert bound.shape == r["sums"].shape and (bound[r["counts"] > 0] > 0).all()
    assert not bound[r["counts"] == 0].any()                            # empty clusters: exactly 0
    applied, smallest = 0, np.inf
    for what, perturb in T.PERTURBATIONS:
        got = perturb(c, r)
        if got is None:
            print(f"{name}: {what}: a no-op at this shape")
            continue
        sums, counts = got
        moved = np.abs(sums - r["sums"])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(moved > 0, moved / bound, 0.0).max()       # (an entry that must be exactly 0: inf when it moves)
        n_cnt = int((counts != r["counts"]).sum())                      # counts are held exactly: any change is past the bound
        print(f"{name}: {what}: largest move / bound {ratio:.3e}, counts changed {n_cnt}")
        assert ratio >= TEETH or n_cnt > 0, (name, what, ratio)
        if what != "histogram of the first 256 tokens":
            assert ratio >= TEETH, (name, what, ratio)                  # the sums alone show it
            smallest = min(smallest, ratio)
        applied += 1
    print(f"{name}: smallest perturbation / bound {smallest:.3e} over {applied} perturbations")
    assert applied >= 2 and smallest >= TEETH, name


def test_skipped_perturbations_are_no_ops():
    """Where a perturbation returns None the mistake it stands for changes nothing at that shape: stated from the shape."""
    for c in T.CASES:
        r, f = T.reference(c["name"]), T.launch_facts(c)
        skipped = {what for what, p in T.PERTURBATIONS if p(c, r) is None}
        assert ("last token added per padding lane" in skipped) == (c["N"] % 8 == 0 and f["pad_lanes"] == 0)
        assert ("ragged last chunk left at zero" in skipped) == (c["D"] % f["CH"] == 0)
        # one chunk: 256 * 0 == 128 * 0; K <= 64: CH is 256
        assert ("chunk offset 256 j at K > 64" in skipped) == (f["CH"] == 256 or c["D"] <= 128)
        if c["N"] <= 256:                                               # one strided round reads every token
            assert "histogram of the first 256 tokens" in skipped and f["hist_rounds"] == 1
            assert all(np.array_equal(np.bincount(l[:256], minlength=c["K"]), n) for l, n in zip(r["labels"], r["cnt"]))
        assert ("second call overwrites" in skipped) == (c["B"] <= c["batch"])
        assert ("image 1's partial from image 0" in skipped) == (c["B"] == 1)
        assert "last token dropped" not in skipped
    assert [c["name"] for c in T.CASES if c["N"] % 8 == 0] == ["k64_d260_n64_b2"]
