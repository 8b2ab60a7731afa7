"""Preconditions of tests/test_gpu_describe_shapes.py, decided by the fp64 oracle alone (no GPU): every case of
tests/describe_shape_cases.py has a top-2 cosine gap >= 1e-4 at every token and non-zero block norms >= 1e-2 -- so the GPU
test leaves out no token and no block -- and reaches the branch it is named for."""
import numpy as np
import pytest

import describe_shape_cases as T

MIN_GAP, MIN_BLOCK_NORM = 1e-4, 1e-2


def test_the_table_holds_the_shapes_the_kernels_branch_on():
    facts = {c["name"]: T.launch_facts(c) for c in T.CASES}
    assert len(set(T.NAMES)) == len(T.NAMES)
    assert {f["assign"] for f in facts.values()} == {"wide<1>", "wide<2>", "narrow<1>", "narrow<4>"}
    # (assign_kernel<2> is only reached by option: the GPU test forces it on the wide<2> cases with assign_narrow=1)
    assert {f["kpad"] for f in facts.values()} == {32, 64, 128}
    assert {1, 2, 3, 12} <= {f["agg_waves"] for f in facts.values()}
    assert {32, 36, 72, 96} <= {f["last_slab"] for f in facts.values()}            # partial 128-wide slabs of D
    assert {0, 1, 2, 3} == {f["kpb_tail"] for f in facts.values()}
    assert {1, 2, 3, 7} <= {f["SC"] for f in facts.values()}
    assert {f["staged"] for f in facts.values()} == {True, False}
    assert {(f["x3"], f["project"]) for f in facts.values()} == {(False, False), (True, False), (True, True)}
    assert {c["expect"].get("task_class") for c in T.CASES} >= set(T.TASK_CLASSES)
    assert any(c["expect"].get("task_class") and c["D"] != 64 for c in T.CASES)
    for c in T.CASES:
        assert len(c["segs"]) == T.B <= 4 and T.P <= 64 and c["segs"][1] == 0 and c["segs"][3] == c["segs"][0]
        assert c["N"] <= 600 or c["name"] == "k32_d32_n1530_s400"
        assert c["K"] <= 128 and c["D"] % 4 == 0 and c["D"] <= 1536


@pytest.mark.parametrize("name", T.NAMES)
def test_case_qualifies(name):
    d = T.build(name)
    c, K, N = d["case"], d["K"], d["N"]
    facts = T.launch_facts(c)
    for key, want in c["expect"].items():
        if key not in ("task_class", "top_label"):
            assert facts[key] == want, (name, key, facts[key], want)
    if name == "k32_d32_n1530_s400":     # the non-staged neighbour union: too large to stage, small enough to run
        assert facts["prep_lds_staged"] > 150 * 1024 and facts["prep_lds"] < 160 * 1024
        assert (facts["prep_lds"], facts["prep_lds_staged"]) == (89360, 188264)
    assert facts["prep_lds"] < 160 * 1024
    for with_adj in (True, False):
        ref = T.reference(name, with_adj)
        gap = ref["gap"].min()
        bn = ref["block_norms"]
        print(f"{name} adj={with_adj}: min gap {gap:.3e}, min non-zero block norm {bn[bn > 0].min():.3e}")
        assert gap >= MIN_GAP, (name, gap)
        assert bn[bn > 0].min() >= MIN_BLOCK_NORM, name
        # what every batch holds
        offs, zero = d["offs"], ref["zero_rows"]
        assert zero[offs[0] + 1] and zero[offs[3] + 1] and (with_adj or zero[offs[2] + 1])
        assert np.all(ref["out"][zero] == 0) and np.all(np.abs(np.linalg.norm(ref["out"][~zero], axis=1) - 1) < 1e-9)
    assert not d["incs"][0][1].any() and not d["incs"][2][1].any()           # a segment that covers no token
    assert d["adjs"][0][1].sum() == 1 and d["adjs"][0][:, 1].sum() >= 1
    assert d["toks"][3] is d["toks"][0] and d["incs"][3] is d["incs"][0]     # the same image twice
    cnt = T.task_sizes(T.reference(name, True)["labels"], K)
    if K >= 2:
        assert (cnt[:, T.EMPTY_CLUSTER] == 0).all() and cnt[:, 0].sum() > 0   # a cluster without a token in any image, behind one that holds some
    if "task_class" in c["expect"]:
        lo, hi = T.TASK_CLASSES[c["expect"]["task_class"]]
        assert cnt[cnt > 0].min() >= lo and cnt.max() <= hi, (name, cnt[cnt > 0].min(), cnt.max())
    if "top_label" in c["expect"]:
        assert T.reference(name, True)["labels"].max() == c["expect"]["top_label"] == K - 1
    assert np.array_equal(cnt.sum(1), [N] * T.B)


@pytest.mark.parametrize("K,D", T.EXTRA_SHAPES)
def test_negative_scores_batch_qualifies(K, D):
    d = T.negative_scores_batch(K, D)
    for b in range(2):
        sc = T.oracle_scores(d["toks"][b], d["C"])
        part = np.partition(sc, -2, axis=1)
        print(f"K={K}: largest score {sc.max():.3f}, min gap {(part[:, -1] - part[:, -2]).min():.3e}")
        assert sc.max() < -0.05                                   # every real centre below the padded centres' 0
        assert (part[:, -1] - part[:, -2]).min() >= MIN_GAP
    ref = T.oracle_batch(d["toks"], d["incs"], d["adjs"], d["C"], True)
    assert ref["labels"].max() < K and len(np.unique(ref["labels"])) > 1
    bn = ref["block_norms"]
    assert bn[bn > 0].min() >= MIN_BLOCK_NORM


@pytest.mark.parametrize("K,D", T.EXTRA_SHAPES)
def test_zero_column_batch_qualifies(K, D):
    from oracle import segvlad_oracle as O

    d = T.zero_column_batch(K, D)
    assert not d["toks"][0][:, T.ZERO_TOKEN].any() and d["incs"][0][0, T.ZERO_TOKEN]
    norms = np.concatenate([np.delete(np.linalg.norm(d["toks"][0], axis=0), T.ZERO_TOKEN), np.linalg.norm(d["toks"][1], axis=0)])
    assert norms.min() < 2e-3 and norms.max() > 5e2               # un-normalised magnitudes over six decades
    ref = T.oracle_batch(d["toks"], d["incs"], d["adjs"], d["C"], True)
    # the zero token: label 0 by the first-maximum rule, residual -C[0] (max(norm, EPS) leaves x^ = 0)
    assert ref["labels"][0, T.ZERO_TOKEN] == 0 and ref["gap"][0, T.ZERO_TOKEN] == 0
    xn = O.normalize_tokens_f32(d["toks"][0])
    assert not xn[T.ZERO_TOKEN].any()
    gap = ref["gap"].copy()
    gap[0, T.ZERO_TOKEN] = np.inf
    assert gap.min() >= MIN_GAP
    bn = ref["block_norms"]
    assert bn[bn > 0].min() >= MIN_BLOCK_NORM
