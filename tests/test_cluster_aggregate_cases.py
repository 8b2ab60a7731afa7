"""Preconditions of tests/test_gpu_cluster_aggregate.py, decided by the fp64 oracle alone (no GPU): every case of
tests/cluster_aggregate_cases.py reaches the shape it is named for, holds the labels it promises, has non-zero block norms
>= 1e-2 -- so the GPU test leaves no block out -- and, where num_c > 128, a reference that a 7-bit label path would miss by more
than 10 times the descriptor bound."""
import numpy as np
import pytest

import cluster_aggregate_cases as T

MIN_BLOCK_NORM, DESC_TOL = 1e-2, 2e-6


def test_the_table_holds_the_shapes_the_entry_has_never_run():
    facts = {c["name"]: T.launch_facts(c) for c in T.CASES}
    assert [(c["num_c"], c["D"], c["N"], c["S"]) for c in T.CASES] == [(1, 4, 65, 3), (5, 36, 200, 9), (129, 36, 300, 37),
                                                                      (200, 132, 513, 70), (255, 64, 257, 9), (256, 32, 1030, 129)]
    assert {0, 1, 3} <= {f["kpb_tail"] for f in facts.values()} and {1, 2, 3} == {f["SC"] for f in facts.values()}
    assert {4, 36} <= {f["last_slab"] for f in facts.values()} and {1, 2} == {f["agg_waves"] for f in facts.values()}
    assert sum(c["num_c"] > 128 for c in T.CASES) == 4 and max(c["num_c"] for c in T.CASES) == 256
    assert any(c["D"] % 4 == 0 and c["D"] % 32 != 0 for c in T.CASES)
    for c in T.CASES:
        assert max(facts[c["name"]]["prep_lds"]) < 150 * 1024            # prep_kernel takes the case, staged


@pytest.mark.parametrize("name", T.NAMES)
def test_case_qualifies(name):
    d = T.build(name)
    c, K, N, S = d["case"], d["num_c"], d["N"], d["S"]
    facts = T.launch_facts(c)
    for key, want in c["expect"].items():
        assert facts[key] == want, (name, key, facts[key], want)
    lab = d["labels"]
    cnt = np.bincount(lab, minlength=K)
    assert lab.dtype == np.uint8 and lab.max() == K - 1 and len(cnt) == K and d["res"].dtype == np.float32
    if K >= 2:
        assert cnt[T.EMPTY] == 0 and cnt[0] > 0                          # an empty cluster behind one that holds tokens
    if K >= 3:
        assert cnt[T.SINGLE] == 1 and d["inc"][0, d["single_token"]]     # a single token, covered
    assert not d["inc"][1].any() and d["adj"][1].sum() == 1 and d["adj"].diagonal().all()
    assert abs(d["adj"].mean() - T.ADJ_DENSITY) < 0.35                  # (S = 3: the diagonal alone is a third)
    assert d["inc"][:, lab == K - 1].any()                              # a top-label token that a segment covers
    for with_adj in (False, True):
        out, bn, zero = T.reference(name, with_adj)
        print(f"{name} adj={int(with_adj)}: min non-zero block norm {bn[bn > 0].min():.3e}, rows exactly 0: {int(zero.sum())}")
        assert bn[bn > 0].min() >= MIN_BLOCK_NORM, name
        assert zero[1] and np.all(out[zero] == 0) and np.all(np.abs(np.linalg.norm(out[~zero], axis=1) - 1) < 1e-9)
        if with_adj and S >= 9:   # the adjacency is more than its diagonal, and the union changes the descriptors
            assert d["adj"].sum() > S and np.abs(out - T.reference(name, False)[0]).max() > 10 * DESC_TOL
        if K >= 2:
            assert not bn[:, T.EMPTY].any()
        if K >= 3:
            assert bn[0, T.SINGLE] > 0
        if K > 128:      # what a 7-bit label path would compute: the top label's tokens in cluster (num_c - 1) & 127
            folded = np.where(lab == K - 1, (K - 1) & 127, lab)
            moved = np.abs(T.oracle(d, folded, with_adj)[0] - out).max()
            print(f"{name} adj={int(with_adj)}: top label folded to 7 bits moves the reference by {moved:.3e} = {moved / DESC_TOL:.1f} x bound")
            assert moved > 10 * DESC_TOL, (name, moved)
