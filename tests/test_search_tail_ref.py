"""Pins tests/search_tail_ref.py: its references against the oracle (and the golden vote cases), and every generated input of
tests/test_gpu_search_tail.py against the conditions that make it worth running.  CPU only."""
import os

import numpy as np
import pytest

import search_tail_ref as R
from oracle import segvlad_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")


def _seg_range(off):
    return [np.arange(off[i], off[i + 1]) for i in range(len(off) - 1)]


# ---- the references ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
def test_vote_refs_equal_the_oracle_on_the_golden_cases(n):
    z = np.load(os.path.join(G, "vote_cases.npz"))
    off, im = z["off"], z["imInds"]
    sr = _seg_range(off)
    ids, sc = R.vote_wt(z["matches"], z["sims"], off, im, n)
    op, os_ = O.get_matches_wt_borda_im(z["matches"], len(sr), z["sims"], sr, im, n=n, return_scores=True)
    assert np.array_equal(ids, z[f"wt_n{n}"])
    for i, row in enumerate(op):
        assert ids[i][:len(row)].tolist() == [int(x) for x in row] and (ids[i][len(row):] == -1).all()
        assert np.array_equal(sc[i][:len(row)].view(np.uint64), np.array(os_[i], np.float64).view(np.uint64))
        assert (sc[i][len(row):].view(np.uint64) == 0).all()
    # COUNT: the documented rule (count desc, image id asc) over the oracle's counts
    ids, sc = R.vote_count(z["matches"], off, im, n)
    _, counts = O.get_matches_max_seg_topk(z["matches"], len(sr), sr, im, n=n)
    for i, bc in enumerate(counts):
        order = np.lexsort((np.arange(len(bc)), -bc))[:n]
        order = order[bc[order] > 0]
        assert ids[i][:len(order)].tolist() == order.tolist() and (ids[i][len(order):] == -1).all()
        assert sc[i][:len(order)].tolist() == bc[order].astype(np.float64).tolist() and (sc[i][len(order):] == 0).all()


def test_vote_refs_on_the_hand_made_tie_case():
    z = np.load(os.path.join(G, "vote_cases.npz"))
    off = np.array([0, 2])
    for n in (1, 4, 5):
        ids, _ = R.vote_wt(z["tie_matches"], z["tie_sims"], off, z["tie_imInds"], n)
        want = (z["tie_pred"].tolist() + [-1] * n)[:n]
        assert ids[0].tolist() == want
        assert [int(x) for x in O.get_matches_wt_borda_im(z["tie_matches"], 1, z["tie_sims"], [np.arange(2)], z["tie_imInds"], n=n)[0]] \
            == z["tie_pred"].tolist()[:n]
    ids, sc = R.vote_count(z["tie_matches"], off, z["tie_imInds"], 4)
    bc = np.bincount(z["tie_imInds"][z["tie_matches"].reshape(-1)])
    order = [g for g in np.lexsort((np.arange(len(bc)), -bc)) if bc[g] > 0][:4]
    assert ids[0][:len(order)].tolist() == order and sc[0][:len(order)].tolist() == bc[order].astype(float).tolist()


def test_vote_refs_skip_ids_outside_the_map_and_take_explicit_extrema():
    im = np.array([3, 3, 1, 0], np.int32)
    matches = np.array([[0, 4, 2], [-1, 1, 11]], np.int64)           # visiting order: 0, -1, 4, 1, 2, 11
    sims = np.array([[1.0, 0.5, 0.25], [0.75, 0.5, 0.0]], np.float32)
    ids, sc = R.vote_wt(matches, sims, np.array([0, 2, 2]), im, 3, smin=0.25, smax=0.75)
    assert ids.tolist() == [[3, 1, -1], [-1, -1, -1]]
    assert sc.tolist() == [[1.5 + 0.5, 0.0, 0.0], [0.0, 0.0, 0.0]]     # (1 - .25)/.5 + (.5 - .25)/.5; image 1: (.25 - .25)/.5
    ids, sc = R.vote_count(matches, np.array([0, 2, 2]), im, 2)
    assert ids.tolist() == [[3, 1], [-1, -1]] and sc.tolist() == [[2.0, 1.0], [0.0, 0.0]]


@pytest.mark.parametrize("shape", [(3, 50), (8, 200), (2, 1), (5, 13)])
@pytest.mark.parametrize("kind", ["distinct", "ties", "padded", "duplicates"])
def test_merge_ref_equals_the_oracle(shape, kind):
    parts, k = shape
    d, idx = R.merge_case(parts, k, kind)
    dp = [d[:, r * k:(r + 1) * k] for r in range(parts)]
    ip = [idx[:, r * k:(r + 1) * k] for r in range(parts)]
    od, oi = O.merge_topk(dp, ip, k)
    for got in (R.merge(dp, ip, k), R.merge(d, idx, k)):
        assert np.array_equal(got[1], oi) and np.array_equal(got[0].view(np.uint32), od.view(np.uint32))


def test_merge_ref_padding_counts_whatever_its_distance():
    d = np.array([[0.5, 0.1, 0.3, 0.2]], np.float32)
    idx = np.array([[7, -1, 9, 4]], np.int64)
    od, oi = R.merge(d, idx, 4)
    assert oi.tolist() == [[4, 9, 7, -1]] and od.tolist() == [[np.float32(0.2), np.float32(0.3), 0.5, np.inf]]


def test_sims_and_minmax_refs():
    d, idx = R.sims_case(4, 7)
    s, i = R.sims_from_d2(d, idx, 3)
    assert s.dtype == np.float32 and np.array_equal(s, (2.0 - d.astype(np.float64)[:, :3]).astype(np.float32)) and np.array_equal(i, idx[:, :3])
    assert all(np.isnan(v) for v in R.minmax(np.zeros(0, np.float32)))
    assert R.minmax(np.array([2, -3, np.inf], np.float32)) == (-3.0, np.inf)


# ---- the generated inputs: section 4 of the issue -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.VOTE_CASES))
def test_vote_case_sits_in_its_regime(name):
    segs, k, entries, regime, epad = R.VOTE_CASES[name]
    c = R.vote_case(name)
    counts = c["counts"]
    assert segs * k == entries and max(counts) == segs and counts[R.LARGEST] == segs and 3 in counts and 0 in counts
    assert R.case_regime(counts, k) == (regime, epad)
    small_regime, small_epad, big = R.launch_regime(counts, k)
    if regime == "global":
        assert big == [R.LARGEST] and entries == 16385                # one entry past the in-LDS sort
    else:
        assert big == [] and small_epad == epad
        # where the padding falls relative to 4096 / 8192 / 16384
        assert {"fast": epad <= 4096, "weights_in_lds": 4096 < epad <= 8192, "no_weight_array": 8192 < epad <= 16384}[regime]
    # runs of hundreds of entries
    rk = R.vote_count_ranking(c["matches"], c["off"], c["img_of_seg"])[R.LARGEST]
    assert rk[0][1] >= 300
    # explicit extrema: at least 1 % of the weights below 0 and at least 1 % above 1
    w = R.weights(c["sims"], *R.inner_extrema(c["sims"]))
    assert (w < 0).mean() >= 0.01 and (w > 1).mean() >= 0.01
    # n_top: the 3-segment image's row ends in padding at the largest value
    tops = R.n_top_set(c)
    assert tops[:2] == [1, 5] and len(R.vote_wt_ranking(c["matches"], c["sims"], c["off"], c["img_of_seg"])[0]) == tops[2] - 1
    # the invalid-id variant
    v = R.with_invalid_ids(c)
    bad = (v["matches"] < 0) | (v["matches"] >= len(v["img_of_seg"]))
    assert 0.03 < bad.mean() < 0.07
    assert {-1, len(v["img_of_seg"]), len(v["img_of_seg"]) + 7} == set(np.unique(v["matches"][bad]).tolist())
    starts, ends = R.run_edges_beside_skipped(v, R.LARGEST)
    assert starts >= 1 and ends >= 1


@pytest.mark.parametrize("name", R.REGIME_SHAPES)
def test_order_case_has_planted_weights_in_long_runs(name):
    c = R.order_case(name)
    assert R.case_regime(c["counts"], c["k"]) == R.VOTE_CASES[name][3:]
    assert np.min(c["sims"]) == 0.0 and c["planted"] >= 60
    n_small, runs = R.planted_weights(c)
    assert n_small >= 20 and runs >= 3
    w = R.weights(c["sims"])
    assert ((w > 0) & (w < 1e-8)).sum() >= 20                          # of order 1e-9 and below: they round in a sum above 2


def test_single_run_case():
    c = R.single_run_case()
    assert R.case_regime(c["counts"], c["k"]) == ("fast", 4096)
    rk = R.vote_count_ranking(c["matches"], c["off"], c["img_of_seg"])[0]
    assert rk == [(17, 4096.0)]
    w = R.weights(c["sims"])[:64]
    assert ((w == 0) | ((w >= R.TWO_M17) & (w <= 1))).all()            # ordinary weights: the run is not poisoned


@pytest.mark.parametrize("poison", [False, True])
def test_composition_cases_cross_the_regimes(poison):
    want = {0: "fast", 82: "weights_in_lds", 164: "no_weight_array", 328: "global"}
    fixed, _ = R.composition_case(0, poison)
    for comp in R.COMPANIONS:
        c, pos = R.composition_case(comp, poison)
        assert R.case_regime(c["counts"], c["k"])[0] == want[comp] and c["counts"][pos] == 40 and c["k"] == 50
        if comp:
            assert c["counts"][1 - pos] * 50 == {82: 4100, 164: 8200, 328: 16400}[comp]
            assert R.launch_regime(c["counts"], c["k"])[0] == ("fast" if comp == 328 else want[comp])
        rows = slice(c["off"][pos], c["off"][pos + 1])
        assert np.array_equal(c["matches"][rows], fixed["matches"]) and np.array_equal(c["sims"][rows], fixed["sims"])
        lo, hi = R.COMPOSITION_EXTREMA
        assert lo <= c["sims"].min() and c["sims"].max() <= hi
    w = R.weights(fixed["sims"], *R.COMPOSITION_EXTREMA)
    assert np.array_equal(w, fixed["sims"])
    n_small = int(((w > 0) & (w < R.TWO_M17)).sum())
    if poison:
        assert n_small >= 20 and fixed["planted"] >= 40
        score = dict(R.vote_wt_ranking(fixed["matches"], fixed["sims"], fixed["off"], fixed["img_of_seg"], *R.COMPOSITION_EXTREMA)[0])
        ids = R.visiting_order(fixed["matches"], fixed["off"], 0)[R.visiting_order((w > 0) & (w < R.TWO_M17), fixed["off"], 0)]
        assert sum(1 for g in set(fixed["img_of_seg"][ids].tolist()) if score[g] > 2.0) >= 3
    else:
        assert n_small == 0


@pytest.mark.parametrize("name", R.REGIME_SHAPES)
def test_tie_case_has_ties_in_the_first_places(name):
    c = R.tie_case(name)
    assert R.case_regime(c["counts"], c["k"]) == R.VOTE_CASES[name][3:]
    assert set(np.unique(c["sims"]).tolist()) == {0.0, 0.25, 0.5, 1.0}
    wt = R.vote_wt_ranking(c["matches"], c["sims"], c["off"], c["img_of_seg"])[R.LARGEST]
    cnt = R.vote_count_ranking(c["matches"], c["off"], c["img_of_seg"])[R.LARGEST]
    gw, gc = R.tie_groups(wt, R.TIE_N_TOP), R.tie_groups(cnt, R.TIE_N_TOP)
    assert len(gw) >= 3 and len(gc) >= 3, (gw, gc)
    # the two tie rules disagree on these inputs: a WT group is not in id order (first appearance decides) ...
    assert any(g != sorted(g) for g in gw)
    # ... and a COUNT group, which is, is not in order of first appearance
    ids = R.visiting_order(c["matches"], c["off"], R.LARGEST)
    first = {}
    for o, g in enumerate(c["img_of_seg"][ids].tolist()):
        first.setdefault(g, o)
    assert all(g == sorted(g) for g in gc) and any(g != sorted(g, key=first.get) for g in gc)


@pytest.mark.parametrize("shape", R.MERGE_SHAPES)
@pytest.mark.parametrize("kind", R.MERGE_KINDS)
def test_merge_case_is_what_its_kind_says(shape, kind):
    parts, k = shape
    d, idx = R.merge_case(parts, k, kind)
    nq, cand = d.shape
    assert cand == parts * k and nq == R.merge_rows(parts, k) and cand <= 8192
    valid = idx >= 0
    assert d.dtype == np.float32 and not np.isnan(d).any() and not np.signbit(d).any() and np.isfinite(d[valid]).all()
    if kind != "duplicates":
        for q in range(nq):
            assert len(np.unique(idx[q][valid[q]])) == valid[q].sum()     # distinct ids
    sd, si = R.sorted_parts(d, idx, parts, k)
    is_sorted = (sd.view(np.uint32) == d.view(np.uint32)).all(axis=1) & (si == idx).all(axis=1)
    if kind == "distinct":
        assert valid.all() and is_sorted.all()
        assert all(len(np.unique(d[q])) == cand for q in range(nq))
    elif kind == "ties":
        assert valid.all() and is_sorted.all() and np.isin(d, R.TIE_POOL).all()
        if parts > 1:
            assert R.cross_part_tie_rows(d, idx, parts, k) >= nq / 2
        if k > 1:                                        # equal distances inside a part as well
            assert (d.reshape(nq, parts, k)[:, :, 1:] == d.reshape(nq, parts, k)[:, :, :-1]).any()
    elif kind == "padded":
        assert is_sorted.all() and not valid[0].any() and np.isinf(d[~valid]).all()
        per_part = valid.reshape(nq, parts, k).sum(axis=2)
        assert per_part[1].tolist() == [k if r == 1 % parts else 0 for r in range(parts)]
        if k > 1:
            assert len(np.unique(per_part[2:])) > 2                  # tails of assorted lengths
    elif kind == "unsorted":
        if k >= 2:
            assert (~is_sorted).sum() == len(range(0, nq, 3)) and not is_sorted[0] and is_sorted[1]
        else:
            assert is_sorted.all()                        # a part of one entry cannot be out of order
    elif kind == "duplicates":
        assert valid.all() and is_sorted.all() and np.isin(d, R.TIE_POOL).all()
        if parts > 1:                                    # the same (distance, id) from two parts, inside or across the first k
            assert R.cross_part_duplicate_rows(d, idx, parts, k) >= nq / 2
            for q in range(nq):                          # an id is always listed with one distance
                u, first = np.unique(idx[q], return_index=True)
                assert len(u) < cand and (d[q] == d[q][first][np.searchsorted(u, idx[q])]).all()
    else:
        assert (~valid).sum(axis=1).tolist() == [1] * nq
        assert np.isfinite(d[~valid][0::2]).all() and np.isinf(d[~valid][1::2]).all()
        if k >= 3:
            assert not is_sorted.any()                   # the slot sits in the middle of its part


@pytest.mark.parametrize("shape", R.SIMS_SHAPES)
@pytest.mark.parametrize("nq", [1, 257])
def test_sims_case(shape, nq):
    k_in, k_keep = shape
    d, idx = R.sims_case(nq, k_in)
    assert d.shape == (nq, k_in) and k_keep <= k_in
    assert (np.isinf(d) == (idx < 0)).all() and np.isinf(d[0]).all()
    assert np.isinf(d[:, :k_keep]).any()                                # a pad reaches the kept columns
    if nq > 1:
        assert np.isfinite(d[:, :k_keep]).any()


@pytest.mark.parametrize("count", R.MINMAX_COUNTS)
@pytest.mark.parametrize("kind", R.MINMAX_KINDS)
def test_minmax_case(count, kind):
    x = R.minmax_case(count, kind)
    assert x.shape == (count,) and not np.isnan(x).any() and (x != 0).all()
    if count == 0:
        return
    lo, hi = R.minmax(x)
    if count > 1:
        assert (x < 0).any() and (x > 0).any()
        if kind == "inf_inside":
            assert lo == -np.inf and hi == np.inf
        else:
            a, b = (0, count - 1) if kind == "min_first_max_last" else (count - 1, 0)
            assert x[a] == lo and x[b] == hi and (x == lo).sum() == 1 and (x == hi).sum() == 1
