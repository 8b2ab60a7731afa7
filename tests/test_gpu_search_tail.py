"""The search tail -- segvlad_merge_topk, segvlad_sims_from_d2, segvlad_minmax, segvlad_vote (csrc/select_kernels.hip,
csrc/vote_kernels.hip) -- against the plain references of tests/search_tail_ref.py, across the code paths these kernels choose by
shape.  Every comparison is bit for bit (ids equal, scores equal as float64 words, distances as float32 words), every query image
and every row is checked.  The inputs come from the generators of search_tail_ref.py; tests/test_search_tail_ref.py holds the
conditions each of them must meet (regime, planted weights, ties, ...), the cheap ones are asserted again here.

The vote's regimes (sv_launch_vote; E = segments x k of the largest image that the in-LDS launch takes):
  fast (E <= 4096)                 test_vote_regimes[fast_last_64x64], test_vote_order_sensitive_sums[fast_last_64x64],
                                   test_vote_one_run_of_4096, test_vote_ties[fast_last_64x64], test_vote_batch_composition (alone)
  weights in LDS (<= 8192)         ..._regimes[wl_first_241x17], [wl_last_64x128], ..._order_sensitive_sums / _ties[wl_first_241x17],
                                   test_vote_batch_composition (beside 82 segments)
  no weight array (<= 16384)       ..._regimes[nowl_first_2731x3], [nowl_last_128x128], [bench_depth_50x200],
                                   ..._order_sensitive_sums / _ties[nowl_first_2731x3], test_vote_batch_composition (beside 164)
  GLOBAL (> 16384)                 ..._regimes[global_first_145x113], ..._order_sensitive_sums / _ties[global_first_145x113],
                                   test_vote_batch_composition (beside 328: the fixed image itself stays in the fast launch)"""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import search_tail_ref as R

pytestmark = pytest.mark.gpu

WT, COUNT = 0, 1


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import SegVLADEngine

    assert (_lib.VOTE_WT_BORDA_IM, _lib.VOTE_COUNT) == (WT, COUNT)
    e = SegVLADEngine(0)
    yield e
    e.close()


def _vote(eng, c, n_top, mode=WT, extrema=(float("nan"), float("nan"))):
    pred, sc = eng.vote(c["matches"], None if mode == COUNT else c["sims"], c["off"], n_top=n_top, mode=mode, img_of_seg=c["img_of_seg"],
                        smin=extrema[0], smax=extrema[1])
    return pred.cpu().numpy(), sc.cpu().numpy()


def _same_vote(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    bad = np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))
    assert len(bad) == 0, (what, bad[:5], got[1][tuple(bad[0])], want[1][tuple(bad[0])])


# ---- the vote, per regime and at each boundary --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.VOTE_CASES))
def test_vote_regimes(eng, name):
    segs, k, entries, regime, epad = R.VOTE_CASES[name]
    c = R.vote_case(name)
    assert c["counts"][R.LARGEST] * c["k"] == entries and R.case_regime(c["counts"], c["k"]) == (regime, epad)
    ext = R.inner_extrema(c["sims"])
    w = R.weights(c["sims"], *ext)
    assert (w < 0).mean() >= 0.01 and (w > 1).mean() >= 0.01
    args = (c["off"], c["img_of_seg"])
    want = {"wt": R.vote_wt_ranking(c["matches"], c["sims"], *args),
            "wt_explicit": R.vote_wt_ranking(c["matches"], c["sims"], *args, *ext),
            "count": R.vote_count_ranking(c["matches"], *args)}
    tops = R.n_top_set(c)
    assert tops[2] == len(want["wt"][0]) + 1             # the 3-segment image's row ends in (-1, 0.0)
    for n_top in tops:
        _same_vote(_vote(eng, c, n_top), R.padded(want["wt"], n_top), ("wt", n_top))
        _same_vote(_vote(eng, c, n_top, extrema=ext), R.padded(want["wt_explicit"], n_top), ("wt_explicit", n_top))
        _same_vote(_vote(eng, c, n_top, mode=COUNT), R.padded(want["count"], n_top), ("count", n_top))
    # ids outside [0, n_ref): skipped; their similarities still enter the extrema that the call computes itself
    v = R.with_invalid_ids(c)
    bad = (v["matches"] < 0) | (v["matches"] >= len(v["img_of_seg"]))
    assert bad.mean() > 0.03 and min(R.run_edges_beside_skipped(v, R.LARGEST)) >= 1
    _same_vote(_vote(eng, v, 5), R.vote_wt(v["matches"], v["sims"], *args, 5), "invalid wt")
    _same_vote(_vote(eng, v, 5, extrema=ext), R.vote_wt(v["matches"], v["sims"], *args, 5, *ext), "invalid wt_explicit")
    _same_vote(_vote(eng, v, 5, mode=COUNT), R.vote_count(v["matches"], *args, 5), "invalid count")


# ---- batch composition must not change an image's bits ------------------------------------------------------------------
@pytest.mark.parametrize("mode", [WT, COUNT], ids=["wt", "count"])
@pytest.mark.parametrize("poison", [False, True], ids=["ordinary", "poisoned"])
def test_vote_batch_composition(eng, mode, poison):
    ext = R.COMPOSITION_EXTREMA
    fixed, _ = R.composition_case(0, poison)
    if poison:
        w = R.weights(fixed["sims"], *ext)
        assert ((w > 0) & (w < R.TWO_M17)).sum() >= 20
    n_top = 7
    if mode == WT:
        want = R.vote_wt(fixed["matches"], fixed["sims"], fixed["off"], fixed["img_of_seg"], n_top, *ext)
    else:
        want = R.vote_count(fixed["matches"], fixed["off"], fixed["img_of_seg"], n_top)
    regimes = []
    for comp in R.COMPANIONS:
        c, pos = R.composition_case(comp, poison)
        regimes.append(R.case_regime(c["counts"], c["k"])[0])
        got = _vote(eng, c, n_top, mode=mode, extrema=ext)
        _same_vote((got[0][pos:pos + 1], got[1][pos:pos + 1]), want, ("fixed image beside", comp))
        # the companion, too, is what the reference says
        if mode == WT:
            _same_vote(got, R.vote_wt(c["matches"], c["sims"], c["off"], c["img_of_seg"], n_top, *ext), ("batch", comp))
        else:
            _same_vote(got, R.vote_count(c["matches"], c["off"], c["img_of_seg"], n_top), ("batch", comp))
    assert regimes == ["fast", "weights_in_lds", "no_weight_array", "global"]


# ---- sums whose bits depend on the order of the additions ---------------------------------------------------------------
@pytest.mark.parametrize("name", R.REGIME_SHAPES)
def test_vote_order_sensitive_sums(eng, name):
    c = R.order_case(name)
    assert R.case_regime(c["counts"], c["k"]) == R.VOTE_CASES[name][3:] and np.min(c["sims"]) == 0.0
    w = R.weights(c["sims"])
    assert ((w > 0) & (w < R.TWO_M17)).sum() >= 20
    want = R.vote_wt_ranking(c["matches"], c["sims"], c["off"], c["img_of_seg"])
    assert sum(1 for g in c["hot"] if dict(want[R.LARGEST])[g] > 2.0) >= 3
    for n_top in (5, 12):
        _same_vote(_vote(eng, c, n_top), R.padded(want, n_top), n_top)


def test_vote_one_run_of_4096(eng):
    c = R.single_run_case()
    assert R.case_regime(c["counts"], c["k"]) == ("fast", 4096)
    _same_vote(_vote(eng, c, 3), R.vote_wt(c["matches"], c["sims"], c["off"], c["img_of_seg"], 3))
    got = _vote(eng, c, 3, mode=COUNT)
    _same_vote(got, R.vote_count(c["matches"], c["off"], c["img_of_seg"], 3))
    assert got[0][0].tolist() == [17, -1, -1] and got[1][0].tolist() == [4096.0, 0.0, 0.0]


# ---- ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.REGIME_SHAPES)
def test_vote_ties(eng, name):
    c = R.tie_case(name)
    assert R.case_regime(c["counts"], c["k"]) == R.VOTE_CASES[name][3:]
    n_top = R.TIE_N_TOP
    wt = R.vote_wt_ranking(c["matches"], c["sims"], c["off"], c["img_of_seg"])
    cnt = R.vote_count_ranking(c["matches"], c["off"], c["img_of_seg"])
    assert len(R.tie_groups(wt[R.LARGEST], n_top)) >= 3 and len(R.tie_groups(cnt[R.LARGEST], n_top)) >= 3
    _same_vote(_vote(eng, c, n_top), R.padded(wt, n_top), "wt")                    # first appearance
    _same_vote(_vote(eng, c, n_top, mode=COUNT), R.padded(cnt, n_top), "count")    # lower image id


# ---- merge ------------------------------------------------------------------------------------------------------------
def _same_lists(got, want, what=""):
    gd, gi = (t.cpu().numpy() for t in got)
    assert gd.dtype == np.float32 and gi.dtype == np.int64 and gi.shape == want[1].shape
    assert np.array_equal(gi, want[1]), (what, np.argwhere(gi != want[1])[:5])
    assert np.array_equal(gd.view(np.uint32), want[0].view(np.uint32)), (what, np.argwhere(gd.view(np.uint32) != want[0].view(np.uint32))[:5])


def _merge(eng, d, idx, parts, k):
    """segvlad_merge_topk into outputs that hold a sentinel: a slot the kernel never writes shows."""
    nq = len(d)
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device=eng.device)
    oi = torch.full((nq, k), -7, dtype=torch.int64, device=eng.device)
    eng._stream()
    rc = eng.lib.segvlad_merge_topk(eng._h, d.ctypes.data, idx.ctypes.data, nq, parts, k, od.data_ptr(), oi.data_ptr())
    assert rc == 0, rc
    return od, oi


@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", R.MERGE_KINDS)
def test_merge(eng, shape, kind):
    parts, k = shape
    d, idx = R.merge_case(parts, k, kind)
    assert d.shape == (R.merge_rows(parts, k), parts * k) and not np.isnan(d).any() and not np.signbit(d).any()
    if kind == "ties" and parts > 1:
        assert R.cross_part_tie_rows(d, idx, parts, k) >= len(d) / 2
    if kind == "duplicates" and parts > 1:
        assert R.cross_part_duplicate_rows(d, idx, parts, k) >= len(d) / 2
    _same_lists(_merge(eng, d, idx, parts, k), R.merge(d, idx, k), (shape, kind))


def test_merge_refuses_more_than_8192_candidates(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    d = np.tile(np.sort(np.random.default_rng(9).random((1, 1024)).astype(np.float32), axis=1), (2, 9))
    idx = np.tile(np.arange(9 * 1024, dtype=np.int64), (2, 1))
    with pytest.raises(SegVLADError) as e:
        eng.merge_topk(d, idx, 9, 1024)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    # the context stays usable, at the limit itself too
    for shape in ((3, 50), (8, 1024)):
        d, idx = R.merge_case(*shape, "distinct")
        _same_lists(eng.merge_topk(d, idx, *shape), R.merge(d, idx, shape[1]), shape)


# ---- sims_from_d2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SIMS_SHAPES, ids=lambda s: "%dto%d" % s)
@pytest.mark.parametrize("nq", [1, 257])
def test_sims_from_d2(eng, shape, nq):
    k_in, k_keep = shape
    d, idx = R.sims_case(nq, k_in)
    assert np.isinf(d[:, :k_keep]).any() and (idx[np.isinf(d)] == -1).all()
    _same_lists(eng.sims_from_d2(d, idx, k_keep), R.sims_from_d2(d, idx, k_keep))


# ---- minmax -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", R.MINMAX_COUNTS)
@pytest.mark.parametrize("kind", R.MINMAX_KINDS)
def test_minmax(eng, count, kind):
    x = R.minmax_case(count, kind)
    assert x.shape == (count,) and not np.isnan(x).any() and (x != 0).all()
    got = eng.minmax(x).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2,)
    if count == 0:
        assert np.isnan(got).all()
        return
    assert got[0] == np.min(x) and got[1] == np.max(x), (got, np.min(x), np.max(x))
    # a device tensor takes the same kernels without the staging copy
    got = eng.minmax(torch.from_numpy(x).to(eng.device)).cpu().numpy()
    assert got[0] == np.min(x) and got[1] == np.max(x)
