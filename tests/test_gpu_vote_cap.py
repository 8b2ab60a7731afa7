"""segvlad_vote with SEGVLAD_VOTE_PER_IMAGE(m) in its mode (csrc/vote_kernels.hip: vote_cap_kernel in front of vote_kernel) against
the contract's equivalence: the capped vote over the lists IS the plain vote over tests/vote_cap_ref.py's blank() of the lists.
Every comparison is bit for bit (ids equal, scores equal as float64 words), every query image is checked, and each result is held
against both sides of the equivalence: the plain references of tests/search_tail_ref.py on the blanked lists, and the library's own
uncapped vote on them.  tests/test_vote_cap_cases.py asserts that the cap bites on these inputs and changes their scores.

The vote's launch regimes (fast, weights in LDS, no weight array, GLOBAL) and k = 3, 17, 64, 113, 200 come from the shapes of
search_tail_ref; the cap kernel's own edges (64 ranks per step, 1024 ranks of a row kept in LDS) from vote_cap_ref.CHUNK_SHAPES."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import search_tail_ref as R
import vote_cap_ref as V

pytestmark = pytest.mark.gpu

WT, COUNT = 0, 1
NAN = float("nan")


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import SegVLADEngine

    assert (_lib.VOTE_WT_BORDA_IM, _lib.VOTE_COUNT, _lib.VOTE_PER_IMAGE_SHIFT) == (WT, COUNT, 8)
    e = SegVLADEngine(0)
    yield e
    e.close()


def _vote(eng, c, n_top, mode=WT, extrema=(NAN, NAN), matches=None, **kw):
    pred, sc = eng.vote(c["matches"] if matches is None else matches, None if (mode & 0xFF) == COUNT else c["sims"], c["off"],
                        n_top=n_top, mode=mode, img_of_seg=c["img_of_seg"], smin=extrema[0], smax=extrema[1], **kw)
    return pred.cpu().numpy(), sc.cpu().numpy()


def _same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    bad = np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))
    assert len(bad) == 0, (what, bad[:5], got[1][tuple(bad[0])], want[1][tuple(bad[0])])


def _check_case(eng, c, caps, tops=(1, 5)):
    """Both bases, every cap, every n_top: the capped vote == the references on blank() == the uncapped vote on blank()."""
    args = (c["off"], c["img_of_seg"])
    for m in caps:
        b = V.blank(c["matches"], c["img_of_seg"], m)
        want = {WT: R.vote_wt_ranking(b, c["sims"], *args), COUNT: R.vote_count_ranking(b, *args)}
        for base in (WT, COUNT):
            for n_top in tops:
                got = _vote(eng, c, n_top, mode=base, per_image=m)
                _same(got, R.padded(want[base], n_top), ("reference", base, m, n_top))
                _same(got, _vote(eng, c, n_top, mode=base, matches=b), ("uncapped on blanked", base, m, n_top))


# ---- parity, per launch regime of the vote ------------------------------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["plain", "invalid_ids"])
@pytest.mark.parametrize("name", V.SHAPES)
def test_parity(eng, name, invalid):
    c = V.case(name, invalid)
    _check_case(eng, c, [1, 2, c["k"]])


# ---- the cap kernel's chunk edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("segs,k", V.CHUNK_SHAPES)
def test_chunk_edges(eng, segs, k):
    c = V.chunk_case(segs, k)
    _check_case(eng, c, [1, 2, 255])
    _check_case(eng, R.with_invalid_ids(c), [1, 3], tops=(5,))


# ---- extrema ------------------------------------------------------------------------------------------------------------
def test_extrema(eng):
    c = V.case("fast_last_64x64", True)
    ext = R.inner_extrema(c["sims"])
    args = (c["sims"], c["off"], c["img_of_seg"], 5)
    for m in (1, 2):
        b = V.blanked("fast_last_64x64", True, m)
        _same(_vote(eng, c, 5, per_image=m, extrema=ext), R.vote_wt(b, *args, *ext), ("explicit", m))
        # computed by the call: over ALL sims of the call, the blanked entries' included -- the uncapped call's extrema
        lo, hi = R.minmax(c["sims"])
        got = _vote(eng, c, 5, per_image=m)
        _same(got, R.vote_wt(b, *args), ("self-computed", m))
        _same(got, _vote(eng, c, 5, per_image=m, extrema=(float(lo), float(hi))), ("self-computed == all sims", m))
    # the extrema of the voting entries alone differ, and so would the scores: the inputs tell the two readings apart
    v = V.blanked("fast_last_64x64", True, 1)
    voting = (v >= 0) & (v < len(c["img_of_seg"]))
    assert c["sims"][voting].min() > c["sims"].min()


# ---- identity and refusals ----------------------------------------------------------------------------------------------
def test_identity_and_refusals(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    c = V.case("wl_first_241x17", True)
    for base in (WT, COUNT):
        plain = _vote(eng, c, 5, mode=base)
        _same(_vote(eng, c, 5, mode=base | (0 << 8)), plain, "PER_IMAGE(0)")
        assert c["k"] <= 255
        _same(_vote(eng, c, 5, mode=base | (255 << 8)), plain, "m = 255 in the mode word")
        _same(_vote(eng, c, 5, mode=base, per_image=255), plain, "m = 255")
    for bad in (2, 1 << 16, 0x100 | 7, (1 << 16) | 0x100, -1):
        with pytest.raises(SegVLADError) as ei:
            _vote(eng, c, 5, mode=bad)
        assert ei.value.code == SEGVLAD_ERR_ARG and "unknown mode" in str(ei.value)
        _same(_vote(eng, c, 5, mode=COUNT, per_image=1), R.vote_count(V.blanked("wl_first_241x17", True, 1), c["off"], c["img_of_seg"], 5),
              "the context stays usable")
    # COUNT without sims: a score is the number of segments that see the image
    pred, sc = eng.vote(c["matches"], None, c["off"], n_top=3, mode=COUNT, img_of_seg=c["img_of_seg"], per_image=1)
    assert sc.cpu().numpy().max() <= max(c["counts"]) and float(sc.cpu().numpy()[1, 0]) == float(int(sc.cpu().numpy()[1, 0]))


# ---- argument forms -----------------------------------------------------------------------------------------------------
def test_argument_forms(eng):
    import async_order

    c = V.case("bench_depth_50x200", True)
    dev = eng.device
    d = dict(matches=torch.from_numpy(c["matches"]).to(dev), sims=torch.from_numpy(c["sims"]).to(dev),
             img=torch.from_numpy(c["img_of_seg"]).to(dev))
    free = async_order.make_engine(False)
    try:
        for base in (WT, COUNT):
            want = _vote(eng, c, 5, mode=base, per_image=2)
            p, s = eng.vote(d["matches"], None if base == COUNT else d["sims"], c["off"], n_top=5, mode=base, img_of_seg=d["img"], per_image=2)
            _same((p.cpu().numpy(), s.cpu().numpy()), want, ("device arguments", base))
            eng.synchronize()                                # (a guarded context: every fence is checked here and after each call)
            _same(_vote(free, c, 5, mode=base, per_image=2), want, ("unguarded context", base))
            p, s = free.vote(d["matches"], None if base == COUNT else d["sims"], c["off"], n_top=5, mode=base, img_of_seg=d["img"], per_image=2)
            _same((p.cpu().numpy(), s.cpu().numpy()), want, ("unguarded context, device arguments", base))
        # a smaller request behind a larger one: the guard's fence follows the request
        small = V.case("nowl_first_2731x3", False)
        _same(_vote(eng, small, 5, per_image=1), R.vote_wt(V.blanked("nowl_first_2731x3", False, 1), small["sims"], small["off"],
                                                            small["img_of_seg"], 5), "smaller request")
    finally:
        free.close()


# ---- the cap is one more launch of the "vote" stage ---------------------------------------------------------------------
def test_launch_count(eng):
    c = V.case("fast_last_64x64", False)
    eng.set_profiling(True)
    try:
        n = {}
        for m in (None, 1):
            eng.profile_reset()
            _vote(eng, c, 5, per_image=m)
            n[m] = eng.stage_ms("vote")[1]
    finally:
        eng.set_profiling(False)
    assert n[1] == n[None] + 1, n


# ---- segvlad_vote_global takes the same bits ----------------------------------------------------------------------------
def test_vote_global_world_1(eng):
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    c = V.case("fast_last_64x64", True)
    e = SegVLADEngine(0)
    try:
        rows = torch.randn((len(c["img_of_seg"]), 64), generator=torch.Generator().manual_seed(3)).to(e.device)
        qs = QueryShardedRetrieval(e, rank=0, world=1, device=e.device, native_comm=True)
        qs.build(rows, c["img_of_seg"])
        assert e.comm_info()["world"] == 1
        for base in (WT, COUNT):
            for m in (1, 2):
                want = _vote(eng, c, 5, mode=base, per_image=m)
                p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, mode=base, img_of_seg=c["img_of_seg"], per_image=m)
                _same((p.cpu().numpy(), s.cpu().numpy()), want, ("vote_global", base, m))
                p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, mode=base | (m << 8), img_of_seg=c["img_of_seg"])
                _same((p.cpu().numpy(), s.cpu().numpy()), want, ("vote_global, bits in the mode", base, m))
        e.comm_destroy()
        p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, img_of_seg=c["img_of_seg"], per_image=1)
        _same((p.cpu().numpy(), s.cpu().numpy()), _vote(eng, c, 5, per_image=1), "no communicator")
    finally:
        e.close()


# ---- pipeline.retrieve(votes_per_image=) --------------------------------------------------------------------------------
def test_pipeline_retrieve(eng):
    from revisit_anything_amd.engine import blank_capped
    from revisit_anything_amd.pipeline import SegVLADPipeline

    rows, img, Q, off = V.revisit_index()
    eng.db_reset()
    eng.db_add(rows, img)
    pipe = SegVLADPipeline(eng, 112, 140)
    n_img = len(off) - 1
    ex = [[(b, b)] for b in range(n_img)]                    # query image b shows place b: its own image is excluded
    for kw in ({}, {"exclude": ex}):
        pred, sc, m, sims = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, votes_per_image=1, **kw)
        p0, s0, m0, sims0 = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, **kw)
        assert torch.equal(m, m0) and torch.equal(sims.view(torch.int32), sims0.view(torch.int32))   # the same search
        b = blank_capped(m, img, 1)
        assert np.array_equal(b, V.blank(m.cpu().numpy(), img, 1)) and (b != m.cpu().numpy()).mean() > 0.05
        ext = (NAN, NAN)
        if kw:
            kept = sims[m >= 0]                              # the filled slots of the lists, blanked entries included
            ext = (float(kept.min()), float(kept.max()))
        wp, ws = eng.vote(b, sims, off, n_top=5, smin=ext[0], smax=ext[1])
        _same((pred.cpu().numpy(), sc.cpu().numpy()), (wp.cpu().numpy(), ws.cpu().numpy()), ("retrieve", sorted(kw)))
        assert not np.array_equal(sc.cpu().numpy(), s0.cpu().numpy())
        if kw:
            assert not (pred.cpu().numpy() == np.arange(n_img)[:, None]).any()
    # COUNT at one vote per image: no score above the image's number of segments
    pred, sc, _, _ = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, mode=COUNT, want_scores=True, votes_per_image=1)
    assert sc.cpu().numpy().max() <= np.diff(off).max()
    # together with the grouped search
    pred, sc, m, sims = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, per_image=2, votes_per_image=1)
    kept = sims[m >= 0]
    wp, ws = eng.vote(blank_capped(m, img, 1), sims, off, n_top=5, smin=float(kept.min()), smax=float(kept.max()))
    _same((pred.cpu().numpy(), sc.cpu().numpy()), (wp.cpu().numpy(), ws.cpu().numpy()), "grouped search and capped vote")
    with pytest.raises(ValueError):
        pipe.retrieve(Q, off, k_search=40, k_vote=20, votes_per_image=0)
