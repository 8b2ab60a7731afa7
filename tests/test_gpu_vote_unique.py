"""segvlad_vote with SEGVLAD_VOTE_UNIQUE_REF in its mode (csrc/vote_kernels.hip: vote_unique_*_kernel in front of vote_cap_kernel
and vote_kernel) against the contract's equivalence: the flagged vote over the lists IS the plain vote over
tests/vote_unique_ref.py's blank_unique() of the lists -- with a cap in the same word, over the cap's blank() of those.  Every
comparison is bit for bit (ids equal, scores equal as float64 words), every query image is checked, and each result is held against
both sides of the equivalence: the plain references of tests/search_tail_ref.py on the blanked lists, and the library's own
unflagged vote on them.  tests/test_vote_unique_cases.py asserts that the flag bites on these inputs, that sims decide, that the
order of flag and cap shows, and that the planted ids stress the table as they claim."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import search_tail_ref as R
import vote_cap_ref as V
import vote_unique_ref as U

pytestmark = pytest.mark.gpu

WT, COUNT, FLAG = 0, 1, 0x80
NAN = float("nan")


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import SegVLADEngine

    assert (_lib.VOTE_WT_BORDA_IM, _lib.VOTE_COUNT, _lib.VOTE_UNIQUE_REF) == (WT, COUNT, FLAG)
    e = SegVLADEngine(0)
    yield e
    e.close()


def _vote(eng, c, n_top, mode=WT, extrema=(NAN, NAN), matches=None, sims="by base", **kw):
    """COUNT runs without sims unless they are asked for: the first visited claim wins there."""
    if isinstance(sims, str):
        sims = None if (mode & 0x7F) == COUNT else c["sims"]
    pred, sc = eng.vote(c["matches"] if matches is None else matches, sims, c["off"], n_top=n_top, mode=mode,
                        img_of_seg=c["img_of_seg"], smin=extrema[0], smax=extrema[1], **kw)
    return pred.cpu().numpy(), sc.cpu().numpy()


def _same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    bad = np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))
    assert len(bad) == 0, (what, bad[:5], got[1][tuple(bad[0])], want[1][tuple(bad[0])])


def _check_case(eng, c, caps=(None, 1, 2), tops=(1, 5), blanked=None):
    """Both bases, flag alone and with each cap, every n_top: the flagged vote == the references on the blanked lists == the
    unflagged vote on them.  WT decides by sims; COUNT runs without sims (the first visited wins) and, once, with them."""
    args = (c["off"], c["img_of_seg"])
    for cap in caps:
        for base in (WT, COUNT):
            b = blanked(base == WT, cap) if blanked else U.blank(c, c["sims"] if base == WT else None, cap)
            want = R.vote_wt_ranking(b, c["sims"], *args) if base == WT else R.vote_count_ranking(b, *args)
            for n_top in tops:
                got = _vote(eng, c, n_top, mode=base, unique_ref=True, per_image=cap)
                _same(got, R.padded(want, n_top), ("reference", base, cap, n_top))
                _same(got, _vote(eng, c, n_top, mode=base, matches=b), ("unflagged on blanked", base, cap, n_top))
    b = blanked(True, caps[-1]) if blanked else U.blank(c, c["sims"], caps[-1])
    _same(_vote(eng, c, tops[-1], mode=COUNT, sims=c["sims"], unique_ref=True, per_image=caps[-1]),
          R.padded(R.vote_count_ranking(b, *args), tops[-1]), ("COUNT with sims: they decide", caps[-1]))


# ---- parity, per launch regime of the vote and of the flag --------------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["plain", "invalid_ids"])
@pytest.mark.parametrize("name", U.SHAPES)
def test_parity(eng, name, invalid):
    _check_case(eng, U.case(name, invalid), blanked=lambda use_sims, cap: U.blanked(name, invalid, use_sims, cap))


# ---- special values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.LITERAL_GPU)
def test_literal_lists(eng, name):
    lit = U.LITERAL[name]
    img = np.array([3, 1, 4, 1, 5, 9, 2, 6], np.int32)                  # one image per segment but for segments 1 and 3
    assert len(img) == lit["n_ref"]
    c = dict(matches=lit["matches"], sims=lit["sims"], off=lit["off"], img_of_seg=img)
    ext = (0.0, 2.0)                                                     # (the lists hold NaN and inf: explicit extrema)
    args = (c["off"], img)
    for n_top in (1, 3):
        # (a NaN or inf weight has no reference sum to compare with: the device's own vote over the blanked lists is the other side)
        _same(_vote(eng, c, n_top, mode=WT, extrema=ext, unique_ref=True), _vote(eng, c, n_top, mode=WT, extrema=ext, matches=lit["with_sims"]),
              ("WT", n_top))
        _same(_vote(eng, c, n_top, mode=COUNT, sims=c["sims"], unique_ref=True), R.vote_count(lit["with_sims"], *args, n_top), ("COUNT, sims", n_top))
        _same(_vote(eng, c, n_top, mode=COUNT, unique_ref=True), R.vote_count(lit["without"], *args, n_top), ("COUNT", n_top))
        _same(_vote(eng, c, n_top, mode=COUNT, sims=c["sims"], unique_ref=True, per_image=1),
              R.vote_count(V.blank(lit["with_sims"], img, 1), *args, n_top), ("COUNT, sims, cap", n_top))


# ---- the table's edges and planted hash stress --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.STRESS_KINDS)
@pytest.mark.parametrize("segs,k", U.EDGE_SHAPES)
def test_table_edges_and_stress(eng, segs, k, kind):
    _check_case(eng, U.stress_case(kind, segs, k), caps=(None, 1), tops=(5,))


# ---- identity and refusals ----------------------------------------------------------------------------------------------
def test_identity_and_refusals(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    c = U.no_duplicates_case()
    for base in (WT, COUNT):
        plain = _vote(eng, c, 5, mode=base)
        _same(_vote(eng, c, 5, mode=base | FLAG), plain, "the flag in the mode word, no duplicates")
        _same(_vote(eng, c, 5, mode=base, unique_ref=True), plain, "unique_ref=True, no duplicates")
    # COUNT with sims=None works, and counts every id of an image once
    d = U.case("wl_first_241x17", True)
    pred, sc = eng.vote(d["matches"], None, d["off"], n_top=3, mode=COUNT | FLAG, img_of_seg=d["img_of_seg"])
    _same((pred.cpu().numpy(), sc.cpu().numpy()), R.vote_count(U.blanked("wl_first_241x17", True, False, None), d["off"], d["img_of_seg"], 3),
          "COUNT, sims=None")
    assert sc.cpu().numpy().max() <= R.SEGS_PER_REF                       # an image has that many segments to be claimed
    with pytest.raises(SegVLADError):                                    # the weighted base still needs sims
        eng.vote(d["matches"], None, d["off"], n_top=3, mode=WT | FLAG, img_of_seg=d["img_of_seg"])
    for bad in (2, 1 << 16, 0x100 | 7, (1 << 16) | 0x100, -1, 0x82, 0x80 | 2 | 0x100, (1 << 16) | FLAG):
        with pytest.raises(SegVLADError) as ei:
            _vote(eng, d, 5, mode=bad, sims=d["sims"])
        assert ei.value.code == SEGVLAD_ERR_ARG and "unknown mode" in str(ei.value)
    _same(_vote(eng, d, 5, unique_ref=True), R.vote_wt(U.blanked("wl_first_241x17", True, True, None), d["sims"], d["off"], d["img_of_seg"], 5),
          "the context stays usable")


# ---- extrema ------------------------------------------------------------------------------------------------------------
def test_extrema(eng):
    name = "fast_last_64x64"
    c = U.case(name, True)
    ext = R.inner_extrema(c["sims"])
    args = (c["sims"], c["off"], c["img_of_seg"], 5)
    for cap in (None, 1):
        b = U.blanked(name, True, True, cap)
        _same(_vote(eng, c, 5, unique_ref=True, per_image=cap, extrema=ext), R.vote_wt(b, *args, *ext), ("explicit", cap))
        # computed by the call: over ALL sims of the call, the blanked entries' included -- the unflagged call's extrema
        lo, hi = R.minmax(c["sims"])
        got = _vote(eng, c, 5, unique_ref=True, per_image=cap)
        _same(got, R.vote_wt(b, *args), ("self-computed", cap))
        _same(got, _vote(eng, c, 5, unique_ref=True, per_image=cap, extrema=(float(lo), float(hi))), ("self-computed == all sims", cap))
    # the extrema of the winners alone differ, and so would the scores: the inputs tell the two readings apart
    b = U.blanked(name, True, True, None)
    winners = (b >= 0) & (b < len(c["img_of_seg"]))
    assert c["sims"][winners].min() > c["sims"].min()


# ---- argument forms -----------------------------------------------------------------------------------------------------
def test_argument_forms(eng):
    import async_order

    free = async_order.make_engine(False)
    try:
        for name in ("bench_depth_50x200", "global_first_145x113"):      # the LDS table, and the global one beside it
            c = U.case(name, True)
            dev = eng.device
            d = dict(matches=torch.from_numpy(c["matches"]).to(dev), sims=torch.from_numpy(c["sims"]).to(dev),
                     img=torch.from_numpy(c["img_of_seg"]).to(dev))
            for base in (WT, COUNT):
                want = _vote(eng, c, 5, mode=base, unique_ref=True, per_image=2)
                _same(want, _vote(eng, c, 5, mode=base, matches=U.blanked(name, True, base == WT, 2)), ("host arguments", name, base))
                s = None if base == COUNT else d["sims"]
                p, sc = eng.vote(d["matches"], s, c["off"], n_top=5, mode=base, img_of_seg=d["img"], unique_ref=True, per_image=2)
                _same((p.cpu().numpy(), sc.cpu().numpy()), want, ("device arguments", name, base))
                eng.synchronize()                            # (a guarded context: every fence is checked here and after each call)
                _same(_vote(free, c, 5, mode=base, unique_ref=True, per_image=2), want, ("unguarded context", name, base))
                p, sc = free.vote(d["matches"], s, c["off"], n_top=5, mode=base, img_of_seg=d["img"], unique_ref=True, per_image=2)
                _same((p.cpu().numpy(), sc.cpu().numpy()), want, ("unguarded context, device arguments", name, base))
        # a smaller request behind a larger one: the guard's fences follow the request
        small = U.case("nowl_first_2731x3", False)
        _same(_vote(eng, small, 5, unique_ref=True), R.vote_wt(U.blanked("nowl_first_2731x3", False, True, None), small["sims"], small["off"],
                                                               small["img_of_seg"], 5), "smaller request")
        eng.synchronize()
    finally:
        free.close()


# ---- two calls return the same bytes; an image's row does not depend on its neighbours -----------------------------------
def test_deterministic_and_per_image(eng):
    for kind, segs, k in (("one_id", 64, 64), ("one_id", 241, 17), ("wrap_chain", 145, 113)):   # hundreds of entries on one slot
        c = U.stress_case(kind, segs, k)
        a = _vote(eng, c, 5, unique_ref=True)
        for _ in range(3):
            _same(_vote(eng, c, 5, unique_ref=True), a, ("again", kind, segs))
    for name in ("fast_last_64x64", "global_first_145x113"):
        c = U.case(name, True)
        whole = _vote(eng, c, 5, unique_ref=True, per_image=1, extrema=(0.0, 2.0))
        off = c["off"]
        for b in (0, R.LARGEST, 3):                          # every image alone: another regime mix, other table offsets
            rows = slice(off[b], off[b + 1])
            alone = dict(c, matches=c["matches"][rows], sims=c["sims"][rows], off=np.array([0, off[b + 1] - off[b]], np.int32))
            got = _vote(eng, alone, 5, unique_ref=True, per_image=1, extrema=(0.0, 2.0))
            _same(got, (whole[0][b:b + 1], whole[1][b:b + 1]), ("alone", name, b))


# ---- launches of the "vote" stage ---------------------------------------------------------------------------------------
def test_launch_count(eng):
    eng.set_profiling(True)
    try:
        n = {}
        for name in ("fast_last_64x64", "global_first_145x113"):
            c = U.case(name, False)
            for key, kw in (("plain", {}), ("cap", dict(per_image=1)), ("flag", dict(unique_ref=True)), ("both", dict(unique_ref=True, per_image=1))):
                eng.profile_reset()
                _vote(eng, c, 5, **kw)
                n[name, key] = eng.stage_ms("vote")[1]
            added = U.launch_regime(c["counts"], c["k"])[2]
            assert n[name, "cap"] == n[name, "plain"] + 1                # what tests/test_gpu_vote_cap.py observes: the flag-clear count
            assert n[name, "flag"] == n[name, "plain"] + added and n[name, "both"] == n[name, "cap"] + added, n
        # the header's figures: 1 launch for the images the LDS table holds, 3 more once an image is larger
        assert U.launch_regime(U.case("fast_last_64x64", False)["counts"], 64)[2] == 1
        assert U.launch_regime(U.case("global_first_145x113", False)["counts"], 113)[2] == 4
        big_only = U.stress_case("one_id", 241, 17)
        rows = slice(big_only["off"][1], big_only["off"][2])
        alone = dict(big_only, matches=big_only["matches"][rows], sims=big_only["sims"][rows], off=np.array([0, 241], np.int32))
        for key, kw in (("plain", {}), ("flag", dict(unique_ref=True))):
            eng.profile_reset()
            _vote(eng, alone, 5, **kw)
            n["alone", key] = eng.stage_ms("vote")[1]
        assert n["alone", "flag"] == n["alone", "plain"] + 3, n
    finally:
        eng.set_profiling(False)


# ---- idx and sims written by preceding work on the stream, no synchronisation in between -----------------------------------
def test_stream_order(eng):
    import async_order

    free = async_order.make_engine(False)
    try:
        delay = async_order.Delay(device=str(free.device))
        for name in ("bench_depth_50x200", "global_first_145x113"):
            c = U.case(name, True)
            dev = free.device
            truth_m, truth_s = torch.from_numpy(c["matches"]).to(dev), torch.from_numpy(c["sims"]).to(dev)
            img = torch.from_numpy(c["img_of_seg"]).to(dev)
            want = _vote(free, c, 5, unique_ref=True, per_image=1)        # serial: host operands, synchronised
            m = torch.full_like(truth_m, 7)                               # decoys: every entry on one id, equal sims
            s = torch.full_like(truth_s, 0.5)
            torch.cuda.synchronize()
            delay.enqueue(async_order.MIN_DELAY_MS)
            m.copy_(truth_m, non_blocking=True)                          # behind the delay, on the stream the call will use
            s.copy_(truth_s, non_blocking=True)
            p, sc = free.vote(m, s, c["off"], n_top=5, img_of_seg=img, unique_ref=True, per_image=1)
            _same((p.cpu().numpy(), sc.cpu().numpy()), want, ("delayed inputs", name))
    finally:
        free.close()


# ---- segvlad_vote_global takes the same bit -----------------------------------------------------------------------------
def test_vote_global_world_1(eng):
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    c = U.case("fast_last_64x64", True)
    e = SegVLADEngine(0)
    try:
        rows = torch.randn((len(c["img_of_seg"]), 64), generator=torch.Generator().manual_seed(3)).to(e.device)
        qs = QueryShardedRetrieval(e, rank=0, world=1, device=e.device, native_comm=True)
        qs.build(rows, c["img_of_seg"])
        assert e.comm_info()["world"] == 1
        for base in (WT, COUNT):
            for cap in (None, 1):
                want = _vote(eng, c, 5, mode=base, sims=c["sims"], unique_ref=True, per_image=cap)
                p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, mode=base, img_of_seg=c["img_of_seg"], unique_ref=True,
                                     per_image=cap)
                _same((p.cpu().numpy(), s.cpu().numpy()), want, ("vote_global", base, cap))
                p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, mode=base | FLAG | ((cap or 0) << 8), img_of_seg=c["img_of_seg"])
                _same((p.cpu().numpy(), s.cpu().numpy()), want, ("vote_global, bits in the mode", base, cap))
        e.comm_destroy()
        p, s = e.vote_global(c["matches"], c["sims"], c["off"], n_top=5, img_of_seg=c["img_of_seg"], unique_ref=True)
        _same((p.cpu().numpy(), s.cpu().numpy()), _vote(eng, c, 5, unique_ref=True), "no communicator")
    finally:
        e.close()


# ---- pipeline.retrieve(vote_unique_ref=) --------------------------------------------------------------------------------
def test_pipeline_retrieve(eng):
    from revisit_anything_amd.engine import blank_capped, blank_unique
    from revisit_anything_amd.pipeline import SegVLADPipeline

    rows, img, Q, off = V.revisit_index()
    eng.db_reset()
    eng.db_add(rows, img)
    pipe = SegVLADPipeline(eng, 112, 140)
    n_img = len(off) - 1
    ex = [[(b, b)] for b in range(n_img)]                    # query image b shows place b: its own image is excluded
    for kw in ({}, {"exclude": ex}):
        pred, sc, m, sims = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, vote_unique_ref=True, **kw)
        p0, s0, m0, sims0 = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, **kw)
        assert torch.equal(m, m0) and torch.equal(sims.view(torch.int32), sims0.view(torch.int32))   # the same search
        b = blank_unique(m, sims, off, len(img))
        assert np.array_equal(b, U.blank_unique(m.cpu().numpy(), sims.cpu().numpy(), off, len(img)))
        assert (b != m.cpu().numpy()).sum() >= n_img         # the flag bites: a blanked claim per query image, on average
        ext = (NAN, NAN)
        if kw:
            kept = sims[m >= 0]                              # the filled slots of the lists, blanked entries included
            ext = (float(kept.min()), float(kept.max()))
        wp, ws = eng.vote(b, sims, off, n_top=5, smin=ext[0], smax=ext[1])
        _same((pred.cpu().numpy(), sc.cpu().numpy()), (wp.cpu().numpy(), ws.cpu().numpy()), ("retrieve", sorted(kw)))
        assert not np.array_equal(sc.cpu().numpy(), s0.cpu().numpy())
        if kw:
            assert not (pred.cpu().numpy() == np.arange(n_img)[:, None]).any()
        # with the cap behind it
        pred, sc, m, sims = pipe.retrieve(Q, off, k_search=40, k_vote=20, n_top=5, want_scores=True, vote_unique_ref=True, votes_per_image=1, **kw)
        wp, ws = eng.vote(blank_capped(b, img, 1), sims, off, n_top=5, smin=ext[0], smax=ext[1])
        _same((pred.cpu().numpy(), sc.cpu().numpy()), (wp.cpu().numpy(), ws.cpu().numpy()), ("retrieve, flag and cap", sorted(kw)))
