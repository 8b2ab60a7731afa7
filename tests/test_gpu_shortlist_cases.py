"""segvlad_search_shortlist and the image -> row map over the shape table of tests/shortlist_cases.py: one case per branch of the
host arithmetic (MT, the slice rule, the buffer size, the final sort, the union kernel's size) and of the kernels' bookkeeping
(mid-loop cuts, cuts inside tie runs, the map's LDS sort / ordered scan / early return).  tests/test_shortlist_cases.py proves on
the CPU what every case reaches; here every case builds a FRESH context, adds the index in the case's db_add calls and is held
against the host brute force of the emulated fp32 chain (tests/fp32_emu.py) -- ids equal, distances equal as uint32 -- once
through a host shortlist and once through a device shortlist.

The shortlist search orders by key at the end, so it sees a missing or duplicated row of the map but not a wrong ORDER; that is
what segvlad_match_pairs sees ((distance, position) must order like (distance, row id)), so the large images go through it too,
and through the exact tail of segvlad_search_excluding, whose ranges are map positions.

Run with `-m gpu` on an MI355X."""
import time

import numpy as np
import pytest
import torch

import shortlist_cases as T
from match_ref import _yardstick

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _query_view(Q, offset):
    """Q [nq, d] (NumPy) as a contiguous device view `offset` floats past a 16-byte boundary."""
    nq, d = Q.shape
    buf = torch.empty(nq * d + 8, dtype=torch.float32, device="cuda:0")
    off = offset + (-(buf.data_ptr() // 4) % 4)
    Qv = buf[off:off + nq * d].view(nq, d)
    Qv.copy_(torch.tensor(Q))
    assert Qv.data_ptr() % 16 == 4 * offset and Qv.is_contiguous()
    return Qv


def _add(eng, x):
    for a, b in x["splits"]:
        eng.db_add(x["R"][a:b], x["img"][a:b])


def _check(got, want):
    gd, gi = (t.cpu().numpy() for t in got)
    wd, wi = want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), np.argwhere(gd.view(np.uint32) != wd.view(np.uint32))[:5]


@pytest.mark.parametrize("c", T.CASES, ids=[c.name for c in T.CASES])
def test_shortlist_case(eng, c):
    x = T.make_data(c.data)
    want = T.brute(c)                                   # (shared by the cases on the same data; never written to)
    t0 = time.perf_counter()
    _add(eng, x)
    Qv = _query_view(x["Q"], c.q_offset)
    # a host shortlist (and host queries, unless the case is about the device view), then a device shortlist: the same bits
    host = eng.search_shortlist(Qv if c.q_offset else x["Q"], x["qoff"], x["sl"], c.k)
    _check(host, want)
    dev = eng.search_shortlist(Qv, x["qoff"], torch.tensor(x["sl"]).cuda(), c.k)
    assert torch.equal(dev[1], host[1]) and torch.equal(dev[0].view(torch.int32), host[0].view(torch.int32))
    _check(dev, want)
    p = T.plan(c)
    print(f"{c.name}: MT {p['MT']} S {p['S']} cap {p['cap']} np2 {p['np2']}: two searches of {x['Q'].shape[0]} rows, "
          f"{time.perf_counter() - t0:.2f} s on the device's side")


def test_large_images_through_match_pairs(eng):
    """The ordered scan leaves the rows of the 4097- and 9000-row images ascending: query rows that are exact copies of a pair of
    identical rows inside such an image have a tie for their nearest column, which match_pairs decides by POSITION in the map --
    the yardstick by row id."""
    from test_gpu_match import _check as check_match

    x = T.make_data("large")
    R, img, Q, qoff = x["R"], x["img"], np.ascontiguousarray(x["Q"][:40]), np.ascontiguousarray(x["qoff"][:3])
    cand = np.array([[T.LARGE_A, T.LARGE_B, 3], [T.LARGE_B, T.LARGE_A, -1]], np.int32)
    want = _yardstick(Q, R, img, qoff, cand, np.inf)
    # the planted ties: the first six rows of either query image equal two rows of its first candidate, rows 10 .. 15 two of its second
    for b, lo, slot, g in ((0, 0, 0, T.LARGE_A), (1, 20, 0, T.LARGE_B), (0, 10, 1, T.LARGE_B), (1, 30, 1, T.LARGE_A)):
        for q in range(lo, lo + T.LARGE_PAIRS):
            twins = np.nonzero((R == Q[q]).all(1))[0]
            assert len(twins) == 2 and (img[twins] == g).all() and want["fwd_idx"][q, slot] == twins.min()
    _add(eng, x)
    got = eng.match_pairs(Q, qoff, cand, want_rows=True)
    check_match(got, want)
    # the forward half against the shortlist search on the same map
    for j in range(cand.shape[1]):
        d2, idx = eng.search_shortlist(Q, qoff, np.ascontiguousarray(cand[:, j:j + 1]), 1)
        assert torch.equal(idx[:, 0], got["fwd_idx"][:, j]) and torch.equal(d2[:, 0].view(torch.int32), got["fwd_d2"][:, j].view(torch.int32))


def _crowded_large(rng, d, nq):
    """test_gpu_exclude._crowded with one image of 4097 rows outside the cluster and every row shuffled: the images 40 .. 79 (2000
    rows) and all query rows in one tight cluster, the rest random -- 70 images of 50 rows and image 5 with 4097."""
    counts = np.full(120, 50)
    counts[5] = T.SL_SORT_CAP + 1
    img = rng.permutation(np.repeat(np.arange(120, dtype=np.int32), counts)).astype(np.int32)
    R = rng.standard_normal((len(img), d)).astype(np.float32)
    c = T._unit(rng.standard_normal((1, d)).astype(np.float32))
    sig = np.float32(0.24 / np.sqrt(d))
    inside = (img >= 40) & (img < 80)
    R[inside] = c + sig * rng.standard_normal((int(inside.sum()), d)).astype(np.float32)
    Q = c + sig * rng.standard_normal((nq, d)).astype(np.float32)
    return T._unit(R), img, T._unit(Q)


def test_large_image_through_the_exclusion_tail(eng):
    """The exact tail of segvlad_search_excluding walks ranges of map POSITIONS: with a 4097-row image in the allowed part, a window
    over the 2000 rows that crowd every query row's nearest 1024 sends every row through the tail, which must return what a fresh
    index without the window's images returns, and the emulated brute force."""
    from revisit_anything_amd.engine import SegVLADEngine
    from test_gpu_exclude import _brute as brute_excluding, _emu_d2, _excluded, _fresh

    rng = np.random.default_rng(17)
    nq, k = 50, 50
    R, img, Q = _crowded_large(rng, 32, nq)
    assert (img == 5).sum() == T.SL_SORT_CAP + 1 and len(img) % 256 != 0
    qoff = np.array([0, nq], np.int32)
    ex = np.array([[[40, 79]]], np.int32)
    D = _emu_d2(Q, R)
    near = np.argsort(D, axis=1, kind="stable")[:, :1024]
    allowed = ~_excluded(img, ex[0])
    assert allowed[near].sum() == 0 and allowed[img == 5].all() and 2000 > 1024 - k
    want = brute_excluding(D, img, qoff, ex, k)
    assert (img[want[1]] == 5).sum() > nq                # the large image's rows are part of the answer
    adds = [(0, 3000), (3000, 7001), (7001, len(R))]
    for a, b in adds:
        eng.db_add(R[a:b], img[a:b])
    got = eng.search_excluding(Q, qoff, ex, k)
    st = eng.exclude_stats()
    assert st["k_fetch"] == 1024 and st["x_max"] == 2000 and st["tail_rows"] == nq, st      # EVERY row went through the tail
    _check(got, want)
    eng2 = SegVLADEngine(0)
    try:
        _check(got, _fresh(eng2, R, img, Q, qoff, ex, k, adds))
    finally:
        eng2.close()


def test_width_that_is_no_multiple_of_32_is_a_limit(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    rng = np.random.default_rng(48)
    R = T._unit(rng.standard_normal((200, 48)).astype(np.float32))
    img = np.repeat(np.arange(10, dtype=np.int32), 20)
    Q = T._unit(R[:10] + 0.1 * rng.standard_normal((10, 48)).astype(np.float32))
    eng.db_add(R, img)
    with pytest.raises(SegVLADError) as e:
        eng.search_shortlist(Q, np.array([0, 10], np.int32), np.array([[1, 2]], np.int32), 5)
    assert e.value.code == SEGVLAD_ERR_LIMIT and "d=48" in str(e.value), str(e.value)
    # the context stays usable: the plain search (every width) answers as the float64 ranking does
    d2, idx = eng.search(Q, 5)
    D = ((Q.astype(np.float64)[:, None, :] - R.astype(np.float64)[None, :, :]) ** 2).sum(2)
    o = np.argsort(D, axis=1, kind="stable")[:, :5]
    gaps = np.diff(np.sort(D, axis=1)[:, :6], axis=1)
    assert gaps.min() > 1e-4                             # (the data's property: no neighbour is contested)
    assert np.array_equal(idx.cpu().numpy(), o) and np.abs(d2.cpu().numpy() - np.take_along_axis(D, o, 1)).max() < 1e-5
