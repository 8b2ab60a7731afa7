"""Exact range search (segvlad_range_search, csrc/range_kernels.hip): every index row with d2 < radius2 of each query row, the
distances bit for bit those of segvlad_search.  The references are the existing exact search and tests/fp32_emu.py -- never the
new code: at 1 M x 1024 one search(Q, 1024) cut at radii taken from its own lists, elsewhere the full distance matrix assembled
from searches over 1024-row slices of the index (a pair's value does not depend on the index it sits in).  Every row of every
case is compared in full: ids, and the distances' bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch
from conftest import engine_scope

import fp32_emu as E

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = np.float32(-777.25), np.int64(-424242)


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


@pytest.fixture(scope=engine_scope)
def eng2():
    """The context of the reference searches."""
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what):
    """(lims, d2, idx) against (lims, d2, idx): ids and the distances' bit patterns, every row."""
    gl, gd, gi = got
    wl, wd, wi = want
    assert np.array_equal(gl, wl), (what, np.nonzero(gl != wl)[0][:5], gl[:6], wl[:6])
    assert np.array_equal(gi, wi), (what, np.nonzero(gi != wi)[0][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, np.nonzero(gd.view(np.uint32) != wd.view(np.uint32))[0][:5])


def _ref_matrix(ref, R, Q):
    """d2 of every (query row, index row) pair, [nq][n], from searches of `ref` over 1024-row slices of R."""
    n, nq = R.shape[0], Q.shape[0]
    D = np.empty((nq, n), np.float32)
    for a in range(0, n, 1024):
        b = min(n, a + 1024)
        ref.db_reset()
        ref.db_add(R[a:b])
        d2, idx = _np(*ref.search(Q, b - a))
        assert np.array_equal(np.sort(idx, 1), np.broadcast_to(np.arange(b - a), idx.shape))
        np.put_along_axis(D[:, a:b], idx, d2, 1)
    ref.db_reset()
    return D


def _expected(D, radius2):
    """The range result of a distance matrix: per row the entries strictly below its radius, ordered by (d2, id)."""
    nq, n = D.shape
    r = np.broadcast_to(np.asarray(radius2, np.float32), (nq,))
    lims = np.zeros(nq + 1, np.int64)
    dd, ii = [], []
    ids = np.arange(n, dtype=np.int64)
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            hit = np.nonzero((D[q] < r[q]) & (r[q] > 0))[0]
        order = hit[np.lexsort((ids[hit], D[q][hit]))]
        dd.append(D[q][order])
        ii.append(order)
        lims[q + 1] = lims[q] + len(order)
    return lims, np.concatenate(dd).astype(np.float32), np.concatenate(ii).astype(np.int64)


def _radius_for_count(D, counts):
    """Per row a radius with (ties aside) exactly counts[q] rows strictly below it: the counts[q]-th smallest distance
    (0-based), or just above the largest for counts[q] == n."""
    nq, n = D.shape
    S = np.sort(D, 1)
    r = np.empty(nq, np.float32)
    for q in range(nq):
        c = int(counts[q % len(counts)])
        r[q] = np.nextafter(S[q, n - 1], np.float32(np.inf)) if c >= n else S[q, c]
    return r


def _clustered(n, d, nq, seed):
    """Unit rows in 8 tight clusters (thousands of near neighbours per row), queries next to the centres."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((8, d)).astype(np.float32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    R = cen[rng.integers(0, 8, n)] + (0.3 / d ** 0.5) * rng.standard_normal((n, d)).astype(np.float32)
    R = (R / np.linalg.norm(R, axis=1, keepdims=True)).astype(np.float32)
    Q = cen[np.arange(nq) % 8] + (0.3 / d ** 0.5) * rng.standard_normal((nq, d)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    R[n - 5] = R[17]   # an exact duplicate pair
    return np.ascontiguousarray(R), np.ascontiguousarray(Q)


def _check_emulated(Q, R, radius2, got, n_pairs=2000, near=24, seed=0):
    """A sample of the result's (query, row) pairs -- each row's `near` hits closest to its radius among them -- against the
    emulated fp32 chain, bit for bit."""
    lims, d2, idx = got
    nq = len(lims) - 1
    rng = np.random.default_rng(seed)
    pq, pj = [], []
    for q in range(nq):
        a, b = int(lims[q]), int(lims[q + 1])
        if b > a:
            pick = np.unique(np.concatenate([np.arange(max(a, b - near), b), rng.integers(a, b, max(8, n_pairs // nq))]))
            pq.append(np.full(len(pick), q))
            pj.append(pick)
    pq, pj = np.concatenate(pq), np.concatenate(pj)
    assert len(pq) >= n_pairs, len(pq)
    q2, r2 = E.row_sumsq(Q), E.row_sumsq(R)
    emu = E.d2(q2[pq], r2[idx[pj]], E.dot_chain(Q[pq], R[idx[pj]]))
    assert np.array_equal(emu.view(np.uint32), d2[pj].view(np.uint32)), np.nonzero(emu.view(np.uint32) != d2[pj].view(np.uint32))[0][:5]
    r = np.broadcast_to(np.asarray(radius2, np.float32), (nq,))
    assert np.all(d2[pj] < r[pq])
    return len(pq)


# ---- 1. against the search at 1 M x 1024 ------------------------------------------------------------------------------
def test_range_equals_the_cut_search_lists_at_1m(eng):
    from revisit_anything_amd.engine import range_from_topk
    from test_gpu_exact_ids import _data

    R, Q = _data()
    nq = Q.shape[0]
    eng.db_reset()
    eng.db_add(R)
    d2_ref, id_ref = _np(*eng.search(Q, 1024))
    assert id_ref[0, 0] == 123_456 and id_ref[0, 1] == 777_777 and d2_ref[0, 0] == d2_ref[0, 1]   # the planted tie
    cyc = [0, 1, 2, 50, 199, 200, 777, 1000]
    c = np.array([cyc[q % len(cyc)] for q in range(nq)])
    r_at = d2_ref[np.arange(nq), c].copy()                          # radius ON a list value: that entry and its ties are out
    r_up = np.nextafter(r_at, np.float32(np.inf))                   # ... just above it: they are all in
    Q3 = torch.cat([Q, Q, Q]).contiguous()
    for name, r in (("at", r_at), ("above", r_up)):
        want = range_from_topk(d2_ref, id_ref, r)
        assert np.all(np.diff(want[0]) <= 1001)
        got = _np(*eng.range_search(Q, r))
        st = eng.range_stats()
        print(f"[range 1M] radius {name} the list value, 64 rows alone: total {st['total']}, candidates mean {st['cand_sum'] / nq:.0f} "
              f"max {st['cand_max']}, long rows {st['long_rows']}, path {st['path']}")
        _same(got, want, f"single image, radius {name}")
        assert st["path"] == "f16" and st["total"] == want[0][-1]
        assert st["long_rows"] == 0, st
        lims, d2, idx = got
        if name == "at":
            assert lims[1] == 0                                     # row 0's radius sits on the planted tie: both twins out
        else:
            assert lims[1] == 2 and idx[0] == 123_456 and idx[1] == 777_777 and d2[0] == d2[1]   # both in, lower id first
        # the same rows inside a 192-row batch
        gb = _np(*eng.range_search(Q3, np.concatenate([r, r, r])))
        stb = eng.range_stats()
        print(f"[range 1M] radius {name}, 192-row batch: candidates mean {stb['cand_sum'] / (3 * nq):.0f} max {stb['cand_max']}, "
              f"long rows {stb['long_rows']}")
        assert stb["path"] == "f16" and stb["long_rows"] == 0, stb
        n1 = int(lims[-1])
        assert np.array_equal(gb[0][:nq + 1], lims) and np.array_equal(gb[0][nq:2 * nq + 1] - n1, lims)
        for rep in range(3):
            assert np.array_equal(gb[2][rep * n1:(rep + 1) * n1], idx)
            assert np.array_equal(gb[1][rep * n1:(rep + 1) * n1].view(np.uint32), d2.view(np.uint32))
        # the exact path gives the same bits
        eng.set_option("knn_filter", "fp32")
        try:
            gf = _np(*eng.range_search(Q, r))
            assert eng.range_stats()["path"] == "exact"
        finally:
            eng.set_option("knn_filter", "auto")
        _same(gf, got, f"knn_filter = fp32, radius {name}")
    eng.db_reset()


# ---- 2. long rows and the exact path against distances that do not come from the new code --------------------------
def test_long_rows_against_the_sliced_reference(eng, eng2):
    n, d, nq = 40_000, 128, 64
    R, Q = _clustered(n, d, nq, 11)
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    D = _ref_matrix(eng2, Rt, Qt)
    eng.db_reset()
    eng.db_add(Rt)
    r_counts = _radius_for_count(D, [0, 1, 8191, 8192, 8193, 9000, 20_000, n])
    n_checked = 0
    for name, r in (("per-row counts", r_counts), ("one scalar", np.float32(np.median(D))), ("+inf", np.float32(np.inf))):
        want = _expected(D, r)
        got = _np(*eng.range_search(Qt, r))
        st = eng.range_stats()
        print(f"[range long] {name}: total {st['total']}, long rows {st['long_rows']}, candidates max {st['cand_max']}, path {st['path']}")
        _same(got, want, name)
        assert st["path"] == "f16" and st["total"] == want[0][-1]
        if name == "per-row counts":
            counts = np.diff(want[0])
            assert (counts > 8192).sum() >= nq // 8 * 4 and st["long_rows"] >= int((counts > 8192).sum()) >= 1, (st, counts[:8])
        if name == "+inf":
            assert st["long_rows"] == nq and want[0][-1] == nq * n
        n_checked += _check_emulated(Q, R, r, got)
        # the exact path on the same index
        eng.set_option("knn_filter", "fp32")
        try:
            gf = _np(*eng.range_search(Qt, r))
            assert eng.range_stats()["path"] == "exact"
        finally:
            eng.set_option("knn_filter", "auto")
        _same(gf, want, name + " (knn_filter = fp32)")
    print(f"[range long] {n_checked} (query, row) pairs equal the emulated fp32 chain bit for bit")
    eng.db_reset()


# ---- 3. exact-path shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(5000, 128), (40_000, 100)])
def test_exact_path_shapes(eng, eng2, n, d):
    nq = 64
    R, Q = _clustered(n, d, nq, 23 + d)
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    D = _ref_matrix(eng2, Rt, Qt)
    eng.db_reset()
    eng.db_add(Rt)
    for name, r in (("per-row counts", _radius_for_count(D, [0, 1, 2, 50, 700, 3000, n - 1, n])), ("one scalar", np.float32(np.median(D)))):
        want = _expected(D, r)
        got = _np(*eng.range_search(Qt, r))
        st = eng.range_stats()
        _same(got, want, name)
        assert st["path"] == "exact" and st["total"] == want[0][-1] and st["long_rows"] == nq
        _check_emulated(Q, R, r, got, n_pairs=1000)
    eng.db_reset()


# ---- 4. the capacity protocol -----------------------------------------------------------------------------------------
def _raw(eng, q, r, lims, d2, idx, capacity):
    from revisit_anything_amd.engine import _ptr

    total = C.c_int64(-1)
    eng._stream()
    rc = eng.lib.segvlad_range_search(eng._h, _ptr(q), q.shape[0], _ptr(r), _ptr(lims), _ptr(d2), _ptr(idx), capacity, C.byref(total))
    torch.cuda.synchronize()
    return rc, int(total.value)


def test_capacity_protocol_and_host_pointers(eng, eng2):
    n, d, nq = 40_000, 128, 64
    R, Q = _clustered(n, d, nq, 31)
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    D = _ref_matrix(eng2, Rt, Qt)
    eng.db_reset()
    eng.db_add(Rt)
    r = _radius_for_count(D, [0, 3, 100, 2000, 9000, 1, 17, 5])
    want = _expected(D, r)
    total = int(want[0][-1])
    rt = torch.from_numpy(r).cuda()

    def bufs(cap):
        return (torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((cap,), float(SENT_F), dtype=torch.float32, device="cuda"),
                torch.full((cap,), int(SENT_I), dtype=torch.int64, device="cuda"))

    # one slot short: OK, true counts, buffers untouched
    lims, d2, idx = bufs(total - 1)
    rc, tot = _raw(eng, Qt, rt, lims, d2, idx, total - 1)
    assert rc == 0 and tot == total and np.array_equal(lims.cpu().numpy(), want[0])
    assert bool((d2 == float(SENT_F)).all()) and bool((idx == int(SENT_I)).all())
    # exactly enough, and more than enough: filled, the slots beyond untouched
    for cap in (total, total + 1000):
        lims, d2, idx = bufs(cap)
        rc, tot = _raw(eng, Qt, rt, lims, d2, idx, cap)
        assert rc == 0 and tot == total
        _same(_np(lims, d2[:total], idx[:total]), want, f"capacity {cap}")
        assert bool((d2[total:] == float(SENT_F)).all()) and bool((idx[total:] == int(SENT_I)).all())
    # count only
    lims = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    rc, tot = _raw(eng, Qt, rt, lims, None, None, 0)
    assert rc == 0 and tot == total and np.array_equal(lims.cpu().numpy(), want[0])
    # host pointers for every argument: the same bits; and untouched when short
    hl, hd, hi = np.full(nq + 1, -1, np.int64), np.full(total + 7, SENT_F, np.float32), np.full(total + 7, SENT_I, np.int64)
    rc, tot = _raw(eng, Q, r, hl, hd, hi, total + 7)
    assert rc == 0 and tot == total
    _same((hl, hd[:total], hi[:total]), want, "host pointers")
    assert np.all(hd[total:] == SENT_F) and np.all(hi[total:] == SENT_I)
    hl, hd, hi = np.full(nq + 1, -1, np.int64), np.full(total - 1, SENT_F, np.float32), np.full(total - 1, SENT_I, np.int64)
    rc, tot = _raw(eng, Q, r, hl, hd, hi, total - 1)
    assert rc == 0 and tot == total and np.array_equal(hl, want[0]) and np.all(hd == SENT_F) and np.all(hi == SENT_I)
    # bad arguments
    lims, d2, idx = bufs(4)
    assert _raw(eng, Qt, rt, lims, d2, idx, -1)[0] == -1
    assert _raw(eng, Qt, rt, None, d2, idx, 4)[0] == -1
    assert _raw(eng, Qt, rt, lims, None, idx, 4)[0] == -1
    assert _raw(eng, Qt, None, lims, d2, idx, 4)[0] == -1
    # the engine's retry: a first offer that is too small is repeated once at the reported total
    got = _np(*eng.range_search(Qt, r, capacity=5))
    assert eng.range_retried
    _same(got, want, "engine retry")
    got = _np(*eng.range_search(Qt, r))   # (default capacity: the previous total)
    assert not eng.range_retried
    _same(got, want, "engine, remembered capacity")
    eng.db_reset()


# ---- 5. degenerate input ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40_000, 3000])
def test_degenerate_radii_and_queries(eng, eng2, n):
    d, nq = 128, 16
    R, Q = _clustered(n, d, nq, 41)
    Q[5, 7] = np.nan                                     # a NaN query row: no hit, the other rows unharmed
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    Qclean = Q.copy()
    Qclean[5] = Q[4]
    D = _ref_matrix(eng2, Rt, torch.from_numpy(Qclean).cuda())
    med = np.float32(np.median(D))
    r = np.full(nq, med, np.float32)
    r[0], r[1], r[2], r[3] = np.nan, 0.0, -1.0, -np.inf
    eng.db_reset()
    eng.db_add(Rt)
    want_r = r.copy()
    want_r[5] = 0.0                                      # (the NaN row: nothing)
    want = _expected(D, want_r)
    got = _np(*eng.range_search(Qt, r))
    _same(got, want, "degenerate")
    assert np.all(np.diff(got[0])[:4] == 0) and np.diff(got[0])[5] == 0 and np.diff(got[0])[6] > 0
    # the same radii without the NaN query: the filter path where the index is large enough
    r2 = r.copy()
    got2 = _np(*eng.range_search(torch.from_numpy(Qclean).cuda(), r2))
    _same(got2, _expected(D, r2), "degenerate radii")
    assert eng.range_stats()["path"] == ("f16" if n > 32768 else "exact")
    # nq == 0
    lims, d2, idx = eng.range_search(Qt[:0], np.zeros(0, np.float32))
    assert lims.cpu().tolist() == [0] and d2.numel() == 0 and idx.numel() == 0
    # an index emptied by removal keeps its dimension: all-zero lims
    eng.db_remove(row_ids=np.arange(n, dtype=np.int64))
    assert eng.db_size() == (0, d)
    lims, d2, idx = eng.range_search(Qt, np.float32(np.inf))
    assert lims.cpu().tolist() == [0] * (nq + 1) and d2.numel() == 0
    eng.db_reset()


def test_no_dimension_is_a_state_error():
    from revisit_anything_amd.engine import SegVLADEngine, SegVLADError

    e = SegVLADEngine(0)
    try:
        with pytest.raises(SegVLADError) as ei:
            e.range_search(torch.zeros(2, 64, device="cuda"), 1.0)
        assert ei.value.code == -3   # SEGVLAD_ERR_STATE
    finally:
        e.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------
def test_range_over_an_index_lifetime(eng, eng2):
    n, d, nq, S = 48_000, 128, 32, 40
    R, Q = _clustered(n, d, nq, 51)
    img = (np.arange(n) // S).astype(np.int32)
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    r = np.float32(0.25)
    eng.db_reset()
    cuts = [0, 7001, 7002, 36_000]
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.db_add(Rt[a:b], img[a:b])
    eng.range_search(Qt, r)                                # (the planes exist before the removal)
    gone_img = np.array([3, 600], np.int32)
    gone_rows = np.array([5, 999, 20_000, 35_999], np.int64)
    eng.db_remove(row_ids=gone_rows, img_ids=gone_img)
    eng.db_add(Rt[36_000:], img[36_000:])
    keep = np.ones(n, bool)
    keep[gone_rows] = False
    keep[np.isin(img, gone_img)] = False
    a = _np(*eng.range_search(Qt, r))
    b = _np(*eng.range_search(Qt, r))
    _same(b, a, "two consecutive calls")
    assert eng.range_stats()["path"] == "f16"
    eng2.db_reset()
    eng2.db_add(torch.from_numpy(np.ascontiguousarray(R[keep])).cuda(), img[keep])
    _same(a, _np(*eng2.range_search(Qt, r)), "fresh engine with the surviving rows")
    assert a[0][-1] > 0
    D = _ref_matrix(eng2, torch.from_numpy(np.ascontiguousarray(R[keep])).cuda(), Qt)
    _same(a, _expected(D, r), "sliced reference")
    eng.db_reset()


# ---- 7. the stage timer, and no state left behind ----------------------------------------------------------------------
def test_stage_timer_and_a_following_search(eng, eng2):
    n, d, nq = 40_000, 128, 50
    R, Q = _clustered(n, d, nq, 61)
    Rt, Qt = torch.from_numpy(R).cuda(), torch.from_numpy(Q).cuda()
    eng2.db_reset()
    eng2.db_add(Rt)
    want = _np(*eng2.search(Qt, 20))                       # a context that never ran a range search on this index
    eng.db_reset()
    eng.db_add(Rt)
    eng.set_profiling(True)
    eng.profile_reset()
    eng.range_search(Qt, np.float32(0.2))
    ms, launches = eng.stage_ms("knn_range")
    eng.set_profiling(False)
    print(f"[range] stage knn_range: {ms:.3f} ms, {launches} launches")
    assert launches > 0 and ms > 0
    got = _np(*eng.search(Qt, 20))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    eng.db_reset()
    eng2.db_reset()
