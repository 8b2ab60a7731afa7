"""Grouped search (segvlad_search_grouped, csrc/group_kernels.hip): per query row the nearest index rows with at most per_image
rows of one reference image.  The yardstick is engine.collapse_lists -- the rule on the host -- over an UNBOUNDED ordered list that
existing, unchanged code produces on the device: oracle A, for an index of n <= 1024 rows, is eng.search(Q, n); oracle B, for a
larger one, the full hit list of eng.range_search under an infinite radius (by the header's contract the unbounded search list).
Every comparison is bit for bit on ids and on distance words, and every query row is checked.

One deviation from the issue's text, case 2 at k = 200, per_image = 1: the default depth there is min(1024, 4 k) = 800 < n = 900,
so the fetched lists do NOT reach the index's end and the rows -- fewer than 200 images exist -- are open: the exact tail finishes
them (the result is still checked against oracle A, and tail_rows against the oracle's count of open rows).  The property the issue
names -- tail_rows == 0 because the list reached the index's end -- is asserted at depth 1024 >= n (option group_fetch)."""
import functools

import numpy as np
import pytest
import torch
from conftest import engine_scope

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


@pytest.fixture(scope=engine_scope)
def eng2():
    """The context of the fresh-index comparisons."""
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _check(got, want):
    gd, gi = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    wd, wi = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in want)
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _load(eng, R, img, pieces=None):
    eng.db_reset()
    for a, b in (pieces or [(0, len(R))]):
        eng.db_add(R[a:b], img[a:b])


def _full_lists_a(eng, Q, n):
    """Oracle A's lists: the search at depth n <= 1024 is unbounded."""
    assert n <= 1024
    d2, idx = eng.search(Q, n)
    return d2.cpu().numpy(), idx.cpu().numpy()


def _full_lists_b(eng, Q, n):
    """Oracle B's lists: every row within an infinite radius, [nq][n] (all distances here are finite)."""
    nq = len(Q)
    lims, d2, idx = eng.range_search(Q, INF, capacity=nq * n)
    assert np.array_equal(lims.cpu().numpy(), np.arange(nq + 1, dtype=np.int64) * n)
    return d2.cpu().numpy().reshape(nq, n), idx.cpu().numpy().reshape(nq, n)


def _open_rows(full, img, n, kf, k, m):
    """The oracle's count of rows the head must leave open at depth kf: fewer than k kept among the nearest kf, and the list does
    not cover the index."""
    from revisit_anything_amd.engine import collapse_lists

    if kf >= n:
        return 0
    _, oi = collapse_lists(full[0][:, :kf], full[1][:, :kf], img, k, m)
    return int((oi[:, k - 1] < 0).sum())


# ---- the crowded 900-row index of cases 2, 3, 6, 8, 10 ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crowded900():
    """900 rows, d = 64, 122 images of ragged sizes 1 .. 40, each image's rows small perturbations of one centre.  The 55 one-row
    images sit tightly around a point P, the 2- and 3-row images a little further out, the larger images around random directions.
    Query kinds: `near P` (the nearest 64 rows name >= 50 images), `at a 40- / 21-row image` (the nearest 64 name < 50), random."""
    rng = np.random.default_rng(11)
    d = 64
    sizes = [1, 1, 1, 1, 1, 2, 3, 5, 8, 13, 21, 40] * 9 + [1] * 10 + [2, 3, 5, 7]
    assert sum(sizes) == 900 and 50 < len(sizes) < 200 and max(sizes) == 40
    P = _unit(rng.standard_normal((1, d)))[0]
    sd = np.float32(1.0 / np.sqrt(d))
    rows, img, centres = [], [], []
    for g, s in enumerate(sizes):
        if s == 1:
            c = P + 0.10 * sd * rng.standard_normal(d)
        elif s <= 3:
            c = P + 0.30 * sd * rng.standard_normal(d)
        else:
            c = _unit(rng.standard_normal((1, d)))[0]
        centres.append(c)
        rows.append(c[None, :] + 0.02 * sd * rng.standard_normal((s, d)))
        img += [g] * s
    R = np.concatenate(rows).astype(np.float32)
    img = np.asarray(img, np.int32)
    perm = rng.permutation(900)                          # no image's rows are contiguous
    R, img = np.ascontiguousarray(R[perm]), np.ascontiguousarray(img[perm])
    centres = np.asarray(centres, np.float32)
    big40 = [g for g, s in enumerate(sizes) if s == 40]
    big21 = [g for g, s in enumerate(sizes) if s == 21]

    def queries(nq, seed):
        r = np.random.default_rng(seed)
        kind = np.arange(nq) % 4
        Q = np.empty((nq, d), np.float32)
        for q in range(nq):
            if kind[q] == 0:
                c = P
            elif kind[q] == 1:
                c = centres[big40[q % len(big40)]]
            elif kind[q] == 2:
                c = centres[big21[q % len(big21)]]
            else:
                c = _unit(r.standard_normal((1, d)))[0]
            Q[q] = c + 0.02 * sd * r.standard_normal(d)
        Q[5] = R[17]                                     # an exact duplicate: distance 0
        return Q

    return R, img, queries


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["at_most_3_rows_per_image", "all_distinct"])
def test_identity(eng, ids):
    rng = np.random.default_rng(1)
    n, d = 3000, 256
    R = _unit(rng.standard_normal((n, d)).astype(np.float32))
    if ids == "all_distinct":
        img, m = rng.permutation(n).astype(np.int32), 1
    else:
        img, m = (np.arange(n) % 1000).astype(np.int32), 16   # interleaved: every image has exactly 3 rows
    _load(eng, R, img, [(0, 1000), (1000, 1700), (1700, 3000)])
    Q = _unit(R[rng.integers(0, n, 70)] + 0.05 * rng.standard_normal((70, d)).astype(np.float32))
    for k in (50, 200):
        want = eng.search(Q, k)
        got = eng.search_grouped(Q, k, m)
        _check(got, want)
        st = eng.group_stats()
        assert st["k_fetch"] == 4 * k and st["tail_rows"] == 0 and st["max_read"] == k, st


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case2_queries():
    return _crowded900()[2](70, 21)


@pytest.mark.parametrize("k", [1, 50, 200])
def test_head_on_the_distance_matrix_path(eng, k):
    from revisit_anything_amd.engine import collapse_lists

    R, img, _ = _crowded900()
    Q = _case2_queries()
    _load(eng, R, img)
    full = _full_lists_a(eng, Q, 900)
    for m in (1, 2, 5):
        want = collapse_lists(full[0], full[1], img, k, m)
        got = eng.search_grouped(Q, k, m)
        st = eng.group_stats()
        print("k", k, "per_image", m, st)
        _check(got, want)
        assert st["k_fetch"] == min(1024, 4 * k)
        assert st["tail_rows"] == _open_rows(full, img, 900, st["k_fetch"], k, m)
        gi = got[1].cpu().numpy()
        for q in range(len(Q)):                          # at most m rows of an image per list
            assert np.bincount(img[gi[q][gi[q] >= 0]]).max() <= m
    if k == 200:
        # fewer than 200 images: with per_image = 1 every list ends in (+inf, -1) ...
        got = eng.search_grouped(Q, 200, 1)
        assert (got[1][:, 122:] == -1).all() and torch.isinf(got[0][:, 122:]).all() and (got[1][:, :122] >= 0).all()
        # ... and at a depth that covers the index no row is open: the list reached the index's end
        eng.set_option("group_fetch", 1024)
        try:
            got = eng.search_grouped(Q, 200, 1)
            st = eng.group_stats()
        finally:
            eng.set_option("group_fetch", 0)
        _check(got, collapse_lists(full[0], full[1], img, 200, 1))
        assert st == {"k_fetch": 1024, "tail_rows": 0, "max_read": 900}, st


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [70, 130])
def test_tail_at_its_smallest_shape(eng, nq):
    from revisit_anything_amd.engine import collapse_lists

    R, img, queries = _crowded900()
    Q = _case2_queries() if nq == 70 else queries(130, 31)
    _load(eng, R, img)
    full = _full_lists_a(eng, Q, 900)
    k, m = 50, 1
    want = collapse_lists(full[0], full[1], img, k, m)
    n_open = _open_rows(full, img, 900, 64, k, m)
    print("open rows at depth 64:", n_open, "of", nq)
    assert 0 < n_open < nq                               # both kinds occur
    eng.set_option("group_fetch", 64)
    try:
        got = eng.search_grouped(Q, k, m)
        st = eng.group_stats()
    finally:
        eng.set_option("group_fetch", 0)
    _check(got, want)
    assert st["k_fetch"] == 64 and st["tail_rows"] == n_open, st
    assert 50 <= st["max_read"] <= 64


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _filter_case():
    """40 000 rows (above the 32 768 where the fp16 filter starts), d = 64, 1000 images of 40 near-duplicate rows: even images tight
    around their centre, odd ones loose, so that some lists crowd and others do not."""
    rng = np.random.default_rng(4)
    n, d, per = 40000, 64, 40
    C = _unit(rng.standard_normal((n // per, d)).astype(np.float32))
    spread = np.where(np.arange(n // per) % 2 == 0, 0.02, 0.6).astype(np.float32)
    img = rng.permutation(np.repeat(np.arange(n // per, dtype=np.int32), per))
    R = _unit(C[img] + (spread[img] / np.sqrt(d))[:, None] * rng.standard_normal((n, d)).astype(np.float32))
    c = rng.integers(0, n // per, 130)
    Q = _unit(C[c] + (0.3 / np.sqrt(d)) * rng.standard_normal((130, d)).astype(np.float32))
    return R, img, Q


@pytest.fixture(scope="module")
def filter_lists():
    """Oracle B's lists of the 130 query rows, computed once on a context of their own."""
    from revisit_anything_amd.engine import SegVLADEngine

    R, img, Q = _filter_case()
    e = SegVLADEngine(0)
    try:
        _load(e, R, img)
        return _full_lists_b(e, Q, len(R))
    finally:
        e.close()


@pytest.mark.parametrize("nq", [50, 130])
def test_filter_path(eng, filter_lists, nq):
    from revisit_anything_amd.engine import collapse_lists

    R, img, Q = _filter_case()
    _load(eng, R, img)
    full = (filter_lists[0][:nq], filter_lists[1][:nq])
    k = 50
    for m in (1, 3):
        got = eng.search_grouped(Q[:nq], k, m)
        st = eng.group_stats()
        ss = eng.search_stats()
        print("nq", nq, "per_image", m, st)
        assert ss["filter"] == "f16" and ss["n_queries"] == nq, ss
        _check(got, collapse_lists(full[0][:, :8192], full[1][:, :8192], img, k, m))
        assert st["k_fetch"] == 200 and st["tail_rows"] == _open_rows(full, img, len(R), 200, k, m), st


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_tail_at_the_default_depth_by_construction(eng):
    from revisit_anything_amd.engine import collapse_lists

    rng = np.random.default_rng(5)
    n, d, k = 6000, 64, 300
    e0 = np.zeros(d, np.float32)
    e0[0] = 1
    sd = np.float32(1.0 / np.sqrt(d))
    # image 0: 1500 near-identical rows around -e0; 900 images of 5 unrelated rows each in the half space around +e0
    big = -e0[None, :] + 0.02 * sd * rng.standard_normal((1500, d)).astype(np.float32)
    rest = _unit(rng.standard_normal((4500, d)).astype(np.float32) + 2 * e0[None, :])
    R = np.concatenate([big, rest]).astype(np.float32)
    img = np.concatenate([np.zeros(1500, np.int32), 1 + np.arange(4500, dtype=np.int32) // 5])
    perm = rng.permutation(n)
    R, img = np.ascontiguousarray(R[perm]), np.ascontiguousarray(img[perm])
    qoff = np.array([0, 20, 40, 60, 80])
    Q = np.concatenate([-e0[None, :] + 0.02 * sd * rng.standard_normal((20, d)).astype(np.float32),
                        _unit(rng.standard_normal((60, d)).astype(np.float32) + 2 * e0[None, :])]).astype(np.float32)
    _load(eng, R, img)
    full = _full_lists_b(eng, Q, n)
    assert (img[full[1][:20, :1500]] == 0).all()         # the input's property: image 0's rows are the nearest 1500 of query image 0
    want = collapse_lists(full[0], full[1], img, k, 1)
    head = collapse_lists(full[0][:, :1024], full[1][:, :1024], img, k, 1)[1]
    assert (head[:20, k - 1] < 0).all() and (head[20:, k - 1] >= 0).all()
    got = eng.search_grouped(Q, k, 1)
    st = eng.group_stats()
    _check(got, want)
    assert st["k_fetch"] == 1024 and st["tail_rows"] == qoff[1] - qoff[0], st
    # the other rows were complete in the head: the same bits without any tail
    got2 = eng.search_grouped(Q[20:], k, 1)
    assert eng.group_stats()["tail_rows"] == 0
    _check(got2, (want[0][20:], want[1][20:]))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_negative_image_ids_are_never_collapsed(eng):
    from revisit_anything_amd.engine import collapse_lists

    R, img, _ = _crowded900()
    Q = _case2_queries()
    img = img.copy()
    sizes = np.bincount(img)
    g40, g21 = int(np.nonzero(sizes == 40)[0][0]), int(np.nonzero(sizes == 21)[0][0])
    Q = Q.copy()
    Q[0] = R[np.nonzero(img == g40)[0][0]]               # a query row on top of a row of the 40-row image that turns negative
    img[img == g40] = -1
    img[img == g21] = -7
    img[np.isin(img, np.nonzero(sizes == 1)[0][:6])] = -1
    _load(eng, R, img)
    full = _full_lists_a(eng, Q, 900)
    for fetch in (0, 64):
        eng.set_option("group_fetch", fetch)
        try:
            for k, m in ((50, 1), (50, 2), (200, 1)):
                got = eng.search_grouped(Q, k, m)
                st = eng.group_stats()
                _check(got, collapse_lists(full[0], full[1], img, k, m))
                kf = max(k, fetch) if fetch else 4 * k    # (a forced depth is clamped to k .. 1024)
                assert st["k_fetch"] == kf and st["tail_rows"] == _open_rows(full, img, 900, kf, k, m), st
                if fetch == 64 and k == 50:
                    assert st["tail_rows"] > 0
        finally:
            eng.set_option("group_fetch", 0)
    # every row of the former 40-row image is in query row 0's list of 50, although per_image = 1
    gi = eng.search_grouped(Q, 50, 1)[1].cpu().numpy()
    assert (img[gi[0]] == -1).sum() >= 40


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_lifetime(eng, eng2):
    """add -> add -> db_remove -> add again: after each step the result is that of a fresh context holding the surviving rows (which
    runs at the default depth, while this one is forced through the tail as well)."""
    R, img, _ = _crowded900()
    Q = _case2_queries()

    def same_as_fresh(Rc, imgc):
        _load(eng2, Rc, imgc)
        for k, m in ((50, 1), (200, 2)):
            want = eng2.search_grouped(Q, k, m)
            for fetch in (0, 64):
                eng.set_option("group_fetch", fetch)
                try:
                    _check(eng.search_grouped(Q, k, m), want)
                finally:
                    eng.set_option("group_fetch", 0)

    eng.db_reset()
    eng.db_add(R[:500], img[:500])
    same_as_fresh(R[:500], img[:500])
    eng.db_add(R[500:], img[500:])
    same_as_fresh(R, img)
    sizes = np.bincount(img)
    gone = np.concatenate([np.nonzero(sizes == 40)[0][:3], np.nonzero(sizes == 1)[0][:20], [7, 8]]).astype(np.int32)
    eng.db_remove(img_ids=gone)
    keep = ~np.isin(img, gone)
    same_as_fresh(R[keep], img[keep])
    eng.db_add(R[~keep], img[~keep])
    same_as_fresh(np.concatenate([R[keep], R[~keep]]), np.concatenate([img[keep], img[~keep]]))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_pointers(eng):
    from revisit_anything_amd.engine import collapse_lists

    R, img, _ = _crowded900()
    Q = _case2_queries()
    nq, k = len(Q), 50
    _load(eng, R, img)
    for fetch in (0, 64):
        eng.set_option("group_fetch", fetch)
        try:
            host_q = eng.search_grouped(Q, k, 1)
            dev_q = eng.search_grouped(torch.from_numpy(Q).cuda(), k, 1)
            _check(dev_q, host_q)
            # host outputs
            hd = np.empty((nq, k), np.float32)
            hi = np.empty((nq, k), np.int64)
            eng._stream()
            rc = eng.lib.segvlad_search_grouped(eng._h, Q.ctypes.data, nq, k, 1, hd.ctypes.data, hi.ctypes.data)
            assert rc == 0
            _check((hd, hi), host_q)
            # a device view 4 bytes behind a 16-byte boundary: the yardstick is the search through the SAME view
            buf = torch.empty(nq * 64 + 5, dtype=torch.float32, device="cuda:0")
            off = 1 + (-(buf.data_ptr() // 4) % 4)
            Qv = buf[off:off + nq * 64].view(nq, 64)
            Qv.copy_(torch.from_numpy(Q))
            assert Qv.data_ptr() % 16 == 4 and Qv.is_contiguous()
            full = _full_lists_a(eng, Qv, 900)
            got = eng.search_grouped(Qv, k, 1)
            _check(got, collapse_lists(full[0], full[1], img, k, 1))
            if fetch:
                assert eng.group_stats()["tail_rows"] > 0
        finally:
            eng.set_option("group_fetch", 0)
    # per_image = 16 on an index of small images: segvlad_search on the same pointer, bit for bit
    small = (np.arange(900) % 300).astype(np.int32)
    _load(eng, R, small)
    _check(eng.search_grouped(Qv, k, 16), eng.search(Qv, k))


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_STATE, SegVLADError
    from revisit_anything_amd.engine import collapse_lists

    rng = np.random.default_rng(9)
    R = _unit(rng.standard_normal((200, 64)).astype(np.float32))
    img = np.repeat(np.arange(10, dtype=np.int32), 20)
    Q = np.ascontiguousarray(R[:10] + 0.01)
    d2 = torch.empty((10, 5), dtype=torch.float32, device="cuda:0")
    idx = torch.empty((10, 5), dtype=torch.int64, device="cuda:0")

    def raw(q, nq, k, m, pd, pi):
        return eng.lib.segvlad_search_grouped(eng._h, q, nq, k, m, pd, pi)

    eng.db_reset()                                       # no dimension yet
    with pytest.raises(SegVLADError) as e:
        eng.search_grouped(Q, 5, 1)
    assert e.value.code == SEGVLAD_ERR_STATE
    eng.db_add(R)                                        # no img_of_seg map
    with pytest.raises(SegVLADError) as e:
        eng.search_grouped(Q, 5, 1)
    assert e.value.code == SEGVLAD_ERR_STATE
    _load(eng, R, img)
    before = eng.search(Q, 5)
    qp, dp, ip = Q.ctypes.data, d2.data_ptr(), idx.data_ptr()
    assert raw(qp, -1, 5, 1, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 0, 1, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 1025, 1, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 5, 0, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 5, 17, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(None, 10, 5, 1, dp, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 5, 1, None, ip) == SEGVLAD_ERR_ARG
    assert raw(qp, 10, 5, 1, dp, None) == SEGVLAD_ERR_ARG
    assert raw(None, 0, 5, 1, None, None) == 0           # nq == 0
    assert eng.lib.segvlad_group_stats(eng._h, None, 3) == SEGVLAD_ERR_ARG
    # the context stays usable, and search is unchanged
    after = eng.search(Q, 5)
    _check(after, before)
    full = _full_lists_a(eng, Q, 200)
    for k, m in ((5, 1), (5, 16), (1024, 1)):            # (k beyond the index: padding)
        _check(eng.search_grouped(Q, k, m), collapse_lists(full[0], full[1], img, k, m))
    # an index that removal has emptied
    eng.db_remove(img_ids=np.arange(10, dtype=np.int32))
    d2e, idxe = eng.search_grouped(Q, 5, 1)
    assert (idxe == -1).all() and torch.isinf(d2e).all() and (d2e > 0).all()
    assert eng.group_stats()["tail_rows"] == 0


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def test_twice_in_one_context_gives_identical_bits(eng):
    R, img, queries = _crowded900()
    Q = queries(130, 31)
    _load(eng, R, img)
    runs = []
    for _ in range(2):
        out = []
        for fetch, k, m in ((0, 50, 1), (64, 50, 1), (64, 50, 3), (0, 200, 2)):
            eng.set_option("group_fetch", fetch)
            try:
                d2, idx = eng.search_grouped(Q, k, m)
                out.append((d2.cpu().numpy().view(np.uint32).copy(), idx.cpu().numpy().copy(), eng.group_stats()))
            finally:
                eng.set_option("group_fetch", 0)
        runs.append(out)
    for (a_d, a_i, a_s), (b_d, b_i, b_s) in zip(*runs):
        assert np.array_equal(a_d, b_d) and np.array_equal(a_i, b_i) and a_s == b_s
    assert runs[0][1][2]["tail_rows"] > 0


# ---- 11 -----------------------------------------------------------------------------------------------------------------------
def test_retrieve_one_vote_per_image(eng):
    from revisit_anything_amd.engine import collapse_lists
    from revisit_anything_amd.pipeline import SegVLADPipeline

    R, img, queries = _crowded900()
    Q = queries(80, 41)
    qoff = np.array([0, 20, 20, 50, 80], np.int32)       # an image without segments
    _load(eng, R, img)
    pipe = SegVLADPipeline(eng, 112, 140)
    pred, sc, m, sims = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5, want_scores=True, per_image=1)
    mi = m.cpu().numpy()
    assert (mi >= 0).all()
    for q in range(len(Q)):
        assert len(np.unique(img[mi[q]])) == 25          # every kept list names distinct images
    # the existing vote applied to the oracle's lists
    full = _full_lists_a(eng, Q, 900)
    od, oi = collapse_lists(full[0], full[1], img, 40, 1)
    wsims, wm = eng.sims_from_d2(od, oi, 25)
    assert torch.equal(wm, m) and torch.equal(wsims.view(torch.int32), sims.view(torch.int32))
    kept = wsims[wm >= 0]
    wp, ws = eng.vote(wm, wsims, qoff, n_top=5, want_scores=True, smin=float(kept.min()), smax=float(kept.max()))
    assert torch.equal(pred, wp)
    assert np.array_equal(sc.cpu().numpy().view(np.uint64), ws.cpu().numpy().view(np.uint64))
    # a depth beyond the number of images: the lists end in pads, which must not become the vote's minimum
    pred, sc, m, sims = pipe.retrieve(Q, qoff, k_search=200, k_vote=200, n_top=5, want_scores=True, per_image=1)
    assert (m[:, 122:] == -1).all() and np.isfinite(sc.cpu().numpy()[[0, 2, 3]]).all()
    with pytest.raises(ValueError):
        pipe.retrieve(Q, qoff, k_search=40, k_vote=25, per_image=1, shortlist=[[1]] * 4)
    with pytest.raises(ValueError):
        pipe.retrieve(Q, qoff, k_search=40, k_vote=25, per_image=1, exclude=[[(1, 2)]] * 4)
