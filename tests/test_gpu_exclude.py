"""Search excluding image-id windows per query image (segvlad_search_excluding, csrc/exclude_kernels.hip): per query row the
exact top-k over the rows whose image id lies in none of its query image's intervals.  Every distance is the device's exact
fp32 chain (tests/fp32_emu.py), so everything is compared BIT for bit: against segvlad_search when nothing is excluded, against
a FRESH index from which the window's images were removed (ids mapped back through db_remove's new_id), and against a host
brute force of the emulated chain ordered by (distance, id)."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import fp32_emu as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


@pytest.fixture(scope=engine_scope)
def eng2():
    """The context of the fresh-index oracle."""
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _emu_d2(Q, R):
    """The emulated fp32 distance of every (query row, index row) pair, [nq][n]."""
    Q, R = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(R, np.float32)
    qn, rn = E.row_sumsq(Q), E.row_sumsq(R)
    RT = np.ascontiguousarray(R.T)
    acc = np.zeros((Q.shape[0], R.shape[0]), np.float32)
    for j in range(R.shape[1]):
        acc = E.fma32(Q[:, j:j + 1], RT[j][None, :], acc)
    return E.d2(qn[:, None], rn[None, :], acc)


def _excluded(img, ivs):
    """Rows (bool [n]) whose image id lies in one of the inclusive intervals; a row with a negative image id is never excluded."""
    m = np.zeros(len(img), bool)
    for lo, hi in np.asarray(ivs, np.int64).reshape(-1, 2):
        m |= (img >= lo) & (img <= hi)
    return m & (img >= 0)


def _brute_near(Q, R, img, ivs, k, margin=2e-4):
    """_brute for a LARGE index (unit rows, d <= 256), where emulating every pair is out of reach: the rows that can be among a
    query row's k nearest allowed rows are picked in float64 -- those within `margin` of the k-th smallest float64 distance --
    and only they are emulated and ordered.  The fp32 chain is within d 2^-24 sum|q_i r_i| <= 1.6e-5 of the exact dot product
    (d = 256, unit rows), the distance within 3.2e-5 + the norms' 1e-6; a row left out lies more than margin - 3.3e-5 above the
    k-th float64 distance in fp32, every one of the k rows at or below it at most 3.3e-5 above: margin > 6.6e-5 suffices."""
    allowed = np.nonzero(~_excluded(img, ivs))[0]
    qn, rn = E.row_sumsq(Q), E.row_sumsq(R[allowed])
    D64 = (Q.astype(np.float64) ** 2).sum(1)[:, None] + (R[allowed].astype(np.float64) ** 2).sum(1)[None, :] \
        - 2.0 * Q.astype(np.float64) @ R[allowed].astype(np.float64).T
    d2 = np.full((len(Q), k), np.inf, np.float32)
    ids = np.full((len(Q), k), -1, np.int64)
    for q in range(len(Q)):
        c = np.nonzero(D64[q] <= np.partition(D64[q], k - 1)[k - 1] + margin)[0]
        dd = E.d2(qn[q], rn[c], E.dot_chain(Q[q], R[allowed[c]]))
        o = np.lexsort((allowed[c], dd))[:k]
        d2[q], ids[q] = dd[o], allowed[c][o]
    return d2, ids


def _brute(D, img, qoff, excl, k):
    """Host reference from the emulated distance matrix D: per query row the allowed rows in (distance, id) order, (+inf, -1)
    padding."""
    nq = D.shape[0]
    d2 = np.full((nq, k), np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    for b in range(len(qoff) - 1):
        allowed = np.nonzero(~_excluded(img, excl[b]))[0]
        for q in range(qoff[b], qoff[b + 1]):
            dd = D[q, allowed]
            o = np.lexsort((allowed, dd))[:k]
            d2[q, :len(o)] = dd[o]
            ids[q, :len(o)] = allowed[o]
    return d2, ids


def _fresh(eng2, R, img, Q, qoff, excl, k, adds=None):
    """The oracle: per query image, a fresh index of the same rows with the window's images removed, searched with the image's
    rows alone; ids mapped back through new_id."""
    nq = Q.shape[0]
    d2 = np.full((nq, k), np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    for b in range(len(qoff) - 1):
        if qoff[b + 1] == qoff[b]:
            continue
        eng2.db_reset()
        for a0, a1 in (adds or [(0, len(R))]):
            eng2.db_add(R[a0:a1], img[a0:a1])
        window = np.unique(img[_excluded(img, excl[b])]).astype(np.int32)
        old_of_new = np.arange(len(R))
        if len(window):
            _, new_id = eng2.db_remove(img_ids=window, want_new_ids=True)
            old_of_new = np.nonzero(new_id.cpu().numpy() >= 0)[0]
        fd, fi = eng2.search(Q[qoff[b]:qoff[b + 1]], k)
        fd, fi = fd.cpu().numpy(), fi.cpu().numpy()
        d2[qoff[b]:qoff[b + 1]] = fd
        ids[qoff[b]:qoff[b + 1]] = np.where(fi >= 0, old_of_new[np.maximum(fi, 0)] if len(old_of_new) else -1, -1)
    return d2, ids


def _check(got, want):
    gd, gi = (t.cpu().numpy() for t in got)
    wd, wi = want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _empty(n_img, e=1):
    x = np.zeros((n_img, e, 2), np.int32)
    x[:, :, 1] = -1
    return x


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["20000x1024", "3000x256_three_adds", "300x64_smaller_than_k"])
def test_no_exclusion_is_the_plain_search(eng, geometry):
    rng = np.random.default_rng(1)
    if geometry == "20000x1024":
        n, d, per = 20000, 1024, 50
        R = _unit(rng.standard_normal((n, d)).astype(np.float32))
        img = np.repeat(np.arange(n // per, dtype=np.int32), per)
        eng.db_reset()
        eng.db_add(R, img)
    elif geometry == "300x64_smaller_than_k":
        n, d = 300, 64
        R = _unit(rng.standard_normal((n, d)).astype(np.float32))
        img = (np.arange(n) // 7).astype(np.int32)
        eng.db_reset()
        eng.db_add(R, img)
    else:
        n, d = 3000, 256
        R = _unit(rng.standard_normal((n, d)).astype(np.float32))
        img = (np.arange(n) % 37).astype(np.int32) * 2   # interleaved: no image's rows are contiguous; odd ids carry no row
        eng.db_reset()
        for a, b in ((0, 1000), (1000, 1700), (1700, 3000)):
            eng.db_add(R[a:b], img[a:b])
    top = int(img.max())
    qoff = np.array([0, 50, 50, 180, 230], np.int32)   # an image without segments, one with 130
    Q = _unit(R[rng.integers(0, n, qoff[-1])] + 0.05 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    Q[7] = R[11]                                        # an exact duplicate: distance 0
    nothing = _empty(4, 3)
    no_rows = _empty(4, 3)                              # intervals over ids no row carries
    no_rows[:, 0] = (top + 1, top + 1000)
    no_rows[:, 1] = (-50, -1)
    if geometry == "3000x256_three_adds":
        no_rows[:, 2] = (5, 5)
    for k in (1, 50, 200, 1024):
        want = eng.search(Q, k)
        for ex in (nothing, no_rows):
            got = eng.search_excluding(Q, qoff, ex, k)
            assert torch.equal(got[1], want[1])
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
            st = eng.exclude_stats()
            assert st["tail_rows"] == 0 and st["x_max"] == 0 and st["k_fetch"] == k and st["n_img_excluding"] == 0
        if k > n:
            assert (got[1][:, n:] == -1).all() and torch.isinf(got[0][:, n:]).all()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _oracle_case():
    rng = np.random.default_rng(2)
    d, per, n_ref_img = 64, 30, 100
    R = _unit(rng.standard_normal((per * n_ref_img, d)).astype(np.float32))
    img = np.repeat(np.arange(n_ref_img, dtype=np.int32), per)
    img[img == 5] = 120                                 # image 5 has no rows; 120 has them, 100 .. 119 have none
    # planted exact ties that straddle the edge of query image 0's window [10, 12]: one copy inside (image 12), two outside in
    # different images (13, 40)
    R[13 * per + 5] = R[12 * per + 3]
    R[40 * per + 1] = R[12 * per + 3]
    qoff = np.array([0, 30, 30, 160, 170, 220], np.int32)   # an image with 0 rows, one with 130
    Q = _unit(R[rng.integers(0, len(R), qoff[-1])] + 0.2 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    Q[0] = R[12 * per + 3]
    return rng, R, img, qoff, Q


def _windows(rng, n_img, e):
    ex = _empty(n_img, e)
    for b in range(n_img):
        for j in range(e):
            lo = int(rng.integers(-5, 125))
            ex[b, j] = (lo, lo + int(rng.integers(0, 5)) - 1)   # (length 0: an empty interval)
    ex[0, 0] = (10, 12)
    if e >= 3:
        ex[0, 1] = (11, 12)                             # overlapping
        ex[0, 2] = (60, 59)
        ex[2, 0] = (30, 36)
        ex[2, 1] = (34, 41)                             # overlapping
        ex[2, 2] = (42, 43)                             # adjacent
    if e == 8:
        ex[0, 3:] = ((8, 11), (-7, 2), (115, 2_000_000_000), (50, 52), (51, 55))
        ex[3, 0] = (-2_000_000_000, 2)                  # below 0
        ex[3, 7] = (118, 2_000_000_000)                 # above the largest id
    return ex


@pytest.mark.parametrize("e", [1, 3, 8])
def test_against_a_fresh_index_without_the_window(eng, eng2, e):
    rng, R, img, qoff, Q = _oracle_case()
    ex = _windows(rng, len(qoff) - 1, e)
    eng.db_reset()
    eng.db_add(R, img)
    D = _emu_d2(Q, R)
    for k in (50, 200):
        got = eng.search_excluding(Q, qoff, ex, k)
        _check(got, _brute(D, img, qoff, ex, k))
        _check(got, _fresh(eng2, R, img, Q, qoff, ex, k))
    # the planted ties: query row 0 finds the two outside copies at distance 0, lower id first, and not the inside one
    gi = got[1].cpu().numpy()
    assert gi[0, :2].tolist() == [13 * 30 + 5, 40 * 30 + 1] and 12 * 30 + 3 not in gi[0]
    assert (got[0][0, :2] == 0).all()
    # the same through device queries
    _check(eng.search_excluding(torch.from_numpy(Q).cuda(), qoff, ex, 50), _brute(D, img, qoff, ex, 50))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _map_6000(rng, d=64):
    R = _unit(rng.standard_normal((6000, d)).astype(np.float32))
    img = np.repeat(np.arange(120, dtype=np.int32), 50)
    return R, img


def test_head_path_by_construction(eng, eng2):
    from revisit_anything_amd.engine import excluded_rows, window_intervals

    rng = np.random.default_rng(3)
    R, img = _map_6000(rng)
    frames = np.array([10, 50, 90, 119])
    qoff = np.array([0, 50, 100, 150, 200], np.int32)
    Q = _unit(np.concatenate([R[img == f] for f in frames]) + 0.1 * rng.standard_normal((200, 64)).astype(np.float32))
    ex = window_intervals(frames, 3)
    X = excluded_rows(ex, np.bincount(img))
    assert X.tolist() == [350, 350, 350, 200]
    eng.db_reset()
    eng.db_add(R, img)
    k = 200
    assert k + X.max() <= 1024
    eng.set_profiling(True)
    eng.profile_reset()
    got = eng.search_excluding(Q, qoff, ex, k)
    eng.synchronize()
    ms, launches = eng.stage_ms("knn_exclude")
    eng.set_profiling(False)
    assert launches == 1 and ms > 0                    # the head path adds ONE kernel to the inner search
    st = eng.exclude_stats()
    assert st["k_fetch"] == k + X.max() and st["x_max"] == X.max() and st["tail_rows"] == 0 and st["n_img_excluding"] == 4
    _check(got, _brute(_emu_d2(Q, R), img, qoff, ex, k))
    _check(got, _fresh(eng2, R, img, Q, qoff, ex, k))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 200])
def test_clamped_depth_answer_still_in_the_list(eng, k):
    rng = np.random.default_rng(7)
    R, img = _map_6000(rng)
    qoff = np.array([0, 50, 100, 150, 200], np.int32)
    Q = _unit(R[rng.integers(0, 6000, 200)] + 0.2 * rng.standard_normal((200, 64)).astype(np.float32))
    ex = np.tile(np.array([[[40, 79]]], np.int32), (4, 1, 1))
    D = _emu_d2(Q, R)
    # the input's property: every query row has at least k allowed rows among its nearest 1024
    near = np.argsort(D, axis=1, kind="stable")[:, :1024]
    allowed_near = (~_excluded(img, ex[0]))[near].sum(axis=1)
    print("allowed rows among the nearest 1024: min", allowed_near.min())
    assert allowed_near.min() >= k
    eng.db_reset()
    eng.db_add(R, img)
    got = eng.search_excluding(Q, qoff, ex, k)
    st = eng.exclude_stats()
    assert st["x_max"] == 2000 and st["k_fetch"] == 1024 and st["tail_rows"] == 0
    _check(got, _brute(D, img, qoff, ex, k))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _crowded(rng, n, d, n_excl_img, first, nq):
    """Rows of the images first .. first + n_excl_img - 1 and all query rows in one tight cluster, the rest random."""
    per = 50
    img = np.repeat(np.arange(n // per, dtype=np.int32), per)
    R = rng.standard_normal((n, d)).astype(np.float32)
    c = _unit(rng.standard_normal((1, d)).astype(np.float32))
    sig = np.float32(0.24 / np.sqrt(d))
    inside = (img >= first) & (img < first + n_excl_img)
    R[inside] = c + sig * rng.standard_normal((int(inside.sum()), d)).astype(np.float32)
    Q = c + sig * rng.standard_normal((nq, d)).astype(np.float32)
    return _unit(R), img, _unit(Q)


@pytest.mark.parametrize("variant", ["50_rows", "130_rows_three_groups", "d1024_n20000", "d32_single_row_range"])
def test_the_tail(eng, eng2, variant):
    rng = np.random.default_rng(7)
    n, d, nq = (20000, 1024, 50) if variant == "d1024_n20000" else (6000, 64, 130 if variant.startswith("130") else 50)
    single = variant == "d32_single_row_range"
    if single:
        d = 32                                          # one k-tile of the tail's GEMM (csrc/group_tile_dev.h)
    R, img, Q = _crowded(rng, n, d, 40, 40, nq)
    qoff = np.array([0, nq], np.int32)
    ex = np.array([[[40, 79]]], np.int32)
    x_max = 2000
    if single:
        # image 60, inside the cluster, keeps ONE row (3000); the windows 40 .. 59 and 61 .. 119 leave two allowed ranges of map
        # positions: the 2000 rows of the images 0 .. 39, and that row
        img[3001:3050] = 61
        ex = np.array([[[40, 59], [61, 119]]], np.int32)
        x_max = 3999
    k = 50
    D = _emu_d2(Q, R)
    # the input's property, not the library's: no allowed row is among a query row's nearest 1024 (single: at most that one row,
    # which is every query row's nearest allowed row)
    near = np.argsort(D, axis=1, kind="stable")[:, :1024]
    allowed = ~_excluded(img, ex[0])
    if single:
        assert allowed.sum() == 2001 and allowed[3000] and (allowed[near].sum(axis=1) <= 1).all()
        assert (_brute(D, img, qoff, ex, k)[1][:, 0] == 3000).all()
    else:
        assert allowed[near].sum() == 0
    eng.db_reset()
    eng.db_add(R, img)
    eng.set_profiling(True)
    eng.profile_reset()
    got = eng.search_excluding(Q, qoff, ex, k)
    eng.synchronize()
    _, launches = eng.stage_ms("knn_exclude")
    eng.set_profiling(False)
    assert launches == 5                                # query norms, compaction, the tail's GEMM, its final sort, the scatter
    st = eng.exclude_stats()
    assert st["k_fetch"] == 1024 and st["x_max"] == x_max
    assert st["tail_rows"] == nq                        # EVERY row must have gone through the tail
    _check(got, _brute(D, img, qoff, ex, k))
    _check(got, _fresh(eng2, R, img, Q, qoff, ex, k))


def test_exclude_stats_fetched_after_a_grouped_search(eng):
    """search_excluding and search_grouped keep their deep lists and query norms in the same scratch, and exclude_stats() reads the
    tail's row counter from the device when it is asked: a grouped search in between -- its own tail running too -- changes neither
    the counter nor the exclusion's outputs."""
    rng = np.random.default_rng(7)
    R, img, Q = _crowded(rng, 6000, 64, 40, 40, 50)
    qoff = np.array([0, 50], np.int32)
    ex = np.array([[[40, 79]]], np.int32)
    eng.db_reset()
    eng.db_add(R, img)
    alone = eng.search_excluding(Q, qoff, ex, 50)
    st_alone = eng.exclude_stats()
    assert st_alone["tail_rows"] == 50                  # (test_the_tail[50_rows]: every row is short)
    got = eng.search_excluding(Q, qoff, ex, 50)
    eng.set_option("group_fetch", 64)
    try:
        eng.search_grouped(Q, 50, 1)
        assert eng.group_stats()["tail_rows"] > 0       # 64 entries of <= 40 images cannot hold 50 different ones
    finally:
        eng.set_option("group_fetch", 0)
    assert eng.exclude_stats() == st_alone
    _check(got, tuple(t.cpu().numpy() for t in alone))


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_everything_excluded_and_fewer_allowed_rows_than_k(eng):
    rng, R, img, qoff, Q = _oracle_case()
    eng.db_reset()
    eng.db_add(R, img)
    D = _emu_d2(Q, R)
    n_img = len(qoff) - 1
    every = np.tile(np.array([[[-5, 1_000_000]]], np.int32), (n_img, 1, 1))
    d2, idx = eng.search_excluding(Q, qoff, every, 50)
    assert (idx == -1).all() and torch.isinf(d2).all() and (d2 > 0).all()
    # all but one image (30 rows) excluded, k = 50; image 2 keeps two images (60 rows); image 3 excludes nothing
    few = _empty(n_img, 2)
    few[:, 0] = (0, 16)
    few[:, 1] = (18, 200)
    few[2, 1] = (19, 200)
    few[3] = ((1, 0), (1, 0))
    got = eng.search_excluding(Q, qoff, few, 50)
    _check(got, _brute(D, img, qoff, few, 50))
    gi = got[1].cpu().numpy()
    assert (gi[:30, :30] >= 0).all() and (gi[:30, 30:] == -1).all() and (gi[30:160] >= 0).all()
    # an index smaller than k_fetch
    eng.db_reset()
    eng.db_add(R[:300], img[:300])
    got = eng.search_excluding(Q, qoff, few, 400)
    _check(got, _brute(D[:, :300], img[:300], qoff, few, 400))
    got = eng.search_excluding(Q, qoff, every, 400)
    assert (got[1] == -1).all() and torch.isinf(got[0]).all()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["70001x128", "300000x256"])
def test_single_image_plan_and_batch_plan_agree(eng, eng2, shape):
    """An index large enough for the plans the feature is meant for (above 32768 rows the search leaves the distance-matrix path):
    the same image's 50 rows alone take the single-image plan (one filter level, device-driven head and tail), inside a 200-row
    batch the deep plan -- both at depth k_fetch > k into the exclusion's scratch.  The two agree bit for bit, with the fresh-index
    oracle and with the emulated brute force."""
    from revisit_anything_amd.engine import excluded_rows, window_intervals

    rng = np.random.default_rng(8)
    n, d = (70001, 128) if shape == "70001x128" else (300000, 256)
    per = 50
    R = _unit(rng.standard_normal((n, d), dtype=np.float32))
    img = (np.arange(n) // per).astype(np.int32)
    frames = np.array([17, 200, 201, n // per - 1])
    Q = _unit(np.concatenate([R[img == f] for f in frames]) + 0.05 * rng.standard_normal((200, d)).astype(np.float32))
    qoff = np.array([0, 50, 100, 150, 200], np.int32)
    ex = window_intervals(frames, 3)
    X = excluded_rows(ex, np.bincount(img))            # (the last frame's window runs over the end of the map)
    assert X.max() == 350 and X[3] < 350
    eng.db_reset()
    eng.db_add(R, img)
    for k in (50, 200):
        bd, bi = eng.search_excluding(Q, qoff, ex, k)
        assert eng.exclude_stats() == {"k_fetch": k + 350, "x_max": 350, "tail_rows": 0, "n_img_excluding": 4}
        st = eng.search_stats()                         # (of the inner search)
        assert st["filter"] == "f16" and st["levels"] >= 2 and st["n_queries"] == 200, st
        for b in range(4):
            sd, si = eng.search_excluding(Q[50 * b:50 * b + 50], np.array([0, 50], np.int32), ex[b:b + 1], k)
            st = eng.search_stats()
            assert st["filter"] == "f16" and st["levels"] == 1 and st["n_queries"] == 50, st
            assert eng.exclude_stats()["k_fetch"] == k + X[b]
            assert torch.equal(si, bi[50 * b:50 * b + 50])
            assert torch.equal(sd.view(torch.int32), bd[50 * b:50 * b + 50].view(torch.int32))
            assert not np.isin(img[si.cpu().numpy()], np.arange(frames[b] - 3, frames[b] + 4)).any()
        _check((bd, bi), _fresh(eng2, R, img, Q, qoff, ex, k))
        _check((bd[:50], bi[:50]), _brute_near(Q[:50], R, img, ex[0], k))
        _check((bd[150:], bi[150:]), _brute_near(Q[150:], R, img, ex[3], k))


def test_device_view_off_a_16_byte_boundary(eng, eng2):
    """Device queries that start 4 bytes behind a 16-byte boundary (a view into a larger tensor), through the head path and through
    the tail, whose GEMM needs an aligned copy.  The reference is the fresh index searched through the SAME view: the norms of such
    rows are summed in another order than those of aligned rows, in segvlad_search as here."""
    rng = np.random.default_rng(7)
    R, img, Q = _crowded(rng, 6000, 64, 40, 40, 50)
    buf = torch.empty(50 * 64 + 5, dtype=torch.float32, device="cuda:0")
    off = 1 + (-(buf.data_ptr() // 4) % 4)             # the first element 4 bytes behind a 16-byte boundary
    Qv = buf[off:off + 50 * 64].view(50, 64)
    Qv.copy_(torch.from_numpy(Q))
    assert Qv.data_ptr() % 16 == 4 and Qv.is_contiguous()
    qoff = np.array([0, 50], np.int32)
    eng.db_reset()
    eng.db_add(R, img)
    for ex, tail_rows in ((np.array([[[40, 79]]], np.int32), 50), (np.array([[[40, 44]]], np.int32), 0)):
        got = eng.search_excluding(Qv, qoff, ex, 50)
        assert eng.exclude_stats()["tail_rows"] == tail_rows
        _check(got, _fresh(eng2, R, img, Qv, qoff, ex, 50))
        gi = got[1].cpu().numpy()
        assert np.array_equal(gi, _brute(_emu_d2(Q, R), img, qoff, ex, 50)[1])   # (the ids of the aligned chain's order too)


def test_rows_with_a_negative_image_id(eng):
    """A row whose image id is negative belongs to no image: no interval excludes it (head path, against the brute force), and a
    window that could need the exact tail -- whose image -> row map does not hold such rows -- is refused with SEGVLAD_ERR_LIMIT;
    the context stays usable."""
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    rng, R, img, qoff, Q = _oracle_case()
    img = img.copy()
    img[(img == 7) | (img == 50)] = -1
    Q[3] = R[7 * 30 + 2]                                # a query row on top of a negative-id row
    eng.db_reset()
    eng.db_add(R, img)
    D = _emu_d2(Q, R)
    ex = _windows(rng, len(qoff) - 1, 3)
    ex[0, 2] = (-5, 9)                                  # reaches below 0 and over the ids 7's rows had
    ex[2, 2] = (48, 52)
    for k in (50, 200):
        got = eng.search_excluding(Q, qoff, ex, k)
        assert eng.exclude_stats()["tail_rows"] == 0
        _check(got, _brute(D, img, qoff, ex, k))
    assert got[1][3, 0].item() == 7 * 30 + 2
    before = eng.search(Q, 50)
    wide = ex.copy()
    wide[4, 0] = (0, 80)                                # more than 1024 - k rows
    with pytest.raises(SegVLADError) as e:
        eng.search_excluding(Q, qoff, wide, 50)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    after = eng.search(Q, 50)
    assert torch.equal(after[1], before[1]) and torch.equal(after[0].view(torch.int32), before[0].view(torch.int32))
    _check(eng.search_excluding(Q, qoff, ex, 50), _brute(D, img, qoff, ex, 50))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_lifetime(eng, eng2):
    """exclude -> db_add more images -> exclude -> db_remove -> exclude: the host mirror of the image -> row map follows the
    index.  Interleaved with search_shortlist on the same context (the two share the map and the GEMM's scratch)."""
    rng, R, img, qoff, Q = _oracle_case()
    ex = _windows(rng, len(qoff) - 1, 3)
    ex[4] = ((0, 45), (60, 100), (1, 0))                # more than 1024 - k rows: may need the tail
    every = np.tile(np.unique(img), (len(qoff) - 1, 1)).astype(np.int32)

    def both(Rc, imgc, adds):
        for k in (30, 200):
            want = eng.search(Q, k)
            got = eng.search_shortlist(Q, qoff, every, k)
            assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
            got = eng.search_excluding(Q, qoff, ex, k)
            _check(got, _brute(_emu_d2(Q, Rc), imgc, qoff, ex, k))
            _check(got, _fresh(eng2, Rc, imgc, Q, qoff, ex, k, adds))

    eng.db_reset()
    eng.db_add(R[:1800], img[:1800])
    both(R[:1800], img[:1800], [(0, 1800)])
    eng.db_add(R[1800:], img[1800:])
    both(R, img, [(0, 1800), (1800, 3000)])
    gone = np.array([11, 12, 35, 36, 37, 90], np.int32)
    eng.db_remove(img_ids=gone)
    keep = ~np.isin(img, gone)
    both(R[keep], img[keep], None)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_LIMIT, SEGVLAD_ERR_STATE, SegVLADError

    rng = np.random.default_rng(5)
    R = _unit(rng.standard_normal((200, 64)).astype(np.float32))
    Q = R[:10].copy()
    qoff = np.array([0, 10], np.int32)
    ex = np.array([[[2, 3]]], np.int32)
    eng.db_reset()
    eng.db_add(R)
    with pytest.raises(SegVLADError) as e:
        eng.search_excluding(Q, qoff, ex, 5)
    assert e.value.code == SEGVLAD_ERR_STATE
    eng.db_reset()
    eng.db_add(np.ascontiguousarray(R[:, :48]), np.repeat(np.arange(10, dtype=np.int32), 20))
    with pytest.raises(SegVLADError) as e:
        eng.search_excluding(np.ascontiguousarray(Q[:, :48]), qoff, ex, 5)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    eng.db_reset()
    img = np.repeat(np.arange(10, dtype=np.int32), 20)
    eng.db_add(R, img)
    before = eng.search(Q, 5)
    d2 = torch.empty((10, 5), dtype=torch.float32, device="cuda:0")
    idx = torch.empty((10, 5), dtype=torch.int64, device="cuda:0")

    def raw(qo, n_img, exc, n_e, k):
        return eng.lib.segvlad_search_excluding(eng._h, Q.ctypes.data, 10, qo.ctypes.data, n_img, exc.ctypes.data, n_e, k,
                                                d2.data_ptr(), idx.data_ptr())

    ex9 = np.zeros((1, 9, 2), np.int32)
    assert raw(qoff, 1, ex, 0, 5) == SEGVLAD_ERR_ARG
    assert raw(qoff, 1, ex9, 9, 5) == SEGVLAD_ERR_ARG
    assert raw(qoff, 1, ex, 1, 0) == SEGVLAD_ERR_ARG
    assert raw(qoff, 1, ex, 1, 1025) == SEGVLAD_ERR_ARG
    assert raw(np.array([0, 9], np.int32), 1, ex, 1, 5) == SEGVLAD_ERR_ARG
    assert raw(np.array([1, 10], np.int32), 1, ex, 1, 5) == SEGVLAD_ERR_ARG
    assert raw(np.array([0, 12, 10], np.int32), 2, np.tile(ex, (2, 1, 1)), 1, 5) == SEGVLAD_ERR_ARG
    dev_qoff = torch.from_numpy(qoff).cuda()
    for bad_qoff in (None, dev_qoff.data_ptr()):   # null; a device pointer
        assert eng.lib.segvlad_search_excluding(eng._h, Q.ctypes.data, 10, bad_qoff, 1, ex.ctypes.data, 1, 5, d2.data_ptr(),
                                                idx.data_ptr()) == SEGVLAD_ERR_ARG
        assert eng.lib.segvlad_last_error(eng._h).decode().startswith("search_excluding: ")
    for bad in (np.zeros((1, 9, 2), np.int32), np.zeros((2, 1, 2), np.int32), np.zeros((1, 2), np.int32), [[(1, 2, 3)]]):
        with pytest.raises(ValueError):
            eng.search_excluding(Q, qoff, bad, 5)
    # the context stays usable, and search is unchanged
    after = eng.search(Q, 5)
    assert torch.equal(after[1], before[1]) and torch.equal(after[0].view(torch.int32), before[0].view(torch.int32))
    got = eng.search_excluding(Q, qoff, ex, 5)
    _check(got, _brute(_emu_d2(Q, R), img, qoff, ex, 5))


# ---- 10 --------------------------------------------------------------------------------------------------------------------
def test_retrieve_a_map_queried_with_its_own_frames(eng, eng2):
    from revisit_anything_amd.engine import window_intervals
    from revisit_anything_amd.pipeline import SegVLADPipeline

    rng = np.random.default_rng(10)
    n_frames, per, d, r = 40, 20, 64, 2
    # a trajectory: every frame's rows are its predecessor's plus a small step, so neighbours in time are near-duplicates
    rows = [_unit(rng.standard_normal((per, d)).astype(np.float32))]
    for _ in range(n_frames - 1):
        rows.append(_unit(rows[-1] + 0.15 * rng.standard_normal((per, d)).astype(np.float32)))
    R = np.concatenate(rows)
    img = np.repeat(np.arange(n_frames, dtype=np.int32), per)
    frames = np.array([0, 3, 17, 38, 39])
    Q = np.concatenate([R[img == f] for f in frames])
    qoff = (np.arange(len(frames) + 1) * per).astype(np.int32)
    eng.db_reset()
    eng.db_add(R, img)
    pipe = SegVLADPipeline(eng, 112, 140)
    p0, _, _, _ = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5)
    assert p0[:, 0].cpu().numpy().tolist() == frames.tolist()   # without exclude every top-1 is the frame itself
    ex = window_intervals(frames, r)
    with pytest.raises(ValueError):
        pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5, exclude=ex, shortlist=[[1]] * len(frames))
    pipe2 = SegVLADPipeline(eng2, 112, 140)
    for b, f in enumerate(frames):
        Qb, qo = Q[qoff[b]:qoff[b + 1]], np.array([0, per], np.int32)
        pred, sc, m, sims = pipe.retrieve(Qb, qo, k_search=40, k_vote=25, n_top=5, want_scores=True, exclude=ex[b:b + 1])
        pred, sc = pred.cpu().numpy(), sc.cpu().numpy()
        assert not ((pred >= f - r) & (pred <= f + r)).any()
        eng2.db_reset()
        eng2.db_add(R, img)
        eng2.db_remove(img_ids=np.arange(max(f - r, 0), min(f + r, n_frames - 1) + 1, dtype=np.int32))
        wp, ws, _, wsims = pipe2.retrieve(Qb, qo, k_search=40, k_vote=25, n_top=5, want_scores=True)
        assert np.array_equal(pred, wp.cpu().numpy())
        assert np.array_equal(sc.view(np.uint64), ws.cpu().numpy().view(np.uint64))
        assert torch.equal(sims.view(torch.int32), wsims.view(torch.int32))
    # the batch form: no prediction inside any image's window
    pred, _, _, _ = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5, exclude=ex)
    pred = pred.cpu().numpy()
    assert not ((pred >= frames[:, None] - r) & (pred <= frames[:, None] + r)).any()


# ---- 11 --------------------------------------------------------------------------------------------------------------------
def test_twice_in_one_context_gives_identical_bits(eng):
    """Head path, clamped depth and tail in one context, twice: identical bits, and (under SEGVLAD_GUARD=1, the suite's default)
    no fence trips -- a tripped fence fails the call that tripped it."""
    rng = np.random.default_rng(7)
    R, img, Q = _crowded(rng, 6000, 64, 40, 40, 130)
    Q2 = _unit(R[rng.integers(0, 6000, 70)] + 0.2 * rng.standard_normal((70, 64)).astype(np.float32))
    Qa = np.concatenate([Q, Q2])
    qoff = np.array([0, 130, 165, 200], np.int32)
    ex = np.array([[[40, 79], [1, 0]], [[3, 5], [4, 9]], [[0, 30], [70, 119]]], np.int32)
    eng.db_reset()
    eng.db_add(R, img)
    runs = []
    for _ in range(2):
        out = []
        for k in (50, 200):
            d2, idx = eng.search_excluding(Qa, qoff, ex, k)
            out.append((d2.cpu().numpy().view(np.uint32).copy(), idx.cpu().numpy().copy(), eng.exclude_stats()))
        runs.append(out)
    for (a_d, a_i, a_s), (b_d, b_i, b_s) in zip(*runs):
        assert np.array_equal(a_d, b_d) and np.array_equal(a_i, b_i) and a_s == b_s
    assert runs[0][0][2]["tail_rows"] >= 130
    _check(eng.search_excluding(Qa, qoff, ex, 50), _brute(_emu_d2(Qa, R), img, qoff, ex, 50))
