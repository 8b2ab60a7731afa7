"""Spatial verification of matched segments (segvlad_verify_pairs, csrc/verify_kernels.hip) on the GPU.

The yardstick is tests/verify_ref.py, a literal NumPy float64 restatement of the contract in include/segvlad.h (NumPy never fuses a
multiplication with an addition), never the code under test.  Counts, winners' samples, inlier flags and the slots' order are
compared for equality -- also on real coordinates, where a fused multiply-add or another order of operations would move a decision
that sits near its bound --, the informative model within 1e-9 absolute: a handful of fp64 operations on values <= 1e3, six orders
above their rounding and six below a pixel."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import verify_ref as V

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -4
INT_KEYS = ("n_inlier", "pair", "order", "inlier")


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(eng, q_xy, r_xy, qoff, fwd, mut, tol, lo=0.5, hi=2.0):
    out = eng.verify_pairs(_dev(q_xy), _dev(r_xy), qoff, _dev(fwd), _dev(mut), tol, lo, hi, want_rows=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, what=""):
    assert set(got) == set(want)
    for key in INT_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5])
    assert got["model"].dtype == np.float64 and got["model"].shape == want["model"].shape
    assert np.array_equal(np.isnan(got["model"]), np.isnan(want["model"])), what
    ok = ~np.isnan(want["model"])
    assert np.abs(got["model"][ok] - want["model"][ok]).max(initial=0.0) <= 1e-9, what


def _flags_add_up(got, qoff):
    for b in range(len(qoff) - 1):
        assert np.array_equal(got["inlier"][qoff[b]:qoff[b + 1]].sum(axis=0, dtype=np.int64), got["n_inlier"][b])


def _raw(eng, q_xy, nq, r_xy, n_r, qoff, n_img, C, fwd, mut, tol, lo, hi, n_inl, pair=None, model=None, order=None, inl=None):
    from revisit_anything_amd.engine import _ptr

    eng._stream()
    return eng.lib.segvlad_verify_pairs(eng._h, _ptr(q_xy), nq, _ptr(r_xy), n_r, _ptr(qoff), n_img, C, _ptr(fwd), _ptr(mut), tol, lo, hi,
                                        _ptr(n_inl), _ptr(pair), _ptr(model), _ptr(order), _ptr(inl))


# ---- 1. integer coordinates: exact in any order of operations, logic errors alone ---------------------------------------------
def _integer_case(seed):
    """6 images of 8 .. 24 rows, 3 slots each.  Query points: DISTINCT integers of [0, 128)^2 per image.  Per slot 60 % of the rows
    follow s = a p + t with a of {1, i, 1 + i, 2} and an integer t, the others get integer outliers of [-128, 256)^2.  Every
    intermediate of the contract is then an integer: |d| <= 180, |e| <= 543, n <= 32 258, |ar|, |ai| <= 97 740, |ux|, |uy| <= 3e7,
    ux^2 + uy^2 <= 1.8e15 < 2^53 -- no result can depend on rounding.  Every reference row is its own entry of r_xy."""
    rng = np.random.default_rng(seed)
    n_img, C = 6, 3
    sizes = rng.integers(8, 25, n_img)
    sizes[0], sizes[1] = 8, 24
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    nq = int(qoff[-1])
    q_xy = np.zeros((nq, 2))
    r_xy = np.zeros((nq * C, 2))
    fwd = rng.permutation(nq * C).astype(np.int64).reshape(nq, C)      # (the table is in no particular order)
    planted = np.zeros((n_img, C), np.int64)
    for b in range(n_img):
        rows = np.arange(qoff[b], qoff[b + 1])
        cells = rng.choice(128 * 128, len(rows), replace=False)
        q_xy[rows] = np.stack([cells % 128, cells // 128], 1)
        pc = q_xy[rows, 0] + 1j * q_xy[rows, 1]
        for j in range(C):
            a = (1, 1j, 1 + 1j, 2)[(b + j) % 4]
            sc = a * pc + complex(int(rng.integers(-20, 21)), int(rng.integers(-20, 21)))
            s = np.stack([sc.real, sc.imag], 1)
            n_in = int(np.ceil(0.6 * len(rows)))
            out_rows = rng.permutation(len(rows))[n_in:]
            s[out_rows] = rng.integers(-128, 256, (len(out_rows), 2))
            r_xy[fwd[rows, j]] = s
            planted[b, j] = n_in
    return q_xy, r_xy, qoff, fwd, np.ones((nq, C), np.uint8), planted


@pytest.mark.parametrize("seed", [1, 2])
def test_integer_coordinates_equal_the_reference(eng, seed):
    q_xy, r_xy, qoff, fwd, mut, planted = _integer_case(seed)
    got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 2.0, 0.25, 4.0)
    _check(got, V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 2.0, 0.25, 4.0))
    _flags_add_up(got, qoff)
    assert (got["n_inlier"] >= planted).all()      # any two planted rows are an exact, eligible hypothesis of all of them


# ---- 2. real coordinates: the arithmetic, operation for operation ---------------------------------------------------------------
def _similarity(rng):
    return rng.uniform(0.7, 1.4) * np.exp(1j * rng.uniform(-0.3, 0.3)), complex(rng.uniform(-40, 40), rng.uniform(-30, 30))


def _real_case(seed, n_img=5, rows=24, n_in=16):
    """Per image `rows` points of a 320 x 240 frame.  Slot 0: the first n_in rows moved by one similarity (scale 0.7 .. 1.4, rotation
    +-0.3 rad) plus 0.5 px of noise, the others random; slot 1: all random."""
    rng = np.random.default_rng(seed)
    nq = n_img * rows
    qoff = np.arange(0, nq + 1, rows, dtype=np.int32)
    q_xy = rng.uniform([0, 0], [320, 240], (nq, 2))
    r_xy = rng.uniform([0, 0], [320, 240], (2 * nq, 2))
    fwd = np.stack([np.arange(nq), nq + np.arange(nq)], 1).astype(np.int64)
    for b in range(n_img):
        a, t = _similarity(rng)
        rws = np.arange(qoff[b], qoff[b] + n_in)
        sc = a * (q_xy[rws, 0] + 1j * q_xy[rws, 1]) + t
        r_xy[rws] = np.stack([sc.real, sc.imag], 1) + rng.normal(0, 0.5, (n_in, 2))
    return q_xy, r_xy, qoff, fwd, np.ones((nq, 2), np.uint8)


@pytest.mark.parametrize("seed", [3, 4])
def test_real_coordinates_equal_the_reference(eng, seed):
    q_xy, r_xy, qoff, fwd, mut = _real_case(seed)
    got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 3.0, 0.5, 2.0)
    want = V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0, 0.5, 2.0)
    _check(got, want)
    _flags_add_up(got, qoff)
    assert (got["order"][:, 0] == 0).all()          # the planted slot first: the reference gives 16 against at most 3 over 200 trials
    assert (want["n_inlier"][:, 0] >= 12).all() and (want["n_inlier"][:, 1] <= 6).all()   # (the case is what it claims to be)


# ---- 3. sizes where it can break ---------------------------------------------------------------------------------------------------
def _sized_case(seed, Ms, C=2):
    """One image per entry of Ms with that many correspondences in slot 0 (and up to 3 more rows that are not mutual there, up to
    the limit of 256 rows); 70 % follow a similarity with noise.  Slot 1 and beyond: the same points under a random mutual mask."""
    rng = np.random.default_rng(seed)
    sizes = [min(256, M + 3) for M in Ms]
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    nq = int(qoff[-1])
    q_xy = rng.uniform([0, 0], [320, 240], (nq, 2))
    r_xy = rng.uniform([0, 0], [320, 240], (nq, 2))
    mut = (rng.random((nq, C)) < 0.6).astype(np.uint8)
    for b, M in enumerate(Ms):
        rws = np.arange(qoff[b], qoff[b + 1])
        a, t = _similarity(rng)
        follow = rws[rng.random(len(rws)) < 0.7]
        sc = a * (q_xy[follow, 0] + 1j * q_xy[follow, 1]) + t
        r_xy[follow] = np.stack([sc.real, sc.imag], 1) + rng.normal(0, 0.5, (len(follow), 2))
        mut[rws, 0] = 0
        mut[rng.permutation(rws)[:M], 0] = 1
    fwd = np.tile(np.arange(nq, dtype=np.int64)[:, None], (1, C))
    return q_xy, r_xy, qoff, fwd, mut


def test_sizes_around_the_ballot_step_and_the_limit(eng):
    Ms = [0, 1, 2, 3, 64, 65, 255, 256]
    q_xy, r_xy, qoff, fwd, mut = _sized_case(5, Ms)
    assert [int(mut[qoff[b]:qoff[b + 1], 0].sum()) for b in range(len(Ms))] == Ms and qoff[-1] - qoff[-2] == 256
    got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 3.0)
    _check(got, V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0))
    _flags_add_up(got, qoff)
    assert got["n_inlier"][:2, 0].tolist() == [0, 0] and got["pair"][:2, 0].tolist() == [[-1, -1]] * 2
    assert got["n_inlier"][-1, 0] > 100              # (the 256-row slot is a real search: 32 640 hypotheses over several tasks)


def test_the_last_hypothesis_of_a_full_slot_can_win(eng):
    """256 correspondences of which only the last two agree with anything eligible: every other query point is the SAME point
    (n = 0 between them) and maps far away, so hypothesis h = 32 639 = (254, 255) is the winner."""
    q_xy = np.tile([[10.0, 20.0]], (256, 1))
    q_xy[254], q_xy[255] = [100.0, 50.0], [130.0, 90.0]
    r_xy = np.arange(512, dtype=np.float64).reshape(256, 2) * 1000.0 + 5000.0
    r_xy[254], r_xy[255] = q_xy[254] + [1.5, -2.5], q_xy[255] + [1.5, -2.5]
    qoff = np.array([0, 256], np.int32)
    fwd, mut = np.arange(256, dtype=np.int64)[:, None], np.ones((256, 1), np.uint8)
    want = V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 1.0)
    assert want["pair"].tolist() == [[[254, 255]]] and want["n_inlier"].tolist() == [[2]]
    _check(_run(eng, q_xy, r_xy, qoff, fwd, mut, 1.0), want)


def test_more_than_256_rows_is_a_limit_and_the_context_stays_usable(eng):
    nq = 257 + 4
    qoff = np.array([0, 4, nq], np.int32)
    q_xy, r_xy = _dev(np.random.default_rng(0).uniform(0, 100, (nq, 2))), _dev(np.random.default_rng(1).uniform(0, 100, (nq, 2)))
    fwd, mut = _dev(np.arange(nq, dtype=np.int64)[:, None].copy()), _dev(np.ones((nq, 1), np.uint8))
    n_inl = torch.full((2, 1), -7, dtype=torch.int32, device="cuda")
    assert _raw(eng, q_xy, nq, r_xy, nq, qoff, 2, 1, fwd, mut, 3.0, 0.5, 2.0, n_inl) == ERR_LIMIT
    assert (n_inl == -7).all()                        # refused before anything ran
    with pytest.raises(ValueError):
        eng.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0)
    q_xy, r_xy, qoff, fwd, mut = _real_case(6, n_img=2)
    _check(_run(eng, q_xy, r_xy, qoff, fwd, mut, 3.0), V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0))


@pytest.mark.parametrize("C", [1, 64])
def test_slot_counts_one_and_sixty_four_with_an_empty_image(eng, C):
    rng = np.random.default_rng(7 + C)
    qoff = np.array([0, 10, 10, 80, 85], np.int32)
    nq = int(qoff[-1])
    q_xy = rng.uniform([0, 0], [320, 240], (nq, 2))
    a, t = _similarity(rng)
    sc = a * (q_xy[:, 0] + 1j * q_xy[:, 1]) + t
    r_xy = np.stack([sc.real, sc.imag], 1) + rng.normal(0, 0.5, (nq, 2))
    r_xy = np.vstack([r_xy, rng.uniform([0, 0], [320, 240], (nq, 2))])
    fwd = np.where(rng.random((nq, C)) < 0.7, np.arange(nq)[:, None], nq + rng.integers(0, nq, (nq, C))).astype(np.int64)
    mut = (rng.random((nq, C)) < rng.uniform(0.1, 1.0, C)[None, :]).astype(np.uint8)
    got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 3.0)
    _check(got, V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0))
    _flags_add_up(got, qoff)
    assert got["order"][1].tolist() == list(range(C)) and not got["n_inlier"][1].any()


def test_no_query_rows_at_all_still_writes_the_per_image_outputs(eng):
    qoff = np.zeros(4, np.int32)
    got = _run(eng, np.zeros((0, 2)), np.zeros((5, 2)), qoff, np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint8), 3.0)
    assert got["n_inlier"].tolist() == [[0, 0, 0]] * 3 and (got["pair"] == -1).all() and np.isnan(got["model"]).all()
    assert got["order"].tolist() == [[0, 1, 2]] * 3 and got["inlier"].shape == (0, 3)
    # no image at all: nothing is written, the call succeeds
    n_inl = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw(eng, None, 0, None, 0, np.zeros(1, np.int32), 0, 3, None, None, 3.0, 0.5, 2.0, n_inl) == 0


def test_a_tied_best_count_goes_to_the_lowest_hypothesis(eng):
    """Slot 0: a pure shift of every row -- every hypothesis has all the inliers, (row 0, row 1) wins.  Slot 1: two groups of four
    rows under two different shifts, interleaved: rows 1, 2, 5, 6 and rows 0, 3, 4, 7; both reach 4, the first eligible hypothesis
    that does is (0, 3)."""
    rng = np.random.default_rng(8)
    q_xy = rng.uniform([0, 0], [320, 240], (8, 2))
    r0 = q_xy + [12.25, -7.5]
    r1 = q_xy + [100.0, 0.0]
    r1[[0, 3, 4, 7]] = q_xy[[0, 3, 4, 7]] + [-30.0, 60.0]
    r_xy = np.vstack([r0, r1])
    fwd = np.stack([np.arange(8), 8 + np.arange(8)], 1).astype(np.int64)
    qoff, mut = np.array([0, 8], np.int32), np.ones((8, 2), np.uint8)
    got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 1.0)
    _check(got, V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 1.0))
    assert got["n_inlier"].tolist() == [[8, 4]] and got["pair"].tolist() == [[[0, 1], [0, 3]]]
    assert got["inlier"][:, 1].tolist() == [1, 0, 0, 1, 1, 0, 0, 1] and got["order"].tolist() == [[0, 1]]


# ---- 4. dropped pairs, eligibility, argument errors ------------------------------------------------------------------------------
def test_dropped_pairs_and_eligibility(eng):
    rng = np.random.default_rng(9)
    rows = 30
    qoff = np.array([0, rows, 2 * rows], np.int32)
    nq = 2 * rows
    q_xy = rng.uniform([0, 0], [320, 240], (nq, 2))
    a, t = 3.0 * np.exp(0.2j), complex(4, 5)                            # image 1 is planted at scale 3
    sc = np.where(np.arange(nq) < rows, 1.1 * np.exp(-0.1j), a) * (q_xy[:, 0] + 1j * q_xy[:, 1]) + t
    r_xy = np.stack([sc.real, sc.imag], 1) + rng.normal(0, 0.3, (nq, 2))
    fwd = np.tile(np.arange(nq, dtype=np.int64)[:, None], (1, 2))
    mut = np.ones((nq, 2), np.uint8)
    # slot 0 of image 0: every kind of dropped row, with mutual = 1
    fwd[2, 0], fwd[5, 0] = -1, nq                                        # no row, and one past the table
    fwd[6, 0] = np.iinfo(np.int64).max
    q_xy[8, 0], q_xy[9, 1] = np.nan, np.inf                              # (dropped in both slots: the query point is shared)
    r_xy[11, 1], r_xy[12, 0] = np.nan, -np.inf
    mut[14, 0] = 0
    q_xy[16] = q_xy[15]                                                  # two correspondences at one query point: n = 0 between them
    mut[20:, 1] = 0                                                      # slot 1 of image 0: rows 0 .. 19, of which 8, 9, 11, 12 drop
    for lo, hi in ((0.5, 2.0), (0.5, 4.0), (2.9, 3.1)):
        got = _run(eng, q_xy, r_xy, qoff, fwd, mut, 3.0, lo, hi)
        want = V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0, lo, hi)
        _check(got, want, (lo, hi))
        _flags_add_up(got, qoff)
        dropped = [2, 5, 6, 8, 9, 11, 12, 14]
        assert not got["inlier"][dropped, 0].any()
        assert not (got["pair"][0, 0][:, None] == np.array(dropped)[None, :]).any()
    # under 0.5 .. 2 the planted scale-3 image reports what the reference reports -- no full consensus
    assert want["n_inlier"][1, 0] >= 29                                  # (last bounds: 2.9 .. 3.1 admit it)
    assert V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0, 0.5, 2.0)["n_inlier"][1, 0] < 10


def test_argument_errors(eng):
    q_xy, r_xy, qoff, fwd, mut = _real_case(10, n_img=2)
    nq, n_r = len(q_xy), len(r_xy)
    dq, dr, df, dm = _dev(q_xy), _dev(r_xy), _dev(fwd), _dev(mut)
    n_inl = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    ok = dict(q_xy=dq, nq=nq, r_xy=dr, n_r=n_r, qoff=qoff, n_img=2, C=2, fwd=df, mut=dm, tol=3.0, lo=0.5, hi=2.0, n_inl=n_inl)
    assert _raw(eng, **ok) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(tol=0.0), dict(tol=-1.0), dict(tol=nan), dict(tol=inf), dict(lo=0.0), dict(lo=-0.5), dict(lo=nan), dict(hi=nan),
                dict(lo=2.5), dict(hi=inf), dict(C=0), dict(C=65), dict(nq=-1), dict(n_r=-1), dict(n_img=-1), dict(nq=nq - 1),
                dict(qoff=None), dict(qoff=_dev(qoff)), dict(qoff=np.array([0, 30, 20, 48], np.int32), n_img=3),
                dict(q_xy=None), dict(r_xy=None), dict(fwd=None), dict(mut=None), dict(n_inl=None)):
        assert _raw(eng, **{**ok, **bad}) == ERR_ARG, bad
    assert _raw(eng, **ok) == 0                                          # the context stays usable


# ---- 5. host and device pointers, optional outputs, determinism ---------------------------------------------------------------------
def test_host_and_device_pointers_optional_outputs_and_determinism(eng):
    q_xy, r_xy, qoff, fwd, mut = _real_case(12, n_img=3)
    nq, n_r, n_img, C = len(q_xy), len(r_xy), 3, 2
    want = V.verify_pairs(q_xy, r_xy, qoff, fwd, mut, 3.0)

    def outs(device):
        mk = (lambda s, t: torch.zeros(s, dtype=t, device="cuda")) if device else \
             (lambda s, t: np.zeros(s, {torch.int32: np.int32, torch.float64: np.float64, torch.uint8: np.uint8}[t]))
        return dict(n_inl=mk((n_img, C), torch.int32), pair=mk((n_img, C, 2), torch.int32), model=mk((n_img, C, 4), torch.float64),
                    order=mk((n_img, C), torch.int32), inl=mk((nq, C), torch.uint8))

    def as_np(o):
        names = dict(n_inl="n_inlier", pair="pair", model="model", order="order", inl="inlier")
        return {names[k]: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}

    results = []
    for ins_dev, outs_dev in ((True, True), (False, False), (True, False), (False, True), (True, True)):
        cv = _dev if ins_dev else np.ascontiguousarray
        o = outs(outs_dev)
        assert _raw(eng, cv(q_xy), nq, cv(r_xy), n_r, qoff, n_img, C, cv(fwd), cv(mut), 3.0, 0.5, 2.0, **o) == 0
        torch.cuda.synchronize()
        results.append(as_np(o))
        _check(results[-1], want, (ins_dev, outs_dev))
    for r in results[1:]:                                                # the same bits, the model included
        for k in r:
            assert r[k].tobytes() == results[0][k].tobytes(), k
    # mixed inputs, and every optional output left out
    n_inl = torch.zeros((n_img, C), dtype=torch.int32, device="cuda")
    assert _raw(eng, q_xy, nq, _dev(r_xy), n_r, qoff, n_img, C, _dev(fwd), mut, 3.0, 0.5, 2.0, n_inl) == 0
    assert np.array_equal(n_inl.cpu().numpy(), want["n_inlier"])
    order = np.zeros((n_img, C), np.int32)
    assert _raw(eng, q_xy, nq, r_xy, n_r, qoff, n_img, C, fwd, mut, 3.0, 0.5, 2.0, n_inl, order=order) == 0
    assert np.array_equal(order, want["order"])


# ---- 6. end to end on a small index -------------------------------------------------------------------------------------------------
def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def small_map():
    """d = 64, 40 reference images x 12 segments with centroids; 8 query images = noisy copies of reference images 3, 8, ... with
    their centroids moved by one similarity per image (+ 0.5 px); candidates: the true image at a random slot among 4 others."""
    rng = np.random.default_rng(13)
    d, S, n_ref = 64, 12, 40
    R = _unit(rng.standard_normal((n_ref * S, d)))
    img = np.repeat(np.arange(n_ref, dtype=np.int32), S)
    r_xy = rng.uniform([0, 0], [320, 240], (n_ref * S, 2))
    true = np.arange(3, 40, 5)[:8]
    rows = (true[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    Q = _unit(R[rows] + 0.15 * rng.standard_normal((len(rows), d)).astype(np.float32) / np.sqrt(d))
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    q_xy = np.zeros((len(rows), 2))
    for b in range(len(true)):
        a, t = _similarity(rng)
        sl = slice(qoff[b], qoff[b + 1])
        p = ((r_xy[rows[sl], 0] + 1j * r_xy[rows[sl], 1]) - t) / a
        q_xy[sl] = np.stack([p.real, p.imag], 1) + rng.normal(0, 0.5, (S, 2))
    cand = np.zeros((len(true), 5), np.int32)
    slot = rng.integers(0, 5, len(true))
    for b, f in enumerate(true):
        others = rng.choice(n_ref - 1, 4, replace=False)
        cand[b] = np.insert(others + (others >= f), slot[b], f)
    return dict(R=R, img=img, r_xy=r_xy, Q=Q, qoff=qoff, q_xy=q_xy, cand=cand, slot=slot, true=true, S=S)


def test_end_to_end_match_then_verify(eng, small_map):
    from revisit_anything_amd.pipeline import SegVLADPipeline

    m = small_map
    pipe = SegVLADPipeline(eng, 112, 140)
    pipe.index_reset()
    Q, q_xy = _dev(m["Q"]), _dev(m["q_xy"])
    half = len(m["R"]) // 2
    pipe.index_add(_dev(m["R"][:half]), m["img"][:half], xy=m["r_xy"][:half])   # in two parts: the table grows with the index
    pipe.index_add(_dev(m["R"][half:]), m["img"][half:], xy=_dev(m["r_xy"][half:]))
    mp = eng.match_pairs(Q, m["qoff"], m["cand"], want_rows=True)
    fwd, mut = mp["fwd_idx"].cpu().numpy(), mp["mutual"].cpu().numpy()
    assert mut[np.arange(len(fwd)), np.repeat(m["slot"], m["S"])].mean() > 0.9    # (the true image's rows do pair up)
    vp = eng.verify_pairs(q_xy, _dev(m["r_xy"]), m["qoff"], mp["fwd_idx"], mp["mutual"], 3.0, want_rows=True)
    got = {k: v.cpu().numpy() for k, v in vp.items()}
    _check(got, V.verify_pairs(m["q_xy"], m["r_xy"], m["qoff"], fwd, mut, 3.0))
    assert np.array_equal(got["order"][:, 0], m["slot"])

    def pipeline_agrees(r_xy_now, expect_true):
        pred, n_inl, n_mut = pipe.verify(Q, m["qoff"], m["cand"], q_xy, 3.0)
        lv = pipe.last_verify
        f, u = lv["match"]["fwd_idx"].cpu().numpy(), lv["match"]["mutual"].cpu().numpy()
        o1 = lv["match"]["order"].cpu().numpy().astype(np.int64)
        row_o1 = np.repeat(o1, m["S"], axis=0)
        want = V.verify_pairs(m["q_xy"], r_xy_now, m["qoff"], np.take_along_axis(f, row_o1, 1), np.take_along_axis(u, row_o1, 1), 3.0)
        gv = {k: v.cpu().numpy() for k, v in lv["verify"].items()}
        for key in ("n_inlier", "pair", "order"):
            assert np.array_equal(gv[key], want[key]), key
        order = np.take_along_axis(o1, want["order"].astype(np.int64), 1)
        assert np.array_equal(pred.cpu().numpy(), np.take_along_axis(m["cand"], order, 1))
        assert np.array_equal(n_inl.cpu().numpy(), np.take_along_axis(want["n_inlier"], want["order"].astype(np.int64), 1))
        assert np.array_equal(n_mut.cpu().numpy(), np.take_along_axis(lv["match"]["n_mutual"].cpu().numpy(), order, 1))
        assert np.array_equal(pred.cpu().numpy()[expect_true, 0], m["true"][expect_true])
        assert (np.diff(n_inl.cpu().numpy().astype(np.int64), axis=1) <= 0).all()

    pipeline_agrees(m["r_xy"], np.arange(len(m["true"])))
    # remove some images -- two true ones, and others in front of the rest: every later row id moves down
    gone = np.array([0, 1, int(m["true"][1]), 20, int(m["true"][5])], np.int32)
    assert pipe.index_remove_images(gone) == len(gone) * m["S"]
    keep = ~np.isin(m["img"], gone)
    pipeline_agrees(m["r_xy"][keep], np.array([b for b, f in enumerate(m["true"]) if f not in gone]))
    assert pipe._index_xy.shape == (int(keep.sum()), 2) and np.array_equal(pipe._index_xy.cpu().numpy(), m["r_xy"][keep])
    # rows without centroids: verify refuses until the index is reset
    pipe.index_add(_dev(m["R"][:4]), m["img"][:4])
    with pytest.raises(ValueError):
        pipe.verify(Q, m["qoff"], m["cand"], q_xy, 3.0)
    pipe.index_reset()
    assert pipe._index_xy is None and not pipe._index_rows_without_xy
