"""Re-ranking by consistency along the query sequence (segvlad_sequence_rerank, csrc/sequence_kernels.hip) on the GPU.

The yardstick is tests/sequence_ref.py, a literal NumPy restatement of the contract in include/segvlad.h (its additions one at a
time, in the contract's order), never the code under test.  Every integer output is compared for equality and seq_score for BIT
equality -- also on real-valued scores, where another order of the additions, a fused operation or another choice among the
slots in reach would show."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import sequence_ref as S

pytestmark = pytest.mark.gpu

ERR_ARG = -1
KEYS = ("seq_score", "n_hit", "vel", "order")
VELS = [0.5, 1.0, 1.5, -1.0]


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(eng, cand, score, so=None, back=5, fwd=5, vel=(1.0,), tol=1):
    out = eng.sequence_rerank(_dev(np.asarray(cand, np.int32)), _dev(np.asarray(score, np.float64)), so, back, fwd, list(vel), tol)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, what=""):
    assert set(got) == set(want) == set(KEYS)
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
    for key in KEYS[1:]:
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5])
    a, b = got["seq_score"].view(np.int64), want["seq_score"].view(np.int64)
    assert np.array_equal(a, b), (what, "seq_score", np.argwhere(a != b)[:5])


def _check(eng, cand, score, so=None, back=5, fwd=5, vel=(1.0,), tol=1, what=""):
    got = _run(eng, cand, score, so, back, fwd, vel, tol)
    _same(got, S.sequence_rerank(cand, score, so, back, fwd, vel, tol), what)
    for row in got["order"]:
        assert sorted(row.tolist()) == list(range(len(row)))
    return got


def _raw(eng, cand, score, T, C, so, n_seq, back, fwd, vel, n_vel, tol, ss, nh=None, vo=None, od=None):
    from revisit_anything_amd.engine import _ptr

    eng._stream()
    return eng.lib.segvlad_sequence_rerank(eng._h, _ptr(cand), _ptr(score), T, C, _ptr(so), n_seq, back, fwd, _ptr(vel), n_vel, tol,
                                           _ptr(ss), _ptr(nh), _ptr(vo), _ptr(od))


def _real_case(seed, T, C, lo=0, hi=200, empty=0.0):
    """Ids of lo .. hi -- most lookups hit and several slots match --, scores of (0, 1) with all 52 bits in use."""
    rng = np.random.default_rng(seed)
    cand = rng.integers(lo, hi + 1, (T, C)).astype(np.int32)
    score = rng.random((T, C))
    if empty:
        cand[rng.random((T, C)) < empty] = -1
    return cand, score


# ---- 1. the planted traversal: logic only, every sum is exact ---------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0, 1])
@pytest.mark.parametrize("v_true", VELS)
def test_planted_case_equals_the_reference(eng, v_true, tol):
    cand, score, slot = S.planted_case(v_true)
    got = _check(eng, cand, score, [0, 17, 40], 5, 5, VELS, tol)
    assert np.array_equal(got["order"][:, 0], slot) and (got["vel"][np.arange(40), slot] == VELS.index(v_true)).all()


# ---- 2. real-valued scores: the order of the additions ---------------------------------------------------------------------------
def test_largest_window_real_scores(eng):
    """T = 70, C = 64, back = fwd = 32 (the largest window and LDS footprint), 16 velocities, tol = 3, ids of 0 .. 200."""
    cand, score = _real_case(1, 70, 64)
    got = _check(eng, cand, score, None, 32, 32, np.linspace(-1.5, 2.25, 16), 3)
    assert got["n_hit"].max() == 64 and len(np.unique(got["vel"])) > 8     # (full windows, and the velocities matter)


@pytest.mark.parametrize("C", [1, 5, 63, 64])
def test_list_widths(eng, C):
    """C = 1, 5 (with -1 padding and 0.0 scores behind the filled slots, as the vote pads), 63, 64; two sequences, the frames of
    several workgroups, an asymmetric window."""
    cand, score = _real_case(10 + C, 150, C, 0, 60 if C < 8 else 200)
    if C == 5:
        fill = np.random.default_rng(3).integers(0, 6, 150)
        pad = np.arange(5)[None, :] >= fill[:, None]
        cand[pad], score[pad] = -1, 0.0
    _check(eng, cand, score, [0, 61, 150], 7, 3, [0.8, 1.0, 1.25], 1, what=f"C={C}")


def test_empty_frames_and_non_finite_scores(eng):
    """Whole frames without a candidate (they support nobody and no window stops at them), NaN and +-inf scores as empty slots."""
    cand, score = _real_case(2, 60, 6, 0, 40, empty=0.2)
    cand[[0, 7, 8, 30, 59]] = -1
    rng = np.random.default_rng(4)
    for val in (np.nan, np.inf, -np.inf):
        score[rng.random(score.shape) < 0.08] = val
    score[20] = np.nan
    got = _check(eng, cand, score, None, 4, 4, [1.0, 0.5], 2)
    e = S.empty_slots(cand, score)
    assert e[[0, 7, 8, 20, 30, 59]].all() and 0.2 < e.mean() < 0.7
    assert not got["seq_score"][e].any() and (got["vel"][e] == -1).all() and (got["vel"][~e] >= 0).all()
    assert np.array_equal(got["order"][20], np.arange(6))


def test_duplicate_ids_get_the_same_answer_twice(eng):
    cand, score = _real_case(5, 40, 8, 0, 30)
    cand[:, 5], score[:, 5] = cand[:, 2], score[:, 2]        # the same id with the same score: the same sums
    cand[:, 7] = cand[:, 0]                                  # the same id with another score: the same support, another own score
    got = _check(eng, cand, score, None, 3, 3, [1.0, 1.1], 1)
    assert np.array_equal(got["seq_score"][:, 5].view(np.int64), got["seq_score"][:, 2].view(np.int64))
    assert np.array_equal(got["n_hit"][:, 7], got["n_hit"][:, 0]) and np.array_equal(got["vel"][:, 5], got["vel"][:, 2])
    assert (np.argsort(got["order"], axis=1)[:, 2] < np.argsort(got["order"], axis=1)[:, 5]).all()      # ties: the lower slot first


def test_short_sequences_and_windows_longer_than_their_sequence(eng):
    """Sequences of 0, 1, 2 frames between longer ones; back = fwd = 32 exceed every sequence."""
    so = [0, 0, 1, 3, 3, 3, 20, 21, 21, 50, 50]
    cand, score = _real_case(6, 50, 7, 0, 50)
    got = _check(eng, cand, score, so, 32, 32, [1.0, -1.0, 0.0], 2)
    assert np.array_equal(got["seq_score"][0].view(np.int64), score[0].view(np.int64)) and not got["n_hit"][[0, 20]].any()
    assert got["n_hit"][1:3].max() <= 1 and got["n_hit"][3:20].max() <= 16 and got["n_hit"][21:].max() <= 28


def test_no_window_is_the_identity(eng):
    """back = fwd = 0: seq_score equals score bit for bit, n_hit = 0, the order is by score."""
    cand, score = _real_case(7, 33, 9, empty=0.1)
    score[3, :4] = score[3, 4]                               # ties keep the slot order
    got = _check(eng, cand, score, None, 0, 0, [1.0, 2.0], 5)
    e = cand < 0
    assert np.array_equal(got["seq_score"][~e].view(np.int64), score[~e].view(np.int64)) and not got["n_hit"].any()
    assert (got["vel"][~e] == 0).all()
    for t in range(33):
        assert got["order"][t].tolist() == sorted(range(9), key=lambda c: (e[t, c], -score[t, c] if not e[t, c] else 0.0, c))


def test_a_row_depends_on_its_window_alone(eng):
    """Row t of a call equals the row of a call over frames t - back .. t + fwd alone, as one sequence."""
    cand, score = _real_case(8, 45, 11, 0, 80)
    back, fwd, vel = 6, 4, [0.9, 1.0, 1.1, 1.2]
    full = _run(eng, cand, score, None, back, fwd, vel, 2)
    for t in (0, 3, 6, 22, 40, 44):
        a, b = max(0, t - back), min(45, t + fwd + 1)
        part = _run(eng, cand[a:b], score[a:b], None, back, fwd, vel, 2)
        _same({k: v[t - a:t - a + 1] for k, v in part.items()}, {k: v[t:t + 1] for k, v in full.items()}, what=f"t={t}")


def test_shifted_ids_and_ids_next_to_int32_max(eng):
    """Adding a constant to every id changes nothing; next to INT32_MAX with positive velocities p = r + rint(v tau) passes 2^31
    and must not wrap (it lives in int64)."""
    cand, score = _real_case(9, 40, 10, 0, 120)
    cand[39, 0] = 120
    vel = [1.0, 2.0, 3.5]
    base = _check(eng, cand, score, [0, 25, 40], 5, 5, vel, 2)
    top = np.iinfo(np.int32).max
    for shift in (1_000_000, top - 120):
        moved = (cand.astype(np.int64) + shift).astype(np.int32)
        assert moved.min() >= 0 and (shift < top - 120 or moved.max() == top)
        _same(_check(eng, moved, score, [0, 25, 40], 5, 5, vel, 2), base, what=f"shift={shift}")
    got = _check(eng, np.full((6, 2), top, np.int32), np.ones((6, 2)), None, 2, 2, [2.0], 2 ** 30)   # tol at its limit: p + tol beyond 2^31
    assert got["n_hit"].tolist() == [[2, 2], [3, 3], [4, 4], [4, 4], [3, 3], [2, 2]]


def test_reversed_sequence_with_negated_velocities(eng):
    """Integer scores (every sum exact in any order): reversing a sequence while negating the velocities and swapping back / fwd
    gives the same scores and hit counts, frame for frame."""
    rng = np.random.default_rng(12)
    cand = rng.integers(0, 60, (37, 8)).astype(np.int32)
    score = rng.integers(0, 9, (37, 8)).astype(np.float64)
    vel = np.array([1.0, 0.5, 1.5, -2.0])
    a = _check(eng, cand, score, None, 6, 2, vel, 1)
    b = _check(eng, cand[::-1].copy(), score[::-1].copy(), None, 2, 6, -vel, 1)
    assert np.array_equal(a["seq_score"], b["seq_score"][::-1]) and np.array_equal(a["n_hit"], b["n_hit"][::-1])
    assert a["n_hit"].max() >= 6


# ---- 3. the call: pointers, optional outputs, determinism, errors ----------------------------------------------------------------
def test_host_and_device_pointers_null_outputs_and_determinism(eng):
    cand, score = _real_case(13, 90, 20, 0, 150, empty=0.05)
    so, vel = np.array([0, 40, 90], np.int32), np.array([0.8, 1.0, 1.2])
    want = S.sequence_rerank(cand, score, so, 5, 5, vel, 1)
    # host inputs and host outputs
    h = {"seq_score": np.full((90, 20), 7.0), "n_hit": np.full((90, 20), 7, np.int32), "vel": np.full((90, 20), 7, np.int32),
         "order": np.full((90, 20), 7, np.int32)}
    assert _raw(eng, cand, score, 90, 20, so, 2, 5, 5, vel, 3, 1, h["seq_score"], h["n_hit"], h["vel"], h["order"]) == 0
    _same(h, want, "host")
    # device inputs and outputs, twice: the same bits; then every optional output NULL, and each one alone
    dc, ds = _dev(cand), _dev(score)
    runs = []
    for _ in range(2):
        d = {"seq_score": torch.full((90, 20), 7.0, dtype=torch.float64, device="cuda"), "n_hit": torch.full((90, 20), 7, dtype=torch.int32, device="cuda"),
             "vel": torch.full((90, 20), 7, dtype=torch.int32, device="cuda"), "order": torch.full((90, 20), 7, dtype=torch.int32, device="cuda")}
        assert _raw(eng, dc, ds, 90, 20, so, 2, 5, 5, vel, 3, 1, d["seq_score"], d["n_hit"], d["vel"], d["order"]) == 0
        runs.append({k: v.cpu().numpy() for k, v in d.items()})
    _same(runs[0], want, "device")
    _same(runs[1], runs[0], "second call")
    ss = torch.full((90, 20), 7.0, dtype=torch.float64, device="cuda")
    assert _raw(eng, dc, ds, 90, 20, so, 2, 5, 5, vel, 3, 1, ss) == 0
    assert np.array_equal(ss.cpu().numpy().view(np.int64), want["seq_score"].view(np.int64))
    for pos, key in ((0, "n_hit"), (1, "vel"), (2, "order")):
        outs = [None, None, None]
        outs[pos] = torch.full((90, 20), 7, dtype=torch.int32, device="cuda")
        assert _raw(eng, dc, ds, 90, 20, so, 2, 5, 5, vel, 3, 1, ss, *outs) == 0
        assert np.array_equal(outs[pos].cpu().numpy(), want[key]), key
    # mixed: device inputs, a host output
    ho = np.full((90, 20), 7, np.int32)
    assert _raw(eng, dc, ds, 90, 20, so, 2, 5, 5, vel, 3, 1, ss, None, None, ho) == 0 and np.array_equal(ho, want["order"])
    # the engine's short form
    short = eng.sequence_rerank(dc, ds, so, 5, 5, vel, 1, want_all=False)
    assert sorted(short) == ["order", "seq_score"] and np.array_equal(short["order"].cpu().numpy(), want["order"])


def test_every_argument_error_leaves_the_context_usable(eng):
    from revisit_anything_amd._lib import SegVLADError

    cand, score = _real_case(14, 12, 4, 0, 20)
    dc, ds = _dev(cand), _dev(score)
    ss = torch.zeros((12, 4), dtype=torch.float64, device="cuda")
    so, vel = np.array([0, 5, 12], np.int32), np.array([1.0, 1.1])
    good = dict(cand=dc, score=ds, T=12, C=4, so=so, n_seq=2, back=2, fwd=2, vel=vel, n_vel=2, tol=1, ss=ss)
    bad_cases = [dict(cand=None), dict(score=None), dict(ss=None), dict(so=None), dict(vel=None), dict(T=-1), dict(n_seq=-1), dict(C=0), dict(C=65),
                 dict(back=-1), dict(back=33), dict(fwd=-1), dict(fwd=33), dict(n_vel=0), dict(n_vel=17), dict(tol=-1), dict(tol=2 ** 30 + 1),
                 dict(vel=np.array([1.0, np.nan])), dict(vel=np.array([np.inf, 1.0])), dict(vel=np.array([1.0, -(2.0 ** 20) - 1.0])),
                 dict(so=np.array([1, 5, 12], np.int32)), dict(so=np.array([0, 5, 11], np.int32)), dict(so=np.array([0, 13, 12], np.int32)),
                 dict(T=11), dict(so=_dev(so)), dict(vel=_dev(vel))]
    for bad in bad_cases:
        a = {**good, **bad}
        rc = _raw(eng, a["cand"], a["score"], a["T"], a["C"], a["so"], a["n_seq"], a["back"], a["fwd"], a["vel"], a["n_vel"], a["tol"], a["ss"])
        assert rc == ERR_ARG, (bad, rc)
        assert b"sequence_rerank" in eng.lib.segvlad_last_error(eng._h)
    with pytest.raises(ValueError):
        eng.sequence_rerank(dc, ds, [0, 5, 11])
    with pytest.raises(SegVLADError):
        eng._check(_raw(eng, dc, ds, 12, 4, so, 2, 2, 2, vel, 2, -1, ss), "sequence_rerank")
    _check(eng, cand, score, so, 2, 2, vel, 1)                      # the context still works
    # the limits themselves are accepted
    _check(eng, cand, score, so, 32, 0, [-(2.0 ** 20), 2.0 ** 20], 2 ** 30)


def test_no_frames(eng):
    vel = np.array([1.0])
    assert _raw(eng, None, None, 0, 4, np.array([0], np.int32), 0, 5, 5, vel, 1, 1, None) == 0
    assert _raw(eng, None, None, 0, 4, np.array([0, 0, 0], np.int32), 2, 5, 5, vel, 1, 1, None) == 0
    assert _raw(eng, None, None, 0, 65, np.array([0], np.int32), 0, 5, 5, vel, 1, 1, None) == ERR_ARG      # (still validated)
    out = eng.sequence_rerank(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    assert sorted(out) == ["n_hit", "order", "seq_score", "vel"] and all(tuple(v.shape) == (0, 3) for v in out.values())


def test_stage_timer(eng):
    cand, score = _real_case(15, 30, 5, 0, 40)
    eng.set_profiling(True)
    eng.profile_reset()
    _run(eng, cand, score)
    eng.synchronize()
    ms, launches = eng.stage_ms("sequence_rerank")
    eng.set_profiling(False)
    assert ms > 0 and launches == 2


# ---- 4. one chain through the index -------------------------------------------------------------------------------------------------
def test_chain_search_vote_sequence(eng):
    """100 images x 20 rows of d = 64; the queries are noisy copies of frames 30 .. 49; search (k = 10) -> sims_from_d2 ->
    vote(n_top = 5, with scores) -> sequence_rerank on the vote's tensors as they are.  The result equals the reference on the
    same tensors, and pipeline.sequence returns the gathered lists."""
    from revisit_anything_amd.pipeline import SegVLADPipeline

    g = torch.Generator(device="cuda:0").manual_seed(5)
    n_img, rows, d = 100, 20, 64
    centres = torch.nn.functional.normalize(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
    R = torch.nn.functional.normalize(centres.repeat_interleave(rows, dim=0) + 0.5 * torch.randn(n_img * rows, d, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    eng.db_reset()
    eng.db_add(R, np.repeat(np.arange(n_img, dtype=np.int32), rows))
    frames = np.arange(30, 50)
    Q = torch.nn.functional.normalize(R[30 * rows:50 * rows] + 0.3 * torch.randn(20 * rows, d, device="cuda:0", generator=g) / d ** 0.5, dim=1).contiguous()
    qoff = np.arange(0, 20 * rows + 1, rows, dtype=np.int32)
    d2, idx = eng.search(Q, 10)
    sims, m = eng.sims_from_d2(d2, idx, 10)
    pred, sc = eng.vote(m, sims, qoff, n_top=5, want_scores=True)
    assert pred.dtype == torch.int32 and sc.dtype == torch.float64 and pred.is_cuda
    out = eng.sequence_rerank(pred, sc, None, 3, 3, None, 1)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = S.sequence_rerank(pred.cpu().numpy(), sc.cpu().numpy(), None, 3, 3, np.linspace(0.8, 1.2, 5), 1)
    _same(got, want, "chain")
    assert np.array_equal(pred.cpu().numpy()[np.arange(20), got["order"][:, 0]], frames)
    assert (got["n_hit"][np.arange(20), got["order"][:, 0]] >= 3).all()
    pipe = SegVLADPipeline(eng, 112, 140)
    pred_seq, seq_score, n_hit = pipe.sequence(pred, sc, back=3, fwd=3)
    o = want["order"].astype(np.int64)
    assert np.array_equal(pred_seq.cpu().numpy(), np.take_along_axis(pred.cpu().numpy(), o, 1))
    assert np.array_equal(seq_score.cpu().numpy().view(np.int64), np.take_along_axis(want["seq_score"], o, 1).view(np.int64))
    assert np.array_equal(n_hit.cpu().numpy(), np.take_along_axis(want["n_hit"], o, 1))
    assert (np.diff(seq_score.cpu().numpy(), axis=1) <= 0).all()
    eng.db_reset()
