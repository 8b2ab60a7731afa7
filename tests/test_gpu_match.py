"""Mutual nearest segments between query images and candidate reference images (segvlad_match_pairs, csrc/match_kernels.hip).

The yardstick is existing code plus tests/fp32_emu.py, never the code under test: per slot the host computes the full A x B matrix
of the device's exact fp32 chain (E.d2(E.row_sumsq(Q), E.row_sumsq(R), E.dot_chain(...))), takes the row minima by (d2, row id) and
the column minima by (d2, query row), marks a pair mutual when the two name each other and d2 < max_d2, and adds the scores
(double)(2.0f - d2) in a Python loop in fp64, in query-row order.  Ids, counts, flags and the order are compared for equality,
fwd_d2 and the scores bit for bit.  The forward half is also compared with segvlad_search_shortlist (k = 1, the slot's image as
the shortlist), code this call does not share."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

from match_ref import _yardstick

pytestmark = pytest.mark.gpu


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _check(got, want):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert set(got) == set(want)
    for key in got:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if key in ("fwd_d2", "score"):                                  # bit for bit
            bits = np.uint32 if key == "fwd_d2" else np.uint64
            assert np.array_equal(got[key].view(bits), want[key].view(bits)), (key, np.argwhere(got[key] != want[key])[:5])
        else:
            assert np.array_equal(got[key], want[key]), (key, np.argwhere(got[key] != want[key])[:5])


def _forward_half_equals_the_shortlist_search(eng, Q, qoff, cand, got):
    for j in range(cand.shape[1]):
        d2, idx = eng.search_shortlist(Q, qoff, np.ascontiguousarray(cand[:, j:j + 1]), 1)
        assert torch.equal(idx[:, 0], got["fwd_idx"][:, j])
        assert torch.equal(d2[:, 0].view(torch.int32), got["fwd_d2"][:, j].view(torch.int32))


def _ragged(seed):
    """The geometry of test_gpu_shortlist._ragged_case, restated -- d = 64, 60 images x 20 rows (image 5 relabelled 70), query images of
    30, 0, 130, 10 and 50 rows -- with images 10 .. 21 relabelled into ONE image of 240 rows (more than a 128-row tile), exact ties
    inside a candidate image and inside a query image, and C = 6 slots per image that hold -1, the id 5 that no row carries, a
    duplicate id and that large image."""
    rng = np.random.default_rng(seed)
    d, per, n_ref_img = 64, 20, 60
    R = _unit(rng.standard_normal((per * n_ref_img, d)).astype(np.float32))
    img = np.repeat(np.arange(n_ref_img, dtype=np.int32), per)
    img[img == 5] = 70                                  # image 5 has no rows; 70 has them
    R[100] = R[300]
    qoff = np.array([0, 30, 30, 160, 170, 220], np.int32)
    Q = _unit(R[rng.integers(0, len(R), qoff[-1])] + 0.2 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    Q[0] = R[300]
    img[(img >= 10) & (img <= 21)] = 10
    assert (img == 10).sum() == 240 and not (img == 5).any()
    R[101] = R[100]                  # two identical rows inside image 70 (rows 100 .. 119)
    R[205] = R[203]                  # ... and inside the large image
    Q[3] = Q[2]                      # two identical query rows in image 0
    Q[40] = R[203]                   # exact duplicates of tied index rows, in the 130-row image, twice
    Q[150] = R[203]
    Q[100] = Q[31]                   # identical query rows in two different groups of the 130-row image
    cand = np.array([[70, 5, 33, 33, -1, 10],
                     [3, 10, -1, 5, 70, 44],      # the image without segments
                     [10, 70, 10, 33, 5, 2],
                     [-1, -1, 5, 5, -1, -1],      # no slot carries rows
                     [59, 10, 0, -1, 70, 59]], np.int32)
    return R, img, qoff, Q, cand


@pytest.mark.parametrize("seed", [2, 7])
def test_ragged_case_against_the_yardstick(eng, seed):
    R, img, qoff, Q, cand = _ragged(seed)
    eng.db_reset()
    eng.db_add(R, img)
    for max_d2 in (np.inf, 1.5, 0.0, np.nan):
        want = _yardstick(Q, R, img, qoff, cand, max_d2)
        got = eng.match_pairs(Q, qoff, cand, max_d2=max_d2, want_rows=True)
        if np.isinf(max_d2):
            filled = want["fwd_idx"] >= 0
            share = float(want["mutual"][filled].mean())
            print(f"[match] ragged seed {seed}: {int(filled.sum())} (row, slot) entries with rows, {share:.3f} mutual")
            assert 0.10 <= share <= 0.90, share          # otherwise the flags test nothing
            _forward_half_equals_the_shortlist_search(eng, Q, qoff, cand, got)
        elif not max_d2 > 0:
            assert not want["mutual"].any() and not want["score"].any()
        _check(got, want)
    # without the per-row outputs, host and device queries alike
    lean = eng.match_pairs(torch.from_numpy(Q).cuda(), qoff, cand, max_d2=1.5)
    assert set(lean) == {"n_mutual", "score", "order"}
    want = _yardstick(Q, R, img, qoff, cand, 1.5)
    _check(lean, {k: want[k] for k in lean})
    # a ragged list of lists is padded to the same array
    _check(eng.match_pairs(Q, qoff, [[int(x) for x in row if x >= 0] for row in cand[:, :4]], max_d2=1.5),
           {k: v for k, v in _yardstick(Q, R, img, qoff, _repad(cand[:, :4]), 1.5).items() if k in lean})


def _repad(c):
    from revisit_anything_amd.engine import pad_candidates

    return pad_candidates([[int(x) for x in row if x >= 0] for row in c])


def test_d1024_interleaved_adds_against_the_yardstick(eng):
    rng = np.random.default_rng(21)
    n_ref_img, per, d = 400, 50, 1024
    n = n_ref_img * per
    R = _unit(rng.standard_normal((n, d)).astype(np.float32))
    img = (np.arange(n) % n_ref_img).astype(np.int32)                   # interleaved: no image's rows are contiguous
    eng.db_reset()
    for a, b in ((0, 7000), (7000, 12000), (12000, n)):
        eng.db_add(R[a:b], img[a:b])
    true = rng.choice(n_ref_img, 8, replace=False)
    Q = np.concatenate([R[img == t] for t in true])
    Q = _unit(Q + 0.5 * rng.standard_normal(Q.shape).astype(np.float32) / np.sqrt(d))
    qoff = np.arange(0, 8 * per + 1, per, dtype=np.int32)
    cand = rng.integers(0, n_ref_img, (8, 5)).astype(np.int32)
    cand[np.arange(8), rng.integers(0, 5, 8)] = true
    Qd = torch.from_numpy(Q).cuda()
    got = eng.match_pairs(Qd, qoff, cand, want_rows=True)
    again = eng.match_pairs(Qd, qoff, cand, want_rows=True)
    for key in got:
        assert torch.equal(got[key].view(torch.uint8), again[key].view(torch.uint8)), key
    _check(got, _yardstick(Q, R, img, qoff, cand, np.inf))
    _forward_half_equals_the_shortlist_search(eng, Qd, qoff, cand, got)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_reranking_puts_the_true_image_first(eng, seed):
    from revisit_anything_amd.pipeline import SegVLADPipeline

    rng = np.random.default_rng(seed)
    n_ref_img, per, d = 60, 20, 64
    R = _unit(rng.standard_normal((n_ref_img * per, d)).astype(np.float32))
    img = np.repeat(np.arange(n_ref_img, dtype=np.int32), per)
    eng.db_reset()
    eng.db_add(R, img)
    true = rng.choice(n_ref_img, 12, replace=False)
    Q = np.concatenate([R[img == t] for t in true])
    Q = _unit(Q + 0.05 * rng.standard_normal(Q.shape).astype(np.float32))
    qoff = np.arange(0, 12 * per + 1, per, dtype=np.int32)
    cand = np.empty((12, 6), np.int32)
    for b, t in enumerate(true):
        others = rng.choice(n_ref_img - 1, 5, replace=False)
        cand[b] = np.insert(others + (others >= t), 3, t)
    out = eng.match_pairs(Q, qoff, cand)
    n_mut = out["n_mutual"].cpu().numpy()
    print(f"[match] rerank seed {seed}: true image {n_mut[:, 3].min()} .. {n_mut[:, 3].max()} pairs, best other {np.delete(n_mut, 3, axis=1).max()}")
    assert (out["order"][:, 0] == 3).all() and (n_mut[:, 3] == per).all()
    tight = eng.match_pairs(Q, qoff, cand, max_d2=0.5)["n_mutual"].cpu().numpy()
    assert (tight[:, 3] == per).all() and not np.delete(tight, 3, axis=1).any()
    pipe = SegVLADPipeline(eng, 112, 140)
    pred = torch.from_numpy(cand).cuda()
    re, n_re, sc_re = pipe.rerank(torch.from_numpy(Q).cuda(), qoff, pred)
    assert re.dtype == pred.dtype and (re[:, 0].cpu().numpy() == true).all()
    order = out["order"].to(torch.int64)
    assert torch.equal(re, torch.gather(pred, 1, order)) and torch.equal(n_re, torch.gather(out["n_mutual"], 1, order))
    assert torch.equal(sc_re, torch.gather(out["score"], 1, order)) and (n_re[:, 0] == per).all()
    re_h, _, _ = pipe.rerank(Q, qoff, cand)                             # host candidates: the same list
    assert np.array_equal(re_h.cpu().numpy(), re.cpu().numpy())


def _tile_edges(d, two_tiles):
    """Shapes at the edges of the gathered-row tile's pipeline (csrc/group_tile_dev.h).  d = 32 is ONE k-tile -- the prologue's load
    alone, the loop body runs once without a prefetch --, d = 96 an odd count of three.  Reference images of 1, 128 and 129 rows: one
    live column, a full 128-row tile, a tile and one column (and 42 more rows in a fourth image that no slot names).  Query images
    of 1 and 32 rows take one accumulator tile per wave, of 33 and 64 rows two: the kernel is chosen per CALL by the longest group,
    so the two pairs are two cases.  Every query image meets every reference image."""
    rng = np.random.default_rng(300 + d + int(two_tiles))
    img = np.repeat(np.arange(4, dtype=np.int32), [1, 128, 129, 42])
    R = _unit(rng.standard_normal((len(img), d)).astype(np.float32))
    rows = (33, 64) if two_tiles else (1, 32)
    qoff = np.array([0, rows[0], rows[0] + rows[1]], np.int32)
    Q = _unit(R[rng.integers(0, len(R), qoff[-1])] + 0.2 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    cand = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    return R, img, qoff, Q, cand


@pytest.mark.parametrize("two_tiles", [False, True], ids=["rows_1_32", "rows_33_64"])
@pytest.mark.parametrize("d", [32, 96])
def test_tile_edges_against_the_yardstick(eng, d, two_tiles):
    R, img, qoff, Q, cand = _tile_edges(d, two_tiles)
    eng.db_reset()
    eng.db_add(R, img)
    want = _yardstick(Q, R, img, qoff, cand, np.inf)
    share = float(want["mutual"].mean())
    print(f"[match] tile edges d={d} rows {np.diff(qoff).tolist()}: {want['mutual'].size} (row, slot) entries, {share:.3f} mutual")
    assert (want["fwd_idx"] >= 0).all() and 0.10 <= share <= 0.90, share   # otherwise the flags test nothing
    got = eng.match_pairs(Q, qoff, cand, want_rows=True)
    _check(got, want)
    _forward_half_equals_the_shortlist_search(eng, Q, qoff, cand, got)
    lim = 1.0 if d == 32 else 1.5                       # (cuts the mutual pairs to 0.29 .. 0.49 of the entries)
    _check(eng.match_pairs(Q, qoff, cand, max_d2=lim, want_rows=True), _yardstick(Q, R, img, qoff, cand, lim))


def test_live_index(eng):
    R, img, qoff, Q, cand = _ragged(4)
    eng.db_reset()
    eng.db_add(R, img)
    gone_rows = np.array([200, 201, 207, 230, 260, 300, 301, 419, 439], np.int64)   # scattered rows of the 240-row image 10
    assert (img[gone_rows] == 10).all()
    removed = eng.db_remove(row_ids=gone_rows, img_ids=np.array([70], np.int32))    # ... and the candidate image 70 as a whole
    keep = np.ones(len(R), bool)
    keep[gone_rows] = False
    keep[img == 70] = False
    assert removed == int((~keep).sum())
    R2, img2 = R[keep], img[keep]                                       # the survivors, renumbered 0 .. n' - 1 in their order
    got = eng.match_pairs(Q, qoff, cand, want_rows=True)
    _check(got, _yardstick(Q, R2, img2, qoff, cand, np.inf))
    assert (got["fwd_idx"][:, 0][:30] == -1).all()                      # slot (0, 0) named image 70
    rng = np.random.default_rng(5)
    extra = _unit(Q[rng.integers(0, len(Q), 90)] + 0.1 * rng.standard_normal((90, R.shape[1])).astype(np.float32))
    extra_img = np.repeat(np.array([70, 10, 5], np.int32), 30)          # image 70 returns, 10 grows, 5 gets its first rows
    eng.db_add(extra, extra_img)
    R3, img3 = np.concatenate([R2, extra]), np.concatenate([img2, extra_img])
    for max_d2 in (np.inf, 0.7):
        _check(eng.match_pairs(Q, qoff, cand, max_d2=max_d2, want_rows=True), _yardstick(Q, R3, img3, qoff, cand, max_d2))


def test_errors(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_LIMIT, SEGVLAD_ERR_STATE, SegVLADError
    from revisit_anything_amd.engine import _ptr

    rng = np.random.default_rng(9)
    R = _unit(rng.standard_normal((200, 64)).astype(np.float32))
    Q = R[:10].copy()
    qoff = np.array([0, 10], np.int32)
    cand = np.array([[1, 2]], np.int32)
    eng.db_reset()
    with pytest.raises(SegVLADError) as e:                              # no dimension yet
        eng.match_pairs(Q, qoff, cand)
    assert e.value.code == SEGVLAD_ERR_STATE
    eng.db_add(R)
    with pytest.raises(SegVLADError) as e:                              # no img_of_seg map
        eng.match_pairs(Q, qoff, cand)
    assert e.value.code == SEGVLAD_ERR_STATE
    eng.db_reset()
    eng.db_add(_unit(rng.standard_normal((40, 48)).astype(np.float32)), np.repeat(np.arange(4, dtype=np.int32), 10))
    with pytest.raises(SegVLADError) as e:
        eng.match_pairs(np.ascontiguousarray(R[:10, :48]), qoff, cand)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    eng.db_reset()
    eng.db_add(R, np.repeat(np.arange(10, dtype=np.int32), 20))
    n_mut = torch.zeros((1, 65), dtype=torch.int32, device="cuda:0")
    score = torch.zeros((1, 65), dtype=torch.float64, device="cuda:0")
    wide = np.zeros((1, 65), np.int32)

    def call(q, nq, qo, n_img, cd, C, nm=n_mut, sc=score):
        eng._stream()
        return eng.lib.segvlad_match_pairs(eng._h, _ptr(q), nq, _ptr(qo), n_img, _ptr(cd), C, float("inf"), _ptr(nm), _ptr(sc),
                                           None, None, None, None)

    assert call(Q, 10, qoff, 1, wide, 0) == SEGVLAD_ERR_ARG
    assert call(Q, 10, qoff, 1, wide, 65) == SEGVLAD_ERR_ARG
    assert call(Q, 10, np.array([0, 9], np.int32), 1, cand, 2) == SEGVLAD_ERR_ARG      # nq != qseg_offsets[n_img]
    assert call(Q, 10, np.array([1, 10], np.int32), 1, cand, 2) == SEGVLAD_ERR_ARG     # does not start at 0
    assert call(Q, 10, np.array([0, 12, 10], np.int32), 2, np.zeros((2, 2), np.int32), 2) == SEGVLAD_ERR_ARG   # decreasing
    assert call(Q, 10, None, 1, cand, 2) == SEGVLAD_ERR_ARG
    assert call(Q, 10, torch.from_numpy(qoff).cuda(), 1, cand, 2) == SEGVLAD_ERR_ARG   # qseg_offsets is host memory
    assert eng.lib.segvlad_last_error(eng._h).decode().startswith("match_pairs: ")
    assert call(Q, 10, qoff, 1, None, 2) == SEGVLAD_ERR_ARG
    assert call(None, 10, qoff, 1, cand, 2) == SEGVLAD_ERR_ARG
    assert call(Q, 10, qoff, 1, cand, 2, nm=None) == SEGVLAD_ERR_ARG
    assert call(Q, 10, qoff, 1, cand, 2, sc=None) == SEGVLAD_ERR_ARG
    assert call(Q, 10, qoff, 1, torch.from_numpy(cand).cuda(), 2) == SEGVLAD_ERR_ARG   # cand is host memory
    assert call(Q, 0, np.array([0, 0], np.int32), 1, cand, 2) == 0                     # nq == 0
    assert call(None, 0, np.array([0], np.int32), 0, None, 2) == 0
    # no query rows, but images: zero counts and scores, the slots that carry rows first (id 40 carries none)
    out = eng.match_pairs(Q[:0], np.array([0, 0, 0], np.int32), np.array([[40, 2, 1], [-1, -1, 3]], np.int32), want_rows=True)
    assert out["n_mutual"].tolist() == [[0, 0, 0], [0, 0, 0]] and out["score"].tolist() == [[0.0] * 3] * 2
    assert out["order"].tolist() == [[1, 2, 0], [2, 0, 1]] and out["fwd_idx"].shape == (0, 3)
    from revisit_anything_amd.pipeline import SegVLADPipeline

    re, n_re, _ = SegVLADPipeline(eng, 112, 140).rerank(Q[:0], np.array([0, 0, 0], np.int32), np.array([[40, 2, 1], [-1, -1, 3]], np.int32))
    assert re.tolist() == [[2, 1, 40], [3, -1, -1]] and not n_re.any()
    assert call(Q, 10, qoff, 1, cand, 2) == 0                                          # NULL optional outputs
    with pytest.raises(ValueError):
        eng.match_pairs(Q, qoff, np.array([[0, -2]], np.int32))
    # Q == the rows of images 0 (first half): every pair is mutual at distance 0, and the stage is timed under its name
    eng.set_profiling(True)
    eng.profile_reset()
    out = eng.match_pairs(R[:20], np.array([0, 20], np.int32), np.array([[3, 0]], np.int32), want_rows=True)
    assert out["n_mutual"][0, 1] == 20 and out["mutual"][:, 1].all() and abs(float(out["score"][0, 1]) - 40.0) < 1e-4
    assert out["order"].tolist() == [[1, 0]] and out["fwd_idx"][:, 1].tolist() == list(range(20))
    ms, launches = eng.stage_ms("match_pairs")
    eng.set_profiling(False)
    assert ms > 0 and launches == 2
