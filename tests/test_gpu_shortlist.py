"""Shortlist-restricted exact search (segvlad_search_shortlist, csrc/shortlist_kernels.hip): per query image, the exact top-k
over the rows of its shortlisted reference images.  Every distance is the device's exact fp32 chain (tests/fp32_emu.py), so
the results are compared BIT for bit -- against segvlad_search when the shortlist holds every image, and against a host
brute force of the emulated chain, ordered by (distance, id), otherwise."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

from shortlist_cases import _brute

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
    gd, gi = (t.cpu().numpy() for t in got)
    wd, wi = want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("geometry", ["20000x1024", "3000x256_three_adds", "300x64_smaller_than_k"])
def test_full_shortlist_equals_full_search(eng, geometry):
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
        img = (np.arange(n) % 37).astype(np.int32)      # interleaved: no image's rows are contiguous
        eng.db_reset()
        for a, b in ((0, 1000), (1000, 1700), (1700, 3000)):
            eng.db_add(R[a:b], img[a:b])
    n_img_ref = int(img.max()) + 1
    qoff = np.array([0, 50, 50, 180, 230], np.int32)   # an image without segments, one with 130
    Q = _unit(R[rng.integers(0, n, qoff[-1])] + 0.05 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    Q[7] = R[11]                                        # an exact duplicate: distance 0
    full = np.tile(np.arange(n_img_ref, dtype=np.int32), (len(qoff) - 1, 1))
    for k in (1, 50, 200, 1024):
        want = eng.search(Q, k)
        got = eng.search_shortlist(Q, qoff, full, k)
        assert torch.equal(got[1], want[1])
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        if k > n:
            assert (got[1][:, n:] == -1).all() and torch.isinf(got[0][:, n:]).all()


def _ragged_case(seed):
    rng = np.random.default_rng(seed)
    d, per, n_ref_img = 64, 20, 60
    R = _unit(rng.standard_normal((per * n_ref_img, d)).astype(np.float32))
    img = np.repeat(np.arange(n_ref_img, dtype=np.int32), per)
    img[img == 5] = 70                                  # image 5 has no rows; 70 has them
    R[100] = R[300]                                     # planted exact ties (two images)
    R[101] = R[300]
    qoff = np.array([0, 30, 30, 160, 170, 220], np.int32)
    Q = _unit(R[rng.integers(0, len(R), qoff[-1])] + 0.2 * rng.standard_normal((qoff[-1], d)).astype(np.float32))
    Q[0] = R[300]
    M = 14
    sl = rng.integers(0, 71, (len(qoff) - 1, M)).astype(np.int32)
    sl[0, 0:3] = (5, 15, 15)                           # id without rows, duplicates
    sl[0, 3:6] = (img[100], img[101], img[300])
    sl[1, 4:] = -1
    sl[3, 1:] = -1                                      # one image: a union of 20 rows (< k below)
    sl[2, :12] = np.arange(12) + 10                     # 240 rows: more than a 128-row tile
    return R, img, qoff, Q, sl


def test_ragged_shortlists_against_brute_force(eng):
    R, img, qoff, Q, sl = _ragged_case(2)
    eng.db_reset()
    eng.db_add(R, img)
    for k in (5, 50):
        _check(eng.search_shortlist(Q, qoff, sl, k), _brute(Q, R, img, qoff, sl, k))
    # the same through a device shortlist
    _check(eng.search_shortlist(torch.from_numpy(Q).cuda(), qoff, torch.from_numpy(sl).cuda(), 50), _brute(Q, R, img, qoff, sl, 50))


def test_index_updates_rebuild_the_map(eng):
    R, img, qoff, Q, sl = _ragged_case(3)
    eng.db_reset()
    eng.db_add(R[:600], img[:600])
    _check(eng.search_shortlist(Q, qoff, sl, 30), _brute(Q, R[:600], img[:600], qoff, sl, 30))
    extra = img[600:].copy()
    extra[::3] = 2                                      # image 2 gains rows far from its first ones
    eng.db_add(R[600:], extra)
    img2 = np.concatenate([img[:600], extra])
    _check(eng.search_shortlist(Q, qoff, sl, 30), _brute(Q, R, img2, qoff, sl, 30))
    R3, img3, _, _, _ = _ragged_case(4)
    img3 = img3[::-1].copy()
    eng.db_reset()
    eng.db_add(R3, img3)
    _check(eng.search_shortlist(Q, qoff, sl, 30), _brute(Q, R3, img3, qoff, sl, 30))


def test_argument_errors(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_STATE, SegVLADError

    rng = np.random.default_rng(5)
    R = _unit(rng.standard_normal((200, 64)).astype(np.float32))
    Q = R[:10].copy()
    qoff = np.array([0, 10], np.int32)
    eng.db_reset()
    eng.db_add(R)
    with pytest.raises(SegVLADError) as e:
        eng.search_shortlist(Q, qoff, np.full((1, 1), -1, np.int32), 5)
    assert e.value.code == SEGVLAD_ERR_STATE
    eng.db_reset()
    eng.db_add(R, np.repeat(np.arange(10, dtype=np.int32), 20))
    dev = torch.zeros((1, 1), dtype=torch.int32, device="cuda:0")
    for bad_qoff, sl, k in ((qoff, torch.zeros((1, 4097), dtype=torch.int32, device="cuda:0"), 5),
                            (qoff, dev, 0), (qoff, dev, 1025),
                            (np.array([0, 9], np.int32), dev, 5), (np.array([1, 10], np.int32), dev, 5)):
        with pytest.raises(SegVLADError) as e:
            eng.search_shortlist(Q, bad_qoff, sl, k)
        assert e.value.code == SEGVLAD_ERR_ARG
    d2 = torch.empty((10, 5), dtype=torch.float32, device="cuda:0")
    idx = torch.empty((10, 5), dtype=torch.int64, device="cuda:0")
    dec, dev_qoff = np.array([0, 12, 10], np.int32), torch.from_numpy(qoff).cuda()
    for bad_qoff, n_img in ((dec.ctypes.data, 2), (None, 1), (dev_qoff.data_ptr(), 1)):   # a decrease; null; a device pointer
        sl = torch.zeros((n_img, 1), dtype=torch.int32, device="cuda:0")
        assert eng.lib.segvlad_search_shortlist(eng._h, Q.ctypes.data, 10, bad_qoff, n_img, sl.data_ptr(), 1, 5, d2.data_ptr(),
                                                idx.data_ptr()) == SEGVLAD_ERR_ARG
        assert eng.lib.segvlad_last_error(eng._h).decode().startswith("search_shortlist: ")
    for ids in ([[-2]], [[10]]):
        with pytest.raises(ValueError):
            eng.search_shortlist(Q, qoff, np.array(ids, np.int32), 5)


def _oracle_vote(idx, sims, qoff, img, n):
    """The oracle's weighted Borda count over the filled slots (id >= 0), extrema over those slots."""
    from oracle import segvlad_oracle as O

    valid = idx >= 0
    smin, smax = np.min(sims[valid]), np.max(sims[valid])
    preds, scores = [], []
    for b in range(len(qoff) - 1):
        mp, sp = idx[qoff[b]:qoff[b + 1]].T, sims[qoff[b]:qoff[b + 1]].T
        pair = [[(int(img[i]), float((s - smin) / (smax - smin))) for i, s in zip(mr, sr) if i >= 0] for mr, sr in zip(mp, sp)]
        ranked, sc = O.weighted_borda_count(*pair)
        preds.append(ranked[:n])
        scores.append([sc[r] for r in ranked[:n]])
    return preds, scores


def test_retrieve_with_a_shortlist(eng):
    from revisit_anything_amd.pipeline import SegVLADPipeline

    R, img, qoff, Q, sl = _ragged_case(6)
    qoff = np.array([0, 30, 160, 170, 220], np.int32)   # (every image votes)
    sl = np.delete(sl, 1, axis=0)
    eng.db_reset()
    eng.db_add(R, img)
    pipe = SegVLADPipeline(eng, 112, 140)
    pred, sc, m, sims = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5, want_scores=True, shortlist=sl)
    bd, bi = _brute(Q, R, img, qoff, sl, 40)
    assert np.array_equal(m.cpu().numpy(), bi[:, :25])
    osims = np.where(bi[:, :25] >= 0, (2 - bd[:, :25]).astype(np.float32), -np.inf).astype(np.float32)
    assert np.array_equal(sims.cpu().numpy(), osims)
    opred, oscore = _oracle_vote(bi[:, :25], osims, qoff, img, 5)
    pred, sc = pred.cpu().numpy(), sc.cpu().numpy()
    for b in range(len(qoff) - 1):
        assert pred[b, :len(opred[b])].tolist() == opred[b]
        assert np.array_equal(sc[b, :len(oscore[b])], np.array(oscore[b]))
    # every image in every shortlist: the plain retrieval's predictions
    full = np.tile(np.unique(img), (len(qoff) - 1, 1)).astype(np.int32)
    p0, _, _, _ = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5)
    p1, _, _, _ = pipe.retrieve(Q, qoff, k_search=40, k_vote=25, n_top=5, shortlist=full)
    assert torch.equal(p0, p1)


def test_two_stage_rerank(eng, tmp_path):
    from revisit_anything_amd import driver, func_vpr, store as st, synth
    from revisit_anything_amd.pipeline import SegVLADPipeline

    K, D, H, W = 8, 64, 112, 140
    N = (H // 14) * (W // 14)
    C = synth.make_vocab(K, D, seed=41)
    rng = np.random.default_rng(42)
    n_ref, n_q = 12, 6
    tau = rng.permutation(n_ref)[:n_q]

    def make(split, n):
        droot, mroot = str(tmp_path / f"{split}_dino"), str(tmp_path / f"{split}_masks")
        keys = []
        for i in range(n):
            key = f"img_{i}.jpg"
            base = i if split == "ref" else int(tau[i])
            t = synth.make_tokens(C, N, seed=5000 + base, noise=0.3)
            if split == "q":
                t = t + 0.05 * np.random.default_rng(777 + i).standard_normal(t.shape).astype(np.float32)
            S = int(rng.integers(4, 8))
            m = synth.make_masks(S, H // 2, W // 2, seed=6000 + base, hmin=6, hmax=30, wmin=6, wmax=40)[:S]
            st.write_dino(droot, key, t.reshape(1, D, H // 14, W // 14))
            st.write_masks(mroot, key, m)
            keys.append(key)
        return st.FeatureStore(droot, "dino"), st.FeatureStore(mroot, "masks"), keys

    dr, mr, kr = make("ref", n_ref)
    dq, mq, kq = make("q", n_q)
    gt = [[int(t)] for t in tau]
    g_ref = func_vpr.aggFt(dr, None, None, None, "vlad", vlad=C)
    g_q = func_vpr.aggFt(dq, None, None, None, "vlad", vlad=C)
    sl = driver.shortlist_from_global(g_ref, g_q, 3)
    assert sl.shape == (n_q, 3) and sl.dtype == np.int32 and ((sl >= 0) & (sl < n_ref)).all()
    eng.set_vocab(C)
    pipe = SegVLADPipeline(eng, H, W, 14, order=2, use_pca=False)
    _, p_plain, _, _ = driver.run_segloc(dr, mr, kr, dq, mq, kq, gt, pipe, batch_size=5, n_top=3, k_search=20, k_vote=10)
    _, p_sl, _, _ = driver.run_segloc(dr, mr, kr, dq, mq, kq, gt, pipe, batch_size=5, n_top=3, k_search=20, k_vote=10, shortlist=sl)
    assert all(set(p_sl[i][p_sl[i] >= 0].tolist()) <= set(sl[i].tolist()) for i in range(n_q))
    sl_all = driver.shortlist_from_global(g_ref, g_q, n_ref)
    _, p_all, _, _ = driver.run_segloc(dr, mr, kr, dq, mq, kq, gt, pipe, batch_size=5, n_top=3, k_search=20, k_vote=10,
                                       shortlist=sl_all)
    assert np.array_equal(p_all, p_plain)
