"""Query-sharded retrieval on the device engine (sharded.QueryShardedRetrieval, segvlad_vote_global): every rank holds the
whole index and votes on its own block of query images with the GLOBAL similarity extrema (func_vpr.py:211-214).
Invariant: gathered predictions, fp64 scores and match lists equal a single index's, bit for bit.

* world 2 through the C-ABI's communicator on the test-only RCCL stand-in (tests/rccl_stub/, SEGVLAD_RCCL_LIB), a rank
  without images, equal similarities (max == min), and a rank whose vote fails on its arguments;
* world 2 and 4 through torch.distributed gloo (at most 4 processes with the GPU open);
* world 1 on the real RCCL: segvlad_vote_global == segvlad_vote with NaN extrema;
* world 8 emulated in ONE process: eight contexts, the exchange done by the test."""
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "rccl_stub")
STUB = os.path.join(STUB_DIR, "librccl_stub.so")
K_SEARCH, K_VOTE, N_TOP = 60, 50, 5


def _problem(n_query_images=12):
    """300 reference images of 20 segments; query images alternate near / far (per-rank extrema would differ)."""
    from revisit_anything_amd import synth

    n_img, S = 300, 20
    R, img = synth.make_planted_db(n_img, S, 64, seed=3100)
    Qs, off = [], [0]
    for i in range(n_query_images):
        Q, _, _ = synth.make_planted_queries(R, n_img, S, 1, seed=4100 + i, sigma_q=(0.5, 3.0)[i % 2])
        Qs.append(Q)
        off.append(off[-1] + Q.shape[0])
    return R, img, np.concatenate(Qs), np.array(off, np.int32)


def _single(n_query_images=12):
    from revisit_anything_amd.engine import SegVLADEngine

    R, img, Q, off = _problem(n_query_images)
    eng = SegVLADEngine(0)
    eng.db_add(R, img)
    d2, ids = eng.search(Q, K_SEARCH)
    sims, m = eng.sims_from_d2(d2, ids, K_VOTE)
    pred, sc = eng.vote(m, sims, off, n_top=N_TOP)
    out = [x.cpu().numpy() for x in (pred, sc, m, sims)]
    eng.close()
    return out


def _local(Q, off, bounds, rank):
    lo, hi = int(off[bounds[rank]]), int(off[bounds[rank + 1]])
    return Q[lo:hi], (off[bounds[rank]:bounds[rank + 1] + 1] - lo).astype(np.int32)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- world 2 through the C-ABI communicator on the RCCL stand-in ------------------------------------------------------
def _build_stub():
    sys.path.insert(0, STUB_DIR)
    try:
        import build_stub

        build_stub.build()
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"the RCCL test stub cannot be built here: {e}")
    finally:
        sys.path.remove(STUB_DIR)


def _stub_worker(rank, world, out_dir, n_query_images):
    sys.path.insert(0, ROOT)
    os.environ["SEGVLAD_RCCL_LIB"] = STUB
    os.environ.setdefault("SVSTUB_TIMEOUT_S", "30")
    import torch

    from revisit_anything_amd._lib import SegVLADError
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    R, img, Q, off = _problem(n_query_images)
    eng = SegVLADEngine(0)
    uid_file = os.path.join(out_dir, "uid.bin")
    if rank == 0:
        with open(uid_file + ".tmp", "wb") as f:
            f.write(eng.comm_unique_id())
        os.replace(uid_file + ".tmp", uid_file)
    else:
        t0 = time.time()
        while not os.path.exists(uid_file):
            assert time.time() - t0 < 60
            time.sleep(0.01)
    eng.comm_init(open(uid_file, "rb").read(), rank, world)
    assert "rccl_stub" in eng.comm_info()["rccl"]
    qs = QueryShardedRetrieval(eng, rank=rank, world=world, device=eng.device, native_comm=True)
    qs.build(torch.from_numpy(R).to(eng.device), img)
    b = qs.split(n_query_images)
    q_local, off_local = _local(Q, off, b, rank)
    res = {}
    out = qs.retrieve(torch.from_numpy(q_local).to(eng.device), off_local, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True)
    res.update(pred=out["pred"].cpu().numpy(), score=out["score"].cpu().numpy(), m=out["m"].cpu().numpy(),
               sims=out["sims"].cpu().numpy())
    # all similarities equal (max == min): the weights are 0 / 0 on every rank, as in one process
    sims_eq = torch.full_like(out["sims"], 1.25)
    p_eq, s_eq = eng.vote_global(out["m"], sims_eq, off_local, n_top=N_TOP, img_of_seg=qs.img_of_seg)
    res.update(pred_eq=p_eq.cpu().numpy(), score_eq=s_eq.cpu().numpy())
    # rank 1's vote fails on its arguments (n_top = 0): it still joins the exchange, every rank returns an error
    try:
        eng.vote_global(out["m"], out["sims"], off_local, n_top=0 if rank == 1 else N_TOP, img_of_seg=qs.img_of_seg)
        res["error"] = "none"
    except SegVLADError as e:
        res.update(error=str(e), code=int(e.code))
    res["world_after"] = eng.comm_info()["world"]
    out2 = qs.retrieve(torch.from_numpy(q_local).to(eng.device), off_local, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True)
    res.update(pred2=out2["pred"].cpu().numpy(), score2=out2["score"].cpu().numpy())
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    eng.close()


@pytest.mark.parametrize("n_query_images", [12, 1])
def test_cabi_two_ranks_equal_single_index(tmp_path, n_query_images):
    """12 images: 6 + 6; 1 image: rank 0 holds none and contributes (+inf, -inf) to the extrema exchange."""
    import torch.multiprocessing as mp

    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import shard_images

    _build_stub()
    mp.spawn(_stub_worker, args=(2, str(tmp_path), n_query_images), nprocs=2, join=True)
    pred, sc, m, sims = _single(n_query_images)
    b = shard_images(n_query_images, 2)
    R, img, Q, off = _problem(n_query_images)
    # the single-process vote on equal similarities
    eng = SegVLADEngine(0)
    p_eq, s_eq = (x.cpu().numpy() for x in eng.vote(m, np.full_like(sims, 1.25), off, n_top=N_TOP, img_of_seg=img))
    eng.close()
    zs = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]
    for r, z in enumerate(zs):
        for p_, s_ in (("pred", "score"), ("pred2", "score2")):
            assert np.array_equal(z[p_], pred) and np.array_equal(z[s_].view(np.uint64), sc.view(np.uint64))
        lo, hi = int(off[b[r]]), int(off[b[r + 1]])
        assert np.array_equal(z["m"], m[lo:hi]) and np.array_equal(z["sims"], sims[lo:hi])
        # max == min: every weight is 0 / 0 (NaN) on every rank, as in one process.  The ORDER of images whose scores are all
        # NaN is not defined (the vote's arg-best has no total order on NaN, and its runs are collected with atomics), so
        # what must agree is the scores' bits, the number of predictions, and that each is an image the query image hit
        assert np.array_equal(z["score_eq"].view(np.uint64), s_eq[b[r]:b[r + 1]].view(np.uint64))
        assert np.isnan(s_eq[p_eq >= 0]).all()
        for i in range(int(b[r]), int(b[r + 1])):
            got = z["pred_eq"][i - int(b[r])]
            assert (got >= 0).sum() == (p_eq[i] >= 0).sum()
            assert set(got[got >= 0].tolist()) <= set(img[m[int(off[i]):int(off[i + 1])].reshape(-1)].tolist())
        assert int(z["world_after"]) == 2                     # the communicator survived the failed vote
    assert int(zs[1]["code"]) == _lib.SEGVLAD_ERR_ARG and "local step failed" in str(zs[1]["error"])
    assert int(zs[0]["code"]) == _lib.SEGVLAD_ERR_COMM and "rank 1" in str(zs[0]["error"])


# ---- world 2 and 4 through torch.distributed gloo ----------------------------------------------------------------------
def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    R, img, Q, off = _problem(10)
    eng = SegVLADEngine(0)
    qs = QueryShardedRetrieval(eng, device=eng.device)
    qs.build(torch.from_numpy(R).to(eng.device), img)
    b = qs.split(len(off) - 1)
    q_local, off_local = _local(Q, off, b, rank)
    out = qs.retrieve(torch.from_numpy(q_local).to(eng.device), off_local, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), pred=out["pred"].cpu().numpy(), score=out["score"].cpu().numpy(),
             m=out["m"].cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


@pytest.mark.parametrize("world", [2, 4])
def test_gloo_ranks_equal_single_index(tmp_path, world):
    import torch.multiprocessing as mp

    from revisit_anything_amd.sharded import shard_images

    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    pred, sc, m, sims = _single(10)
    R, img, Q, off = _problem(10)
    b = shard_images(10, world)
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert np.array_equal(z["pred"], pred) and np.array_equal(z["score"].view(np.uint64), sc.view(np.uint64))
        assert np.array_equal(z["m"], m[int(off[b[r]]):int(off[b[r + 1]])])


# ---- world 1 on the real RCCL ---------------------------------------------------------------------------------------------
def test_vote_global_world_1_equals_vote():
    import torch

    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    R, img, Q, off = _problem()
    pred, sc, m, sims = _single()
    eng = SegVLADEngine(0)
    qs = QueryShardedRetrieval(eng, rank=0, world=1, device=eng.device, native_comm=True)
    qs.build(torch.from_numpy(R).to(eng.device), img)
    assert eng.comm_info()["world"] == 1
    pg, sg = eng.vote_global(m, sims, off, n_top=N_TOP, img_of_seg=img)
    assert np.array_equal(pg.cpu().numpy(), pred) and np.array_equal(sg.cpu().numpy().view(np.uint64), sc.view(np.uint64))
    out = qs.retrieve(torch.from_numpy(Q).to(eng.device), off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True,
                      n_query_images=len(off) - 1)
    assert np.array_equal(out["pred"].cpu().numpy(), pred) and np.array_equal(out["score"].cpu().numpy().view(np.uint64), sc.view(np.uint64))
    # COUNT mode stays collective and equals the plain vote
    pc, scc = eng.vote(m, sims, off, n_top=N_TOP, mode=1, img_of_seg=img)
    pgc, sgc = eng.vote_global(m, sims, off, n_top=N_TOP, mode=1, img_of_seg=img)
    assert torch.equal(pc, pgc) and torch.equal(scc, sgc)
    eng.comm_destroy()
    # no communicator: exactly segvlad_vote with NaN extrema
    pn, sn = eng.vote_global(m, sims, off, n_top=N_TOP, img_of_seg=img)
    assert np.array_equal(pn.cpu().numpy(), pred) and np.array_equal(sn.cpu().numpy().view(np.uint64), sc.view(np.uint64))
    eng.close()


# ---- world 8 emulated in one process --------------------------------------------------------------------------------------
def test_world_8_emulated_in_one_process():
    """Eight contexts on this GPU, each with the whole index and its block of the 12 query images (four ranks hold one image,
    four hold two); the test does the exchange: local extrema -> exact global min / max -> every rank votes with them."""
    import torch

    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval, shard_images

    W = 8
    R, img, Q, off = _problem()
    pred, sc, m, sims = _single()
    b = shard_images(len(off) - 1, W)
    engs = [SegVLADEngine(0) for _ in range(W)]
    loc, recs = [], []
    for r, eng in enumerate(engs):
        eng.db_add(R, img)
        q_local, off_local = _local(Q, off, b, r)
        d2, ids = eng.search(q_local, K_SEARCH)
        s_r, m_r = eng.sims_from_d2(d2, ids, K_VOTE)
        loc.append((off_local, s_r, m_r))
        recs.append(eng.minmax(s_r).cpu().numpy())
    recs = np.array(recs, np.float32)
    smin, smax = float(recs[:, 0].min()), float(recs[:, 1].max())
    assert smin == float(sims.min()) and smax == float(sims.max())
    preds, scores = [], []
    for eng, (off_local, s_r, m_r) in zip(engs, loc):
        p, s = eng.vote(m_r, s_r, off_local, n_top=N_TOP, smin=smin, smax=smax)
        preds.append(p.cpu().numpy())
        scores.append(s.cpu().numpy())
    assert np.array_equal(np.concatenate(preds), pred)
    assert np.array_equal(np.concatenate(scores).view(np.uint64), sc.view(np.uint64))
    # per-rank extrema would not do: the fixture's near / far images make them change predictions
    own = np.concatenate([eng.vote(m_r, s_r, o, n_top=N_TOP)[0].cpu().numpy() for eng, (o, s_r, m_r) in zip(engs, loc)])
    assert not np.array_equal(own, pred)
    bytes_ = QueryShardedRetrieval.collective_bytes(W, len(off) - 1, N_TOP)
    assert bytes_["extrema_allgather_recv"] == W * 16
    for eng in engs:
        eng.close()
