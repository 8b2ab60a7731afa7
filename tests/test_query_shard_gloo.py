"""Query-sharded retrieval (sharded.QueryShardedRetrieval) on CPU: 2 and 3 gloo processes with an oracle checker backend.

Every rank holds the WHOLE index and retrieves its own contiguous block of query images; the vote's min / max must be the
GLOBAL extrema of all ranks' similarities (func_vpr.py:211-214).  The fixture mixes near (sigma 0.5) and far (sigma 3) query
images, so that each rank's own extrema differ from the global ones and -- as asserted below -- would change the predictions:
the exchange is what makes the gathered predictions and fp64 scores equal a single index's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_sharded_gloo import OracleBackend  # noqa: E402

K_SEARCH, K_VOTE, N_TOP = 20, 10, 3


class QueryOracleBackend(OracleBackend):
    """OracleBackend + minmax and a vote that takes the extrema it is given (NaN: its own), like SegVLADEngine.vote."""

    def minmax(self, sims):
        s = np.asarray(sims, dtype=np.float32)
        return torch.tensor([s.min(), s.max()], dtype=torch.float32)

    def vote(self, m, sims, qoff, n_top=5, mode=0, img_of_seg=None, want_scores=False, smin=float("nan"), smax=float("nan"), **kw):
        m, s = np.asarray(m), np.asarray(sims, dtype=np.float32)
        img = np.asarray(img_of_seg).astype(np.int64)
        lo = np.float32(s.min()) if np.isnan(smin) else np.float32(smin)
        hi = np.float32(s.max()) if np.isnan(smax) else np.float32(smax)
        n_img = len(qoff) - 1
        pred = np.full((n_img, n_top), -1, np.int32)
        sc = np.zeros((n_img, n_top), np.float64)
        for i in range(n_img):
            rows = np.arange(qoff[i], qoff[i + 1])
            mp_, sp = m[rows].T, (s[rows].T - lo) / (hi - lo)   # fp32, as func_vpr.py:214
            pair = [list(zip(img[mp_[k]].tolist(), sp[k].tolist())) for k in range(len(sp))]
            ranked, score = self.O.weighted_borda_count(*pair)
            for j, r in enumerate(ranked[:n_top]):
                pred[i, j], sc[i, j] = r, score[r]
        return torch.from_numpy(pred), torch.from_numpy(sc)


class FailingSearchBackend(QueryOracleBackend):
    def search(self, Q, k):
        raise RuntimeError("injected local search failure")


def make_problem(n_query_images=7):
    """61 reference images of 7 segments; query images alternate near / far from their reference image."""
    from revisit_anything_amd import synth

    R, img = synth.make_planted_db(61, 7, 32, seed=3003)
    Qs, off = [], [0]
    for i in range(n_query_images):
        Q, _, _ = synth.make_planted_queries(R, 61, 7, 1, seed=4000 + 17 * 3 + i, sigma_q=(0.5, 3.0)[i % 2])
        Qs.append(Q)
        off.append(off[-1] + Q.shape[0])
    return R, img, np.concatenate(Qs), np.array(off, np.int32)


def local_slice(Q, off, bounds, rank):
    lo, hi = int(off[bounds[rank]]), int(off[bounds[rank + 1]])
    return Q[lo:hi], (off[bounds[rank]:bounds[rank + 1] + 1] - lo).astype(np.int32)


def worker(rank, world, port, out_dir, n_query_images, failing_rank):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from revisit_anything_amd._lib import SegVLADError
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    R, img, Q, off = make_problem(n_query_images)
    qs = QueryShardedRetrieval(FailingSearchBackend() if rank == failing_rank else QueryOracleBackend())
    qs.build(R, img)
    b = qs.split(len(off) - 1)
    q_local, off_local = local_slice(Q, off, b, rank)
    res = {}
    try:
        out = qs.retrieve(torch.from_numpy(q_local), off_local, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True)
        res.update(pred=out["pred"].numpy(), score=out["score"].numpy(), pred_local=out["pred_local"].numpy())
    except SegVLADError as e:
        res.update(error=str(e), code=int(e.code))
    except RuntimeError as e:
        res.update(error=str(e), code=0)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def single_index(n_query_images=7):
    from revisit_anything_amd.sharded import ShardedSegmentIndex

    R, img, Q, off = make_problem(n_query_images)
    idx = ShardedSegmentIndex(QueryOracleBackend(), rank=0, world=1)
    idx.build(R, img)
    pred, sc, m, sims = idx.retrieve(Q, off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True)
    return pred.numpy(), sc.numpy(), m.numpy(), sims.numpy()


def per_rank_extrema_votes(world, n_query_images=7):
    """What the ranks would predict if each normalised with its OWN min / max (the mistake the exchange prevents)."""
    from revisit_anything_amd.sharded import shard_images

    R, img, Q, off = make_problem(n_query_images)
    _, _, m, sims = single_index(n_query_images)
    b = shard_images(len(off) - 1, world)
    be, preds = QueryOracleBackend(), []
    for r in range(world):
        lo, hi = int(off[b[r]]), int(off[b[r + 1]])
        if hi > lo:
            o = (off[b[r]:b[r + 1] + 1] - lo).astype(np.int32)
            preds.append(be.vote(torch.from_numpy(m[lo:hi]), torch.from_numpy(sims[lo:hi]), o, n_top=N_TOP, img_of_seg=img)[0].numpy())
    return np.concatenate(preds)


@pytest.mark.parametrize("world,n_query_images", [(2, 7), (3, 7), (3, 2)])
def test_query_sharded_equals_single_index(tmp_path, world, n_query_images):
    """(2, 7) and (3, 7): ragged image splits; (3, 2): rank 0 holds no query image at all."""
    from oracle import segvlad_oracle as O
    from revisit_anything_amd.sharded import shard_images

    mp.spawn(worker, args=(world, free_port(), str(tmp_path), n_query_images, -1), nprocs=world, join=True)
    pred, sc, m, sims = single_index(n_query_images)
    # the single index itself is the reference vote (func_vpr.py:207-224 through the oracle)
    R, img, Q, off = make_problem(n_query_images)
    rng = [np.arange(off[i], off[i + 1]) for i in range(len(off) - 1)]
    ref_p, ref_s = O.get_matches_wt_borda_im(m, len(rng), sims, rng, img.astype(np.int64), n=N_TOP, return_scores=True)
    for i in range(len(rng)):
        assert pred[i, :len(ref_p[i])].tolist() == [int(x) for x in ref_p[i]]
        assert sc[i, :len(ref_s[i])].tolist() == list(ref_s[i])
    b = shard_images(n_query_images, world)
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert "error" not in z, str(z["error"])
        assert np.array_equal(z["pred"], pred)
        assert np.array_equal(z["score"].view(np.uint64), sc.view(np.uint64))      # fp64 scores, bit for bit
        assert np.array_equal(z["pred_local"], pred[b[r]:b[r + 1]])
    if n_query_images == 2:
        assert b[1] - b[0] == 0
    else:
        # the fixture matters: voting with each rank's own extrema would have given other predictions
        assert not np.array_equal(per_rank_extrema_votes(world, n_query_images), pred)


def test_a_failed_local_step_raises_on_every_rank(tmp_path):
    from revisit_anything_amd import _lib

    mp.spawn(worker, args=(2, free_port(), str(tmp_path), 7, 1), nprocs=2, join=True)
    z0, z1 = (np.load(tmp_path / f"r{r}.npz") for r in range(2))
    assert "injected local search failure" in str(z1["error"])
    assert int(z0["code"]) == _lib.SEGVLAD_ERR_COMM and "rank 1" in str(z0["error"])


def test_single_process_and_bytes():
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    R, img, Q, off = make_problem()
    pred, sc, _, _ = single_index()
    qs = QueryShardedRetrieval(QueryOracleBackend(), rank=0, world=1)
    qs.build(R, img)
    with pytest.raises(ValueError):
        qs.retrieve(torch.from_numpy(Q), off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP)      # no split yet
    out = qs.retrieve(torch.from_numpy(Q), off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True,
                      n_query_images=len(off) - 1)
    assert np.array_equal(out["pred"].numpy(), pred) and np.array_equal(out["score"].numpy().view(np.uint64), sc.view(np.uint64))
    with pytest.raises(ValueError):
        qs.retrieve(torch.from_numpy(Q), off[:3], n_query_images=len(off) - 1)                  # wrong number of images
    b = QueryShardedRetrieval.collective_bytes(8, 200, 5)
    assert b["extrema_allgather_send"] == 16 and b["extrema_allgather_recv"] == 128
    assert b["pred_allgather_send"] == 25 * 15 * 4 and b["pred_allgather_recv"] == 8 * 25 * 15 * 4
