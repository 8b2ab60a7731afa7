"""The vote's one-to-one flag through the two sharded classes, on CPU: 2 gloo processes and a checker backend whose vote applies
tests/vote_unique_ref.py's blank_unique() for bit 0x80 of `mode`, the cap's blank() for bits 8..15 behind it, and then runs the plain
references of tests/search_tail_ref.py.

ShardedSegmentIndex.retrieve(vote_unique_ref=True) must equal a single index's: the merged lists carry global row ids, so the
claims on one reference segment meet whatever rank held it.  QueryShardedRetrieval.retrieve(vote_unique_ref=True) must still exchange
the weighted mode's extrema: the base is `mode & 0x7f` now, and a test on `mode & 0xff == 0` would skip the exchange."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import search_tail_ref as R  # noqa: E402
import vote_cap_ref as V  # noqa: E402
import vote_unique_ref as U  # noqa: E402
from tests.test_query_shard_gloo import free_port, local_slice, make_problem  # noqa: E402
from tests.test_sharded_gloo import OracleBackend  # noqa: E402

K_SEARCH, K_VOTE, N_TOP = 20, 10, 3
N_QUERY_IMAGES = 7
FLAG = 0x80


class UniqueBackend(OracleBackend):
    """OracleBackend with SegVLADEngine.vote's mode word: base in bits 0..6, the one-to-one flag in bit 7, the cap in bits 8..15."""

    def minmax(self, sims):
        s = np.asarray(sims, dtype=np.float32)
        return torch.tensor([s.min(), s.max()], dtype=torch.float32)

    def vote(self, m, sims, qoff, n_top=5, mode=0, img_of_seg=None, want_scores=False, smin=float("nan"), smax=float("nan"), **kw):
        assert not kw, kw                                    # flag and cap travel in `mode`
        base, cap = mode & 0x7F, (mode >> 8) & 0xFF
        assert mode >> 16 == 0 and base in (0, 1)
        m, img = np.asarray(m), np.asarray(img_of_seg)
        off = np.asarray(qoff)
        s32 = None if sims is None else np.asarray(sims, np.float32)
        self.last_vote = dict(mode=mode, smin=float(smin), smax=float(smax))
        if mode & FLAG:
            m = U.blank_unique(m, s32, off, len(img))
        if cap:
            m = V.blank(m, img, cap)
        if base == 1:
            pred, sc = R.vote_count(m, off, img, n_top)
        else:
            pred, sc = R.vote_wt(m, s32, off, img, n_top, None if np.isnan(smin) else smin, None if np.isnan(smax) else smax)
        return torch.from_numpy(pred), torch.from_numpy(sc)


def single_index(**kw):
    from revisit_anything_amd.sharded import ShardedSegmentIndex

    Rr, img, Q, off = make_problem(N_QUERY_IMAGES)
    idx = ShardedSegmentIndex(UniqueBackend(), rank=0, world=1)
    idx.build(Rr, img)
    pred, sc, m, sims = idx.retrieve(Q, off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, want_scores=True, **kw)
    return pred.numpy(), sc.numpy(), np.asarray(m), np.asarray(sims), idx.be.last_vote


def worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from revisit_anything_amd.sharded import QueryShardedRetrieval, ShardedSegmentIndex, shard_images

    Rr, img, Q, off = make_problem(N_QUERY_IMAGES)
    res = {}
    # rows sharded: every rank holds a block of the reference images and all the queries
    ib = shard_images(61, world)
    rows = slice(ib[rank] * 7, ib[rank + 1] * 7)
    idx = ShardedSegmentIndex(UniqueBackend())
    idx.build(Rr[rows], img[rows])
    for mode in (0, 1):
        for cap in (None, 1):
            pred, sc, m, sims = idx.retrieve(torch.from_numpy(Q), off, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, mode=mode,
                                             want_scores=True, vote_unique_ref=True, votes_per_image=cap)
            res[f"rows_pred{mode}{cap}"], res[f"rows_score{mode}{cap}"] = pred.numpy(), sc.numpy()
            assert idx.be.last_vote["mode"] == mode | FLAG | ((cap or 0) << 8)
    # queries sharded: every rank holds the whole index and a block of the query images
    qs = QueryShardedRetrieval(UniqueBackend())
    qs.build(Rr, img)
    b = qs.split(len(off) - 1)
    q_local, off_local = local_slice(Q, off, b, rank)
    for mode in (0, 1):
        for cap in (None, 1):
            out = qs.retrieve(torch.from_numpy(q_local), off_local, k_search=K_SEARCH, k_vote=K_VOTE, n_top=N_TOP, mode=mode,
                              want_scores=True, vote_unique_ref=True, votes_per_image=cap)
            res[f"query_pred{mode}{cap}"], res[f"query_score{mode}{cap}"] = out["pred"].numpy(), out["score"].numpy()
            res[f"query_smin{mode}{cap}"], res[f"query_smax{mode}{cap}"] = qs.be.last_vote["smin"], qs.be.last_vote["smax"]
            assert qs.be.last_vote["mode"] == mode | FLAG | ((cap or 0) << 8)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_index(tmp_path):
    world = 2
    mp.spawn(worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    Rr, img, Q, off = make_problem(N_QUERY_IMAGES)
    plain = single_index()
    want = {(mode, cap): single_index(mode=mode, vote_unique_ref=True, votes_per_image=cap) for mode in (0, 1) for cap in (None, 1)}
    m, sims = plain[2], plain[3]
    # the flag bites on these lists and changes the weighted scores
    b = U.blank_unique(m, sims, off, len(img))
    assert (b != m).sum() >= len(off) - 1
    assert not np.array_equal(want[0, None][1].view(np.uint64), plain[1].view(np.uint64))
    # the single index's flagged result is the plain vote over the blanked lists, the cap behind the flag
    wp, ws = R.vote_wt(b, sims, off, img, N_TOP)
    assert np.array_equal(want[0, None][0], wp) and np.array_equal(want[0, None][1].view(np.uint64), ws.view(np.uint64))
    wp, ws = R.vote_wt(V.blank(b, img, 1), sims, off, img, N_TOP)
    assert np.array_equal(want[0, 1][0], wp) and np.array_equal(want[0, 1][1].view(np.uint64), ws.view(np.uint64))
    # every rank normalising with its own extrema would score differently: the exchange matters on this input
    from revisit_anything_amd.sharded import shard_images

    bounds = shard_images(len(off) - 1, world)
    lo = int(off[bounds[1]])
    assert (sims[:lo].min(), sims[:lo].max()) != (sims[lo:].min(), sims[lo:].max())
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        for (mode, cap), (pred, sc, *_) in want.items():
            for kind in ("rows", "query"):
                assert np.array_equal(z[f"{kind}_pred{mode}{cap}"], pred), (r, mode, cap, kind)
                assert np.array_equal(z[f"{kind}_score{mode}{cap}"].view(np.uint64), sc.view(np.uint64)), (r, mode, cap, kind)
            # the weighted mode voted with the global extrema of ALL kept similarities, the count mode needs none
            if mode == 0:
                assert np.float32(z[f"query_smin0{cap}"]) == sims.min() and np.float32(z[f"query_smax0{cap}"]) == sims.max()
            else:
                assert np.isnan(z[f"query_smin1{cap}"]) and np.isnan(z[f"query_smax1{cap}"])


def test_single_process_keyword_and_mode_bits_agree():
    a = single_index(vote_unique_ref=True, votes_per_image=2)
    b = single_index(mode=FLAG | (2 << 8))
    assert a[4]["mode"] == b[4]["mode"] == 0x280
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
