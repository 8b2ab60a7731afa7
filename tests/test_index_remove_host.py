"""Removal from the index, the parts that need no GPU: the C-ABI entry exists and is bound, and the row-sharded index's collective
remove (sharded.ShardedSegmentIndex.remove) over gloo processes with a NumPy backend whose db_remove follows faiss's remove_ids
(survivors keep their order, every later id moves down).  Invariant: after removals, sharded search, global ids and votes equal
one NumPy index over the survivors; a rank given other lists makes every rank raise with no shard changed."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMG, S, D = 61, 7, 32          # 427 rows: not divisible by the world size


class RemovingOracleBackend:
    """SegVLADEngine-shaped test double (NumPy oracle inside), with db_remove."""

    def __init__(self):
        from oracle import segvlad_oracle as O

        self.O = O
        self.device = torch.device("cpu")
        self.R = np.zeros((0, D), np.float32)
        self.removed_calls = []

    def db_reset(self):
        self.R = np.zeros((0, D), np.float32)

    def db_add(self, R, img):
        self.R = np.concatenate([self.R, np.asarray(R, dtype=np.float32)])

    def db_remove(self, row_ids=None, img_ids=None, want_new_ids=False):
        assert img_ids is None, "the row-sharded build holds no image map: image removal must arrive as row removal"
        ids = np.asarray(row_ids, dtype=np.int64).reshape(-1)
        n = self.R.shape[0]
        keep = np.ones(n, bool)
        keep[ids[(ids >= 0) & (ids < n)]] = False
        self.removed_calls.append(ids.copy())
        self.R = self.R[keep]
        return int((~keep).sum())

    def search(self, Q, k):
        d2, idx = self.O.knn_l2(self.R, np.asarray(Q, dtype=np.float32), k)
        return torch.from_numpy(d2), torch.from_numpy(idx)

    def merge_topk(self, d2c, idc, parts, k):
        d2c, idc = d2c.numpy(), idc.numpy()
        dp = [d2c[:, p * k:(p + 1) * k] for p in range(parts)]
        ip = [idc[:, p * k:(p + 1) * k] for p in range(parts)]
        d, i = self.O.merge_topk(dp, ip, k)
        return torch.from_numpy(d), torch.from_numpy(i)

    def sims_from_d2(self, d2, idx, k_keep):
        return (2 - d2[:, :k_keep]).to(torch.float32), idx[:, :k_keep]

    def vote(self, m, sims, qoff, n_top=5, mode=0, img_of_seg=None, want_scores=False, **kw):
        rng = [np.arange(qoff[i], qoff[i + 1]) for i in range(len(qoff) - 1)]
        p, sc = self.O.get_matches_wt_borda_im(m.numpy(), len(rng), sims.numpy(), rng, img_of_seg.numpy().astype(np.int64),
                                               n=n_top, return_scores=True)
        out = np.full((len(rng), n_top), -1, np.int32)
        for i, row in enumerate(p):
            out[i, :len(row)] = row
        return torch.from_numpy(out), sc


def make_problem():
    from revisit_anything_amd import synth

    R, img = synth.make_planted_db(N_IMG, S, D, seed=3100)
    Q, tau, off = synth.make_planted_queries(R, N_IMG, S, 9, seed=4100, sigma_q=2.0)
    return R, img, Q, off


# Two removal steps: scattered rows (global ids; out-of-range, negative and duplicate ids among them) and whole images
# (the largest id, an id no row carries, duplicates, a negative one), then rows of the now-shifted numbering.
STEPS = [
    {"row_ids": [0, 5, 5, 97, 212, 213, 426, 426, 1000, -3], "img_ids": None},
    {"row_ids": None, "img_ids": [N_IMG - 1, 3, 3, 17, 500, -1]},
    {"row_ids": list(range(40, 60)) + [350], "img_ids": [20]},
]


def numpy_after(R, img, steps):
    """The survivors' rows and image map after `steps`, applied one after the other with faiss's renumbering."""
    for st in steps:
        n = R.shape[0]
        keep = np.ones(n, bool)
        if st["row_ids"] is not None:
            r = np.asarray(st["row_ids"], np.int64)
            keep[r[(r >= 0) & (r < n)]] = False
        if st["img_ids"] is not None:
            keep &= ~np.isin(img, [g for g in st["img_ids"] if g >= 0])
        R, img = R[keep], img[keep]
    return R, img


def reference_results(R, img, Q, off):
    from oracle import segvlad_oracle as O

    d2, ids = O.knn_l2(R, Q, 20)
    sims = (2 - d2[:, :10]).astype(np.float32)
    rng = [np.arange(off[i], off[i + 1]) for i in range(len(off) - 1)]
    preds = O.get_matches_wt_borda_im(ids[:, :10], len(rng), sims, rng, img.astype(np.int64), n=3)
    return d2, ids, preds


def worker(rank, world, port, out_dir, mismatch):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from revisit_anything_amd.sharded import ShardedSegmentIndex, shard_bounds

    R, img, Q, off = make_problem()
    rb = shard_bounds(R.shape[0], world)
    be = RemovingOracleBackend()
    idx = ShardedSegmentIndex(be)
    idx.build(R[rb[rank]:rb[rank + 1]], img[rb[rank]:rb[rank + 1]])
    if mismatch:
        # rank 1 removes one row more than the others: every rank must raise, no shard may change
        rows = [3, 9] + ([11] if rank == 1 else [])
        raised = False
        try:
            idx.remove(row_ids=rows)
        except RuntimeError:
            raised = True
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), raised=raised, n=be.R.shape[0], calls=len(be.removed_calls),
                 row_start=idx.row_start, n_img=idx.img_of_seg_global.shape[0])
    else:
        counts = []
        for st in STEPS:
            counts.append(idx.remove(**st))
            d2, ids = idx.search(torch.from_numpy(Q), 20)
            pred, sc, m, sims = idx.retrieve(torch.from_numpy(Q), off, k_search=20, k_vote=10, n_top=3, want_scores=True)
            assert int(idx.row_start[-1]) == idx.img_of_seg_global.shape[0]
            assert be.R.shape[0] == int(idx.row_start[rank + 1] - idx.row_start[rank])
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), d2=d2.numpy(), ids=ids.numpy(), pred=pred.numpy(), counts=np.array(counts),
                 img=idx.img_of_seg_global.numpy(), row_start=idx.row_start)
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_the_library_exports_and_binds_db_remove():
    from revisit_anything_amd import _lib

    assert "segvlad_db_remove" in _lib.SIGNATURES
    lib = _lib.load(build_if_missing=False)
    fn = lib.segvlad_db_remove
    n_removed = C.c_int64(7)
    assert fn(None, None, 0, None, 0, None, C.byref(n_removed)) == _lib.SEGVLAD_ERR_ARG
    with open(os.path.join(ROOT, "include", "segvlad.h")) as f:
        assert "int segvlad_db_remove(" in f.read()


@pytest.mark.parametrize("world", [2, 3])
def test_row_sharded_remove_equals_one_index_over_the_survivors(tmp_path, world):
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), False), nprocs=world, join=True)
    R, img, Q, off = make_problem()
    counts = []
    for j in range(len(STEPS)):
        before = numpy_after(R, img, STEPS[:j])[0].shape[0]
        counts.append(before - numpy_after(R, img, STEPS[:j + 1])[0].shape[0])
    Rs, imgs = numpy_after(R, img, STEPS)
    assert Rs.shape[0] < R.shape[0] - 50
    d2, ids, preds = reference_results(Rs, imgs, Q, off)
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert z["counts"].tolist() == counts
        assert np.array_equal(z["img"], imgs)
        assert int(z["row_start"][-1]) == Rs.shape[0]
        assert np.array_equal(z["ids"], ids)        # global ids of the survivors, bit for bit
        assert np.array_equal(z["d2"], d2)
        for i, p in enumerate(preds):
            assert z["pred"][i][:len(p)].tolist() == [int(x) for x in p]


def test_a_rank_given_other_lists_makes_every_rank_raise(tmp_path):
    world = 3
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), True), nprocs=world, join=True)
    from revisit_anything_amd.sharded import shard_bounds

    rb = shard_bounds(N_IMG * S, world)
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert bool(z["raised"]), r
        assert int(z["calls"]) == 0 and int(z["n"]) == int(rb[r + 1] - rb[r]), r
        assert np.array_equal(z["row_start"], rb) and int(z["n_img"]) == N_IMG * S


def test_single_process_remove_and_the_keep_mask_rule():
    from revisit_anything_amd.sharded import ShardedSegmentIndex, removal_keep_mask

    R, img, Q, off = make_problem()
    im = torch.from_numpy(img.astype(np.int32))
    keep = removal_keep_mask(im, row_ids=[1, 1, -1, 10 ** 6], img_ids=[0, -5, 10 ** 6, N_IMG - 1])
    want = ~np.isin(img, [0, N_IMG - 1])
    want[1] = False
    assert np.array_equal(keep.numpy(), want)
    idx = ShardedSegmentIndex(RemovingOracleBackend(), rank=0, world=1)
    idx.build(R, img)
    assert idx.remove(**STEPS[0]) == 6
    assert idx.remove() == 0
    Rs, imgs = numpy_after(R, img, STEPS[:1])
    d2, ids, preds = reference_results(Rs, imgs, Q, off)
    got_d2, got_ids = idx.search(torch.from_numpy(Q), 20)
    assert np.array_equal(got_ids.numpy(), ids) and np.array_equal(got_d2.numpy(), d2)
    assert idx.n_total == Rs.shape[0] and np.array_equal(idx.img_of_seg_global.numpy(), imgs)
