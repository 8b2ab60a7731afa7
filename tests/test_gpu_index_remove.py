"""Removal from a LIVE index (segvlad_db_remove): the index shrinks on the device, its survivors keep their order and are renumbered
0 .. n' - 1.  The derived state the context keeps between calls (csrc/ctx.h; tests/test_gpu_index_lifecycle.py lists it) must follow:
the fp16 image of the rows and its scale, the max row norm, the bf16 hi/lo planes, db_heur_off, the shortlist's image -> row map, the
single-image pass's device words.  The check of every step: the live context gives the same (d2, idx) bits and the same plan
statistics as a FRESH context holding the survivors in one db_add, and a subset of query rows equals the emulated fp32 reference
(tests/fp32_emu.py: check_contested).

Every test owns its contexts (no module fixture: the history IS the subject)."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch

import fp32_emu as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 50
SINGLE = (1, 50, 128)     # one query image per pass (<= 128 rows: the single-image plan)
BATCH = 320               # a batch (the multi-level plan)


def _engine(**opts):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    for key, v in opts.items():
        eng.set_option(key, v)
    return eng


def _unit_rows(n, d, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=g), dim=1)


def _queries(R, m, seed, noise=0.05):
    """m noise-perturbed copies of rows of R, scaled to their source's norm."""
    g = torch.Generator(device=R.device)
    g.manual_seed(seed)
    src = torch.randint(0, R.shape[0], (m,), device=R.device, generator=g)
    base = R[src]
    nrm = base.norm(dim=1, keepdim=True)
    return (nrm * torch.nn.functional.normalize(base / nrm + noise * torch.randn(m, R.shape[1], device=R.device, generator=g), dim=1)).contiguous()


def _step_queries(R, seed):
    return [_queries(R, m, seed + j) for j, m in enumerate(SINGLE + (BATCH,))]


def _run(eng, Qs, k=K):
    return [(*eng.search(Q, k), eng.search_stats()) for Q in Qs]


def _check_against_fresh(R, Qs, got, k=K, opts=None, img=None, emulate=True):
    fresh = _engine(**(opts or {}))
    fresh.db_add(R, img)
    ref = _run(fresh, Qs, k)
    fresh.close()
    for Q, (d2, idx, st), (rd2, ridx, rst) in zip(Qs, got, ref):
        m = Q.shape[0]
        assert torch.equal(idx, ridx), (R.shape, m, int((idx != ridx).sum()))
        assert torch.equal(d2.view(torch.int32), rd2.view(torch.int32)), (R.shape, m)
        assert (st["levels"], st["filter"]) == (rst["levels"], rst["filter"]), (R.shape, m, st, rst)
        assert st["n_redo"] == 0 and st["n_fallback"] == 0, (R.shape, m, st)
        assert rst["n_redo"] == 0 and rst["n_fallback"] == 0, (R.shape, m, rst)
        if emulate:
            E.check_contested(Q, R, d2, idx, k, queries=sorted({0, m // 2, m - 1}))


def _scattered(n, n_keep, seed, dev):
    """A random keep mask with n_keep survivors (scattered removals)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[torch.randperm(n, device=dev, generator=g)[:n_keep]] = True
    return keep


def _remove_mask(eng, keep):
    """Removes the rows where keep is False (as a row-id list with a duplicate and out-of-range ids mixed in); checks the count
    and the new ids against NumPy."""
    gone = torch.nonzero(~keep).reshape(-1)
    noise = torch.tensor([-1, keep.shape[0], keep.shape[0] + 7], device=keep.device)
    ids = torch.cat([gone, gone[:1], noise]) if gone.numel() else noise
    n_removed, new_ids = eng.db_remove(row_ids=ids, want_new_ids=True)
    assert n_removed == int(gone.numel())
    want = torch.where(keep, torch.cumsum(keep.to(torch.int64), 0) - 1, torch.full_like(keep, -1, dtype=torch.int64))
    assert torch.equal(new_ids, want)
    assert eng.db_size()[0] == int(keep.sum())


# Shrinking across the single-image plan's stride and the head's grid (small_stride: the smallest power of two >= 16 that leaves
# n0 = ceil(n / stride) <= 4096 sample rows; NW = ceil(n0 / 32)):  1 M rows NW 123 -> 140 000 NW 69 -> 100 000 NW 98 -> 80 000 NW 79
# -> 20 000 (the matrix path) -> db_add back to 60 000 (the filter plan again).  d = 96: the path without the fused head.
@pytest.mark.parametrize("d", [1024, 96])
def test_shrink_across_plan_changes(d):
    dev = torch.device("cuda:0")
    R = _unit_rows(1_000_000, d, 9000 + d, dev)
    live = _engine()
    live.db_add(R)
    _check_against_fresh(R, _step_queries(R, 10 + d), _run(live, _step_queries(R, 10 + d)))
    for s, n in enumerate((140_000, 100_000, 80_000, 20_000)):
        keep = _scattered(R.shape[0], n, 9100 + s, dev)
        _remove_mask(live, keep)
        R = R[keep].contiguous()
        Qs = _step_queries(R, 100 * s + d)
        got = _run(live, Qs)
        if n <= 32768:
            assert all(st["filter"] == "none" for _, _, st in got), [st for _, _, st in got]
        _check_against_fresh(R, Qs, got)
    R2 = _unit_rows(40_000, d, 9200 + d, dev)
    live.db_add(R2)
    R = torch.cat([R, R2])
    Qs = _step_queries(R, 900 + d)
    _check_against_fresh(R, Qs, _run(live, Qs))
    live.close()


def test_fp16_scale_history():
    """Removing the x4-magnitude rows that set the fp16 image's scale (the scale is kept: it still bounds every survivor), and
    removing rows added under an OLDER scale (1e-3 rows quantised under the unit rows' scale) together with unit rows."""
    dev = torch.device("cuda:0")
    d = 256
    R0 = _unit_rows(60_000, d, 40, dev)
    for case in ("larger", "smaller"):
        live = _engine()
        live.db_add(R0)
        live.search(_queries(R0, 50, 41), K)
        Rh = 4.0 * _unit_rows(20_000, d, 42, dev) if case == "larger" else 1e-3 * _unit_rows(1_000, d, 43, dev)
        live.db_add(Rh)
        R1 = torch.cat([R0, Rh])
        live.search(_queries(R1, 50, 44), K)         # (the fp16 image covers every row: rescaled for "larger")
        keep = torch.ones(R1.shape[0], dtype=torch.bool, device=dev)
        if case == "larger":
            keep[R0.shape[0]:] = False               # every row that set the scale
        else:
            keep[R0.shape[0] + 1::2] = False         # half of the rows quantised under the older scale
            keep[:R0.shape[0]:3] = False             # and a third of the unit rows
        _remove_mask(live, keep)
        R = R1[keep].contiguous()
        Qs = _step_queries(R, 520)
        _check_against_fresh(R, Qs, _run(live, Qs))
        live.close()


@pytest.mark.parametrize("filt", ["f16", "bf16x3", "fp32"])
def test_partial_planes(filt):
    """Add, search, add again with no search in between (the 16-bit planes cover a prefix), then remove rows from both parts; and
    a removal before any search has built a plane."""
    dev = torch.device("cuda:0")
    d = 256
    A, B = _unit_rows(60_000, d, 60, dev), _unit_rows(30_000, d, 61, dev)
    live = _engine(knn_filter=filt)
    live.db_add(A)
    live.search(_queries(A, 320, 62), K)
    live.db_add(B)
    R = torch.cat([A, B])
    keep = _scattered(R.shape[0], 70_000, 63, dev)
    _remove_mask(live, keep)
    R = R[keep].contiguous()
    Qs = _step_queries(R, 640)
    got = _run(live, Qs)
    assert all(st["filter"] == filt for _, _, st in got), [st for _, _, st in got]
    _check_against_fresh(R, Qs, got, opts={"knn_filter": filt})
    live.close()
    fresh_live = _engine(knn_filter=filt)           # removal before any plane exists
    fresh_live.db_add(A)
    keep = _scattered(A.shape[0], 45_000, 64, dev)
    _remove_mask(fresh_live, keep)
    R = A[keep].contiguous()
    Qs = _step_queries(R, 650)
    _check_against_fresh(R, Qs, _run(fresh_live, Qs), opts={"knn_filter": filt}, emulate=False)
    fresh_live.close()


def test_remove_images():
    from revisit_anything_amd import _lib
    from revisit_anything_amd._lib import SegVLADError

    dev = torch.device("cuda:0")
    d, per, n = 256, 50, 100_000
    R = _unit_rows(n, d, 90, dev)
    img = torch.arange(n, device=dev, dtype=torch.int32) // per
    n_img = n // per
    live = _engine()
    live.db_add(R, img)
    live.search(_queries(R, 50, 91), K)
    gone_imgs = [n_img - 1, 5, 5, 17, 1000, n_img + 30, -1, -7]
    from revisit_anything_amd.pipeline import SegVLADPipeline

    assert SegVLADPipeline(live, 224, 224).index_remove_images(np.array(gone_imgs, np.int32)) == 4 * per
    assert live.n_img_ref == n_img                   # (a shortlist may still name a removed image)
    keep = ~torch.isin(img, torch.tensor([n_img - 1, 5, 17, 1000], device=dev, dtype=torch.int32))
    Rs, imgs = R[keep].contiguous(), img[keep].contiguous()
    Qs = _step_queries(Rs, 910)
    _check_against_fresh(Rs, Qs, _run(live, Qs), img=imgs)
    fresh = _engine()
    fresh.db_add(Rs, imgs)
    for m_img, seed in ((1, 920), (7, 930)):
        Q = _queries(Rs, m_img * per, seed)
        qoff = np.arange(0, m_img * per + 1, per, dtype=np.int32)
        every = np.tile(np.arange(n_img, dtype=np.int32), (m_img, 1))
        sd2, sidx = live.search_shortlist(Q, qoff, every, K)
        d2, idx = live.search(Q, K)
        assert torch.equal(sidx, idx) and torch.equal(sd2.view(torch.int32), d2.view(torch.int32))
        only_removed = np.tile(np.array([5, 17, n_img - 1], np.int32), (m_img, 1))
        od2, oidx = live.search_shortlist(Q, qoff, only_removed, K)
        assert bool((oidx == -1).all()) and bool(torch.isinf(od2).all())
        sims, m = live.sims_from_d2(d2, idx, K)
        pred, sc = live.vote(m, sims, qoff, n_top=5, want_scores=True)
        rd2, ridx = fresh.search(Q, K)
        rs, rm = fresh.sims_from_d2(rd2, ridx, K)
        rpred, rsc = fresh.vote(rm, rs, qoff, n_top=5, want_scores=True)
        assert torch.equal(pred, rpred) and torch.equal(sc, rsc)
    fresh.close()
    live.close()
    plain = _engine()
    plain.db_add(R[:40_000])
    with pytest.raises(SegVLADError) as ei:
        plain.db_remove(img_ids=[1])
    assert ei.value.code == _lib.SEGVLAD_ERR_STATE
    assert plain.db_size()[0] == 40_000
    plain.close()


def test_remove_everything():
    from revisit_anything_amd._lib import SegVLADError

    dev = torch.device("cuda:0")
    d, per = 256, 50
    R = _unit_rows(60_000, d, 100, dev)
    img = torch.arange(60_000, device=dev, dtype=torch.int32) // per
    live = _engine()
    live.db_add(R, img)
    live.search(_queries(R, 320, 101), K)
    assert live.db_remove(img_ids=torch.arange(60_000 // per, device=dev)) == 60_000
    assert live.db_size() == (0, d)
    Q = _queries(R, 50, 102)
    for m in (1, 50, 320):
        d2, idx = live.search(_queries(R, m, 103), K)
        assert bool((idx == -1).all()) and bool(torch.isinf(d2).all())
    d2, idx = live.search_shortlist(Q, np.array([0, 50], np.int32), [[0, 1, 2]], K)
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all())
    assert live.db_remove(row_ids=[0, 1]) == 0
    with pytest.raises(SegVLADError):
        live.db_add(_unit_rows(10, 128, 104, dev), torch.zeros(10, dtype=torch.int32, device=dev))    # another d
    with pytest.raises(SegVLADError):
        live.db_add(_unit_rows(10, d, 105, dev))                                                       # no image map
    R2 = _unit_rows(50_000, d, 106, dev)
    img2 = torch.arange(50_000, device=dev, dtype=torch.int32) // per
    live.db_add(R2, img2)
    Qs = _step_queries(R2, 1070)
    _check_against_fresh(R2, Qs, _run(live, Qs), img=img2)
    live.close()


def test_new_ids_host_and_device_and_index_flat_l2():
    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import _ptr
    from revisit_anything_amd.place_rec import IndexFlatL2

    dev = torch.device("cuda:0")
    d, n = 128, 40_000
    R = _unit_rows(n, d, 110, dev)
    rng = np.random.default_rng(111)
    gone = rng.choice(n, 3_000, replace=False).astype(np.int64)
    keep = np.ones(n, bool)
    keep[gone] = False
    want = np.where(keep, np.cumsum(keep) - 1, -1)
    for host_out in (True, False):
        eng = _engine()
        eng.db_add(R)
        out = np.full(n, -5, np.int64) if host_out else torch.full((n,), -5, dtype=torch.int64, device=dev)
        nrm = C.c_int64(-1)
        eng._stream()
        rc = eng.lib.segvlad_db_remove(eng._h, _ptr(gone), len(gone), None, 0, _ptr(out), C.byref(nrm))
        assert rc == _lib.SEGVLAD_OK, eng.lib.segvlad_last_error(eng._h)
        got = out if host_out else out.cpu().numpy()
        assert np.array_equal(got, want) and nrm.value == len(gone)
        eng.close()
    index = IndexFlatL2(d)
    index.add(R.cpu().numpy())
    assert index.remove_ids(np.concatenate([gone, gone[:5], [-1, n]])) == len(gone)
    assert index.ntotal == n - len(gone)
    Rs = R.cpu().numpy()[keep]
    q = Rs[[0, 100, 20_000, len(Rs) - 1]]
    d2, idx = index.search(q, 5)
    assert idx[:, 0].tolist() == [0, 100, 20_000, len(Rs) - 1] and np.all(d2[:, 0] < 1e-5)
    with pytest.raises(TypeError):
        index.remove_ids(np.array([1.0]))


@pytest.mark.parametrize("on_side_stream", [False, True])
def test_interleaved_searches_across_a_removal(on_side_stream):
    """Single-image and batch searches enqueued back to back on either side of a removal that changes the head's grid
    (100 000 -> 80 000 rows: NW 98 -> 79), with no synchronisation between the searches."""
    dev = torch.device("cuda:0")
    d = 1024
    R = _unit_rows(100_000, d, 120, dev)
    keep = _scattered(100_000, 80_000, 121, dev)
    Rs = R[keep].contiguous()
    Qa = [_queries(R, m, 122 + j) for j, m in enumerate((50, BATCH, 1, 50))]
    Qb = [_queries(Rs, m, 132 + j) for j, m in enumerate((50, BATCH, 50, 1))]
    gone = torch.nonzero(~keep).reshape(-1)
    live = _engine()
    stream = torch.cuda.Stream(dev) if on_side_stream else torch.cuda.current_stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        live.db_add(R)
        out_a = [live.search(Q, K) for Q in Qa]
        live.db_remove(row_ids=gone)
        out_b = [live.search(Q, K) for Q in Qb]
        out_c = [live.search(Q, K) for Q in Qb]
    stream.synchronize()
    torch.cuda.synchronize()
    st = live.search_stats()
    assert st["n_redo"] == 0 and st["n_fallback"] == 0 and st["levels"] == 1, st
    live.close()
    for rows, Qs, outs in ((R, Qa, [out_a]), (Rs, Qb, [out_b, out_c])):
        fresh = _engine()
        fresh.db_add(rows)
        for Q, o in zip(Qs, zip(*outs)):
            rd2, ridx = fresh.search(Q, K)
            for d2, idx in o:
                assert torch.equal(idx, ridx) and torch.equal(d2.view(torch.int32), rd2.view(torch.int32)), (rows.shape, Q.shape)
        fresh.close()


def test_64_bit_offsets():
    """d = 98 304 (raw K*D descriptors) x 40 000 rows: 3.9 G elements (15.7 GB) of fp32 rows and, built by a search before the
    removal, the fp16 image of every row (7.9 GB) -- element offsets past 2^31 and byte offsets past 2^32 in both gathers.  (Their
    16-byte unit index stays below 2^31: that would take planes of more than 32 GiB.)  Rows near the start are removed; each of the
    last surviving rows, queried as itself, comes back as its new id at distance ~0."""
    dev = torch.device("cuda:0")
    d, n, chunk, m = 98_304, 40_000, 4_000, 130
    live = _engine()
    g = torch.Generator(device=dev)
    g.manual_seed(140)
    for c0 in range(0, n, chunk):                       # (built in slices: one 15.7 GB tensor less in flight)
        live.db_add(torch.randn(chunk, d, device=dev, generator=g))
    tail = torch.Generator(device=dev)
    tail.manual_seed(140)
    for _ in range(n // chunk - 1):
        torch.randn(chunk, d, device=dev, generator=tail)
    last = torch.randn(chunk, d, device=dev, generator=tail)[-m:].contiguous()   # rows n-m .. n-1 (a batch: > 128 query rows)
    d2, idx = live.search(last, K)
    assert live.search_stats()["filter"] == "f16"      # (the fp16 image of every row exists now)
    assert idx[:, 0].tolist() == list(range(n - m, n)), idx[:, 0].tolist()
    gone = torch.tensor([0, 1, 2, 7, 100, 3_000], device=dev)
    assert live.db_remove(row_ids=gone) == 6
    assert live.db_size() == (n - 6, d)
    d2, idx = live.search(last, K)
    assert live.search_stats()["filter"] == "f16"
    assert idx[:, 0].tolist() == list(range(n - m - 6, n - 6)), idx[:, 0].tolist()
    # (0 up to the fp32 rounding of a 98 304-term dot product against the stored norm, ~5e-5 of ||r||^2; any other row is ~2 d away)
    assert bool((d2[:, 0] <= 2e-4 * last.pow(2).sum(1)).all()) and bool((d2[:, 1] > d).all()), d2
    live.close()


@pytest.mark.parametrize("d", [97, 98])
def test_row_pitch_not_a_multiple_of_16_bytes(d):
    """Odd d (4-byte accesses) and d % 4 == 2 (8-byte accesses, rows shorter than a wave's worth of units): scattered removals across
    the fp32 filter plan (> 32 768 rows) and into the matrix path, against a fresh context."""
    dev = torch.device("cuda:0")
    R = _unit_rows(40_000, d, 160 + d, dev)
    live = _engine()
    live.db_add(R)
    live.search(_queries(R, 50, 161), K)
    for s, n in enumerate((36_000, 20_000)):
        keep = _scattered(R.shape[0], n, 170 + s, dev)
        _remove_mask(live, keep)
        R = R[keep].contiguous()
        Qs = _step_queries(R, 180 + 10 * s)
        got = _run(live, Qs)
        assert all(st["filter"] == ("fp32" if n > 32768 else "none") for _, _, st in got), [st for _, _, st in got]
        _check_against_fresh(R, Qs, got, emulate=False)
    live.close()


def _sharded_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import ShardedSegmentIndex, shard_bounds

    R, img, Q, off = _sharded_problem()
    eng = SegVLADEngine(0)
    rb = shard_bounds(R.shape[0], world)
    idx = ShardedSegmentIndex(eng, device=eng.device)
    idx.build(torch.from_numpy(R[rb[rank]:rb[rank + 1]]).to(eng.device), img[rb[rank]:rb[rank + 1]])
    n1 = idx.remove(**_SHARD_STEPS[0])
    n2 = idx.remove(**_SHARD_STEPS[1])
    pred, sc, m, sims = idx.retrieve(torch.from_numpy(Q).to(eng.device), off, k_search=60, k_vote=50, n_top=5, want_scores=True)
    d2, ids = idx.search(torch.from_numpy(Q).to(eng.device), 60)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), d2=d2.cpu().numpy(), ids=ids.cpu().numpy(), pred=pred.cpu().numpy(),
             sc=sc.cpu().numpy(), n=np.array([n1, n2]))
    dist.barrier()
    dist.destroy_process_group()


def _sharded_problem():
    from revisit_anything_amd import synth

    R, img = synth.make_planted_db(900, 40, 64, seed=3300)
    Q, tau, off = synth.make_planted_queries(R, 900, 40, 12, seed=4300, sigma_q=2.0)
    return R, img, Q, off


_SHARD_STEPS = [{"row_ids": list(range(0, 36_000, 7)) + [-1, 10 ** 6], "img_ids": None},
                {"row_ids": None, "img_ids": [899, 3, 450, 451, 5000]}]


def _survivors(R, img):
    keep = np.ones(R.shape[0], bool)
    keep[np.arange(0, 36_000, 7)] = False
    R, img = R[keep], img[keep]
    keep = ~np.isin(img, [899, 3, 450, 451])
    return R[keep], img[keep]


def _single_index_reference(Rs, imgs, Q, off):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    dev = eng.device
    eng.db_add(torch.from_numpy(Rs).to(dev), torch.from_numpy(imgs.astype(np.int32)).to(dev))
    d2, ids = eng.search(torch.from_numpy(Q).to(dev), 60)
    sims, m = eng.sims_from_d2(d2, ids, 50)
    pred, sc = eng.vote(m, sims, off, n_top=5, want_scores=True)
    out = (d2[:, :50].cpu().numpy(), ids[:, :50].cpu().numpy(), pred.cpu().numpy(), sc.cpu().numpy())
    eng.close()
    return out


def test_row_sharded_world_2_and_query_sharded_world_1(tmp_path):
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    R, img, Q, off = _sharded_problem()
    Rs, imgs = _survivors(R, img)
    rd2, rids, rpred, rsc = _single_index_reference(Rs, imgs, Q, off)
    n_first = len(range(0, 36_000, 7))
    for r in range(2):
        z = np.load(tmp_path / f"r{r}.npz")
        assert z["n"][0] == n_first and z["n"][1] == 36_000 - n_first - Rs.shape[0]
        assert np.array_equal(z["ids"][:, :50], rids) and np.array_equal(z["d2"][:, :50], rd2)
        assert np.array_equal(z["pred"], rpred) and np.array_equal(z["sc"], rsc)
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.sharded import QueryShardedRetrieval

    for native in (False, True):
        eng = SegVLADEngine(0)
        qs = QueryShardedRetrieval(eng, rank=0, world=1, device=eng.device, native_comm=native)
        qs.build(torch.from_numpy(R).to(eng.device), img)
        assert qs.remove(**_SHARD_STEPS[0]) == n_first
        qs.remove(**_SHARD_STEPS[1])
        out = qs.retrieve(torch.from_numpy(Q).to(eng.device), off, k_search=60, k_vote=50, n_top=5, want_scores=True,
                          n_query_images=len(off) - 1)
        assert np.array_equal(out["pred"].cpu().numpy(), rpred) and np.array_equal(out["score"].cpu().numpy(), rsc), native
        assert np.array_equal(out["m"].cpu().numpy(), rids)
        eng.close()
