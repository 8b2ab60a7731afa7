"""ONE rank of a W-way QUERY-sharded run (sharded.QueryShardedRetrieval), emulated on one MI355X.

Every rank of that form holds the WHOLE index (replicated) and handles nQ / W of the query images: it describes them, searches
their segments k_vote deep against the full index and votes on them.  Per step and per W this tool times exactly that at the
bench geometry (default: 200 query images of 50 segments, 20000 reference images = 1 M rows of 1024 PCA dims): describe of
nQ / W images, their search against all rows, sims, the local min / max and the vote.

The collectives are NOT executed.  The exchange of the vote's extrema (16 bytes per rank) is replaced by a LOCAL stand-in --
segvlad_vote_global on a context without a communicator, i.e. the vote with this rank's own extrema: the same kernels, minus
the all-gather and the one-wave reduction of W records -- and the gather of the predictions is not run either; both are
reported by their byte counts.  One JSON line:
{"per_rank": {W: {"per_rank_ms", "stages_ms", "implied_images_per_s", ...}}, "collective_stand_in": ..., ...}
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import QUERY_OWN_DEFAULT, ImageFactory  # noqa: E402
from revisit_anything_amd import synth  # noqa: E402
from revisit_anything_amd.engine import SegVLADEngine  # noqa: E402
from revisit_anything_amd.pipeline import SegVLADPipeline  # noqa: E402
from revisit_anything_amd.sharded import QueryShardedRetrieval, shard_images  # noqa: E402

STAGES = ("incidence", "adjacency", "assign", "prep", "aggregate", "pca", "describe", "knn_level0", "knn_gemm", "knn_select", "vote")


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--worlds", default="2,4,8")
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--query-images", type=int, default=200)
    p.add_argument("--db-images", type=int, default=20000)
    p.add_argument("--segments", type=int, default=50)
    p.add_argument("--clusters", type=int, default=64)
    p.add_argument("--dim", type=int, default=1536)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--pca-dim", type=int, default=1024)
    p.add_argument("--order", type=int, default=3)
    p.add_argument("--build-batch", type=int, default=100)
    p.add_argument("--group", type=int, default=4)
    p.add_argument("--k-vote", type=int, default=50)
    p.add_argument("--n-top", type=int, default=5)
    return p.parse_args(argv)


def run(a) -> dict:
    S, K, D, H, W_, P = a.segments, a.clusters, a.dim, a.height, a.width, a.pca_dim
    N, Hm, Wm = (H // 14) * (W_ // 14), H // 2, W_ // 2
    nQ, nR, kv = a.query_images, a.db_images, a.k_vote
    dev = torch.device("cuda:0")
    eng = SegVLADEngine(0)
    C_np = synth.make_vocab(K, D, seed=1000)
    eng.set_vocab(C_np)
    g = torch.Generator(device=dev)
    g.manual_seed(5000)
    comps = torch.randn(P, K * D, device=dev, generator=g) / (K * D) ** 0.5
    mean = torch.randn(K * D, device=dev, generator=g) * (0.2 / (K * D) ** 0.5)
    eng.pca_set(mean, comps, torch.logspace(-3, -6, P, device=dev), whiten=True)
    del comps
    eng.set_option("pca_path", "project")
    pipe = SegVLADPipeline(eng, H, W_, 14, order=a.order, use_pca=True)
    fac = ImageFactory(dev, torch.from_numpy(C_np).to(dev), N, S, Hm, Wm, QUERY_OWN_DEFAULT, a.group)
    bb = a.build_batch
    tok = torch.empty(bb, D, N, device=dev)
    msk = torch.empty(bb * S, Hm, Wm, dtype=torch.uint8, device=dev)
    # the replicated index: every reference image (what EVERY rank of this form holds)
    rows = torch.empty(nR * S, P, device=dev)
    for b0 in range(0, nR, bb):
        nb = min(bb, nR - b0)
        for j in range(nb):
            t, m = fac.reference(b0 + j)
            tok[j] = t
            msk[j * S:(j + 1) * S] = m
        rows[b0 * S:(b0 + nb) * S] = pipe.describe(tok[:nb], msk[:nb * S], (np.arange(nb + 1) * S).astype(np.int32))
    eng.db_add(rows, None)
    del rows, tok, msk
    img_of_seg = torch.arange(nR, device=dev, dtype=torch.int32).repeat_interleave(S)
    tau = np.random.Generator(np.random.PCG64(4000)).integers(0, nR, size=nQ)
    out = {}
    for W in [int(w) for w in a.worlds.split(",") if w.strip()]:
        b = shard_images(nQ, W)
        nQ_l = int(b[1] - b[0])                     # rank 0's block (the largest when W does not divide nQ)
        q_tok = torch.empty(nQ_l, D, N, device=dev)
        q_msk = torch.empty(nQ_l * S, Hm, Wm, dtype=torch.uint8, device=dev)
        for j in range(nQ_l):
            t, m = fac.query(int(tau[j]), j)
            q_tok[j] = t
            q_msk[j * S:(j + 1) * S] = m
        q_off = (np.arange(nQ_l + 1) * S).astype(np.int32)
        eng.hint_query_groups(q_off)

        def rank_step():
            qd = pipe.describe(q_tok, q_msk, q_off)                 # this rank's query images
            d2, idx = eng.search(qd, kv)                           # their segments against ALL rows (k_vote deep: same votes)
            sims, m = eng.sims_from_d2(d2, idx, kv)
            # stand-in for the collective vote: no communicator bound -> this rank's own extrema, no all-gather
            return eng.vote_global(m, sims, q_off, n_top=a.n_top, img_of_seg=img_of_seg)

        for _ in range(a.warmup):
            rank_step()
        eng.set_profiling(True)
        eng.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            rank_step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.iters * 1e3
        stages = {}
        for st in STAGES:
            try:
                v = eng.stage_ms(st)
            except Exception:   # noqa: BLE001 -- a stage this step does not run
                continue
            if v[1]:
                stages[st] = round(v[0] / a.iters, 4)
        eng.set_profiling(False)
        out[str(W)] = {"per_rank_ms": round(ms, 4), "stages_ms": stages, "query_images_described": nQ_l,
                       "query_rows_searched": nQ_l * S, "index_rows": nR * S,
                       "implied_images_per_s": round(nQ / (ms * 1e-3), 1),
                       "collective_bytes_not_executed": QueryShardedRetrieval.collective_bytes(W, nQ, a.n_top)}
        del q_tok, q_msk
    eng.close()
    torch.cuda.empty_cache()
    return {"tool": "query_shard_sim", "geometry": {"query_images": nQ, "db_images": nR, "segments": S, "pca_dim": P, "k_vote": kv},
            "per_rank": out,
            "collective_stand_in": "LOCAL: segvlad_vote_global without a communicator (the rank's own extrema); the 16-byte extrema "
                                   "all-gather, its one-wave reduction and the prediction gather were NOT executed",
            "note": "one rank's compute of a W-way query-sharded run on ONE GPU: implied_images_per_s = nQ / per_rank_ms is an UPPER "
                    "bound on the W-GPU rate -- collectives and load imbalance come on top; not a W-GPU measurement"}


def main(argv=None):
    assert torch.cuda.is_available(), "query_shard_sim needs a GPU"
    print(json.dumps(run(parse(argv))), flush=True)


if __name__ == "__main__":
    main()
