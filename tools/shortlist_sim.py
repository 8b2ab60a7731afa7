"""Timing of the shortlist-restricted exact search (segvlad_search_shortlist) at the bench geometry, on one MI355X.

Index: 20 000 reference images x 50 segments = 1 M rows of d = 1024 (unit rows, each image's rows scattered around its own
centre).  Queries: 200 images x 50 segments, noisy copies of reference images' rows.  Per query image the shortlist holds its
true image plus M - 1 random others (distinct).  For every (M, k) the tool times search_shortlist (median of --reps calls after a
warm-up; the image -> row map is built once before timing), and reports the exact-GEMM flops of the pass (query rows x union rows
x 2 d), its effective rate against the 157 TF/s fp32 matrix peak, the row bytes the GEMM gathers (a group reads its union once
per group), and segvlad_search on the same queries at the same k for comparison.  One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK_TFS = 157.3


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--n-ref-img", type=int, default=20000)
    p.add_argument("--segs", type=int, default=50, help="segments per image (reference and query)")
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--n-q-img", type=int, default=200)
    p.add_argument("--m", default="25,100,400", help="shortlist lengths M")
    p.add_argument("--k", default="50,200", help="search depths k")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    return p.parse_args(argv)


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main(argv=None):
    args = parse(argv)
    import torch

    from revisit_anything_amd.engine import SegVLADEngine

    g = torch.Generator(device="cuda:0").manual_seed(args.seed)
    n_img, S, d = args.n_ref_img, args.segs, args.d
    n = n_img * S
    eng = SegVLADEngine(0)
    centres = torch.nn.functional.normalize(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
    R = torch.empty(n, d, device="cuda:0")
    for a in range(0, n_img, 2000):   # (in blocks: the noise of 1 M rows at once doubles the peak memory)
        b = min(n_img, a + 2000)
        blk = centres[a:b].repeat_interleave(S, dim=0)
        R[a * S:b * S] = torch.nn.functional.normalize(blk + 0.5 * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    img = torch.arange(n_img, device="cuda:0", dtype=torch.int32).repeat_interleave(S)
    eng.db_add(R, img)
    rng = np.random.default_rng(args.seed)
    truth = rng.choice(n_img, args.n_q_img, replace=False)
    rows = (truth[:, None] * S + rng.integers(0, S, (args.n_q_img, S))).reshape(-1)
    Q = torch.nn.functional.normalize(R[torch.from_numpy(rows).cuda()] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5,
                                      dim=1).contiguous()
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    nq = len(rows)
    del centres
    out = {"tool": "shortlist_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": nq,
           "peak_fp32_matrix_tfs": FP32_MATRIX_PEAK_TFS, "runs": []}
    full_ms = {}
    for k in [int(x) for x in args.k.split(",")]:
        full_ms[k] = _time(lambda: eng.search(Q, k), args.reps)
    for M in [int(x) for x in args.m.split(",")]:
        sl = np.empty((args.n_q_img, M), np.int32)
        for b in range(args.n_q_img):
            others = rng.choice(n_img - 1, M - 1, replace=False)
            others[others >= truth[b]] += 1
            sl[b] = np.concatenate([[truth[b]], others])
        sl_dev = torch.from_numpy(sl).cuda()
        union_rows = M * S
        flop = 2.0 * nq * union_rows * d
        groups = args.n_q_img * ((S + 63) // 64)
        gathered = groups * union_rows * d * 4
        for k in [int(x) for x in args.k.split(",")]:
            ms = _time(lambda: eng.search_shortlist(Q, qoff, sl_dev, k), args.reps)
            out["runs"].append({"M": M, "k": k, "ms": round(ms, 4), "tflops_eff": round(flop / ms / 1e9, 2),
                                "frac_of_peak": round(flop / ms / 1e9 / FP32_MATRIX_PEAK_TFS, 3), "flop": flop,
                                "gathered_bytes": gathered, "full_search_ms": round(full_ms[k], 4),
                                "speedup_vs_full": round(full_ms[k] / ms, 2)})
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
