"""Timing of the exact range search (segvlad_range_search) against the top-k search it replaces, at the bench geometry, on one
MI355X.

Index: 20 000 reference images x 50 segments = 1 M rows of d = 1024 (unit rows, each image's rows scattered around its own
centre).  Queries: 200 of the map's own frames x 50 segments (noisy copies of their rows), as a batch and the first frame alone.
Per depth c the radius of every query row is the c-th entry (0-based) of its search(Q, 1024) list, so the row has c hits
(ties aside).  Timed in one process (HIP events, warm, median of --reps): search(k = min(1024, c + 24)) -- what a caller has to
run today to cut lists at that radius -- search(k = c) where c <= 1024 names a depth, and ONE segvlad_range_search call whose
capacity suffices; beside them the engine's call with a capacity that is too small (the retry a bad guess costs) and range_stats.
One JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def int_list(text: str):
    return [int(x) for x in text.split(",") if x.strip()]


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--n-ref-img", type=int, default=20000)
    p.add_argument("--segs", type=int, default=50, help="segments per image (reference and query)")
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--n-q-img", type=int, default=200)
    p.add_argument("--depth", type=int_list, default=[50, 1000], help="hits per query row (the radius sits on that list entry)")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if args.n_q_img > args.n_ref_img:
        p.error("--n-q-img exceeds --n-ref-img: the queries are frames of the map")
    if args.reps < 1 or min(args.depth, default=1) < 1 or max(args.depth, default=1) > 1023:
        p.error("need reps >= 1 and 1 <= depth <= 1023")
    return args


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


def run(args) -> dict:
    import torch

    from revisit_anything_amd.engine import SegVLADEngine, _ptr

    g = torch.Generator(device="cuda:0").manual_seed(args.seed)
    n_img, S, d = args.n_ref_img, args.segs, args.d
    n = n_img * S
    rng = np.random.default_rng(args.seed)
    frames = np.sort(rng.choice(n_img, args.n_q_img, replace=False))
    eng = SegVLADEngine(0)
    centres = torch.nn.functional.normalize(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
    R = torch.empty(n, d, device="cuda:0")
    for a in range(0, n_img, 2000):   # (in blocks: the noise of 1 M rows at once doubles the peak memory)
        b = min(n_img, a + 2000)
        blk = centres[a:b].repeat_interleave(S, dim=0)
        R[a * S:b * S] = torch.nn.functional.normalize(blk + 0.5 * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    del centres
    eng.db_add(R)
    rows = (frames[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    Q = torch.nn.functional.normalize(R[torch.from_numpy(rows).cuda()] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5,
                                      dim=1).contiguous()
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    out = {"tool": "range_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": len(rows),
           "reps": args.reps, "guard": os.environ.get("SEGVLAD_GUARD", "0"), "runs": []}
    for name, q, qo in (("batch", Q, qoff), ("single", Q[:S].contiguous(), qoff[:2].copy())):
        nq = q.shape[0]
        eng.hint_query_groups(qo)
        d2_deep, _ = eng.search(q, 1024)
        plain = {}
        for c in args.depth:
            r = d2_deep[:, c].contiguous()                       # device radii: row q has c hits (ties aside)
            lims, d2, idx = eng.range_search(q, r)
            st = eng.range_stats()
            total = int(lims[-1])
            assert total == st["total"] and total <= nq * c
            cap = max(total, 1)
            lims_b = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
            d2_b = torch.empty(cap, dtype=torch.float32, device="cuda:0")
            idx_b = torch.empty(cap, dtype=torch.int64, device="cuda:0")
            tot = C.c_int64()

            def one_call():
                eng._stream()
                rc = eng.lib.segvlad_range_search(eng._h, _ptr(q), nq, _ptr(r), _ptr(lims_b), _ptr(d2_b), _ptr(idx_b), cap, C.byref(tot))
                assert rc == 0 and tot.value == total

            range_ms = _time(one_call, args.reps)
            assert torch.equal(lims_b, lims) and torch.equal(idx_b[:total], idx) and torch.equal(d2_b[:total], d2)

            def retried():
                eng.range_search(q, r, capacity=max(total // 2, 1))

            retry_ms = _time(retried, max(args.reps // 4, 3))
            k_cut = min(1024, c + 24)
            for k in {c, k_cut}:
                if k not in plain:
                    plain[k] = _time(lambda: eng.search(q, k), args.reps)
            out["runs"].append({"shape": name, "depth": c, "total_hits": total, "range_ms": round(range_ms, 4),
                                "range_retry_ms": round(retry_ms, 4), "search_k_ms": round(plain[c], 4), "k_cut": k_cut,
                                "search_k_cut_ms": round(plain[k_cut], 4), "ratio_vs_search_k": round(range_ms / plain[c], 4),
                                "ratio_vs_search_k_cut": round(range_ms / plain[k_cut], 4), "cand_mean": round(st["cand_sum"] / nq, 1),
                                "cand_max": st["cand_max"], "long_rows": st["long_rows"], "path": st["path"]})
    eng.close()
    return out


def main(argv=None):
    print(json.dumps(run(parse(argv))))


if __name__ == "__main__":
    main()
