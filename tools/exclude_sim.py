"""Timing of the search that excludes image-id windows (segvlad_search_excluding) at the bench geometry, on one MI355X.

Index: 20 000 reference images x 50 segments = 1 M rows of d = 1024 (unit rows, each image's rows scattered around its own
centre); image ids are frame numbers.  Queries: 200 of the map's own frames x 50 segments (noisy copies of their rows), as a
batch and the first frame alone.  For every (k, window radius) the tool times, in one process (HIP events, warm, median of
--reps): search(k), search(k_fetch) -- the baseline: the same inner search, code the exclusion does not touch -- and
search_excluding, and reports exclude_stats.  --crowd R0 draws the rows of the frames within R0 of the FIRST query frame tightly
around that frame's centre, so that with (2 R0 + 1) x segs >= 1024 and radius >= R0 that image's rows go through the exact tail
(its time per group is then the single-image figure).  --alt also times what the call replaces for ONE window: db_remove of the
window's images, search(k), db_add of the rows again.  One JSON line."""
from __future__ import annotations

import argparse
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
    p.add_argument("--k", type=int_list, default=[50, 200], help="search depths k")
    p.add_argument("--radius", type=int_list, default=[0, 5, 20, 200], help="window radii (frames on either side)")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--crowd", type=int, default=0, help="frames on either side of the first query frame drawn around its centre")
    p.add_argument("--alt", action="store_true", help="also time db_remove + search + db_add for one window")
    args = p.parse_args(argv)
    if args.n_q_img > args.n_ref_img:
        p.error("--n-q-img exceeds --n-ref-img: the queries are frames of the map")
    if args.reps < 1 or min(args.k, default=1) < 1 or max(args.k, default=1) > 1024 or min(args.radius, default=0) < 0:
        p.error("need reps >= 1, 1 <= k <= 1024, radius >= 0")
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

    from revisit_anything_amd.engine import SegVLADEngine, window_intervals

    g = torch.Generator(device="cuda:0").manual_seed(args.seed)
    n_img, S, d = args.n_ref_img, args.segs, args.d
    n = n_img * S
    rng = np.random.default_rng(args.seed)
    frames = np.sort(rng.choice(n_img, args.n_q_img, replace=False))
    eng = SegVLADEngine(0)
    centres = torch.nn.functional.normalize(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
    if args.crowd > 0:
        f0 = int(frames[0])
        centres[max(f0 - args.crowd, 0):f0 + args.crowd + 1] = centres[f0].clone()
    R = torch.empty(n, d, device="cuda:0")
    for a in range(0, n_img, 2000):   # (in blocks: the noise of 1 M rows at once doubles the peak memory)
        b = min(n_img, a + 2000)
        blk = centres[a:b].repeat_interleave(S, dim=0)
        R[a * S:b * S] = torch.nn.functional.normalize(blk + 0.5 * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    img = torch.arange(n_img, device="cuda:0", dtype=torch.int32).repeat_interleave(S)
    eng.db_add(R, img)
    rows = (frames[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    Q = torch.nn.functional.normalize(R[torch.from_numpy(rows).cuda()] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5,
                                      dim=1).contiguous()
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    del centres
    out = {"tool": "exclude_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": len(rows),
           "reps": args.reps, "crowd": args.crowd, "guard": os.environ.get("SEGVLAD_GUARD", "0"), "runs": []}
    shapes = (("batch", Q, qoff, slice(0, args.n_q_img)), ("single", Q[:S].contiguous(), qoff[:2].copy(), slice(0, 1)))
    plain = {}
    for name, q, qo, sel in shapes:
        eng.hint_query_groups(qo)
        for r in args.radius:
            ex = window_intervals(frames[sel], r)
            for k in args.k:
                eng.search_excluding(q, qo, ex, k)
                st = eng.exclude_stats()
                for depth in {k, st["k_fetch"]}:
                    if (name, depth) not in plain:
                        plain[(name, depth)] = _time(lambda: eng.search(q, depth), args.reps)
                ms = _time(lambda: eng.search_excluding(q, qo, ex, k), args.reps)
                base = plain[(name, st["k_fetch"])]
                out["runs"].append({"shape": name, "k": k, "radius": r, "exclude_ms": round(ms, 4), "search_k_ms": round(plain[(name, k)], 4),
                                    "search_k_fetch_ms": round(base, 4), "ratio_vs_k_fetch": round(ms / base, 4),
                                    "depth_cost": round(base / plain[(name, k)], 4), "exclude_stats": st})
    if args.alt:
        f, r, k = int(frames[0]), max(args.radius), args.k[0]
        q = Q[:S].contiguous()
        window = np.arange(max(f - r, 0), min(f + r, n_img - 1) + 1, dtype=np.int32)
        back = slice(int(window[0]) * S, (int(window[-1]) + 1) * S)
        Rw, iw = R[back].contiguous(), img[back].contiguous()

        def alt():
            eng.db_remove(img_ids=window)
            eng.search(q, k)
            eng.db_add(Rw, iw)

        out["alt"] = {"k": k, "radius": r, "remove_search_add_ms": round(_time(alt, min(args.reps, 3)), 4)}
    eng.close()
    return out


def main(argv=None):
    print(json.dumps(run(parse(argv))))


if __name__ == "__main__":
    main()
