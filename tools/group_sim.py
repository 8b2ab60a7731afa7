"""Timing of the grouped search (segvlad_search_grouped: at most per_image rows per reference image) at the bench geometry, on one MI355X.

Index: 20 000 reference images x 50 segments = 1 M rows of d = 1024, unit rows, in the construction of synth.make_planted_db, drawn
on the device: images in sibling groups share unit base rows, row = normalize(base + sigma_r g / sqrt(d)).  `plain`: groups of one
-- every row an independent direction; `planted`: groups of --group (31: the 17places-like record of bench.py), so every segment
has --group near-identical rows in as many images.  `centred` (not run by default) is the database of exclude_sim.py: each image's
50 rows scattered around the image's own centre, so a row's nearest 50 are its own image and per_image = 1 sends about half the
rows through the exact tail -- what the tail costs.
Queries: 200 of the map's own images x 50 segments (noisy copies of their rows).  Per database and per --fetch setting (0 = the
library's default depth) the tool times, in one process (HIP events, warm, median of --reps): search_grouped(k, per_image) and
the unchanged search at depth k_fetch -- the baseline, code the grouped search does not touch -- and reports their ratio and
group_stats (tail_rows, max_read).  One JSON line."""
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
    p.add_argument("--k", type=int, default=50)
    p.add_argument("--per-image", type=int, default=1)
    p.add_argument("--group", type=int, default=31, help="sibling images per place of the planted database")
    p.add_argument("--sigma-r", type=float, default=0.05, help="noise of a planted row around its base row")
    p.add_argument("--fetch", type=int_list, default=[0], help="inner search depths to measure (option group_fetch; 0 = default)")
    p.add_argument("--db", default="plain,planted", help="databases to run: plain, planted, centred")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    args.db = [x for x in args.db.split(",") if x]
    if args.n_q_img > args.n_ref_img:
        p.error("--n-q-img exceeds --n-ref-img: the queries are images of the map")
    if args.reps < 1 or not 1 <= args.k <= 1024 or not 1 <= args.per_image <= 16 or args.group < 1 or set(args.db) - {"plain", "planted", "centred"}:
        p.error("need reps >= 1, 1 <= k <= 1024, 1 <= per-image <= 16, group >= 1, db among plain / planted / centred")
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


def _rows(kind, args, g):
    """[n_img * S][d] unit rows on the device, in blocks (the noise of 1 M rows at once doubles the peak memory)."""
    import torch

    n_img, S, d = args.n_ref_img, args.segs, args.d
    nrm = torch.nn.functional.normalize
    R = torch.empty(n_img * S, d, device="cuda:0")
    if kind == "centred":
        centres = nrm(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
        for a in range(0, n_img, 2000):
            b = min(n_img, a + 2000)
            blk = centres[a:b].repeat_interleave(S, dim=0)
            R[a * S:b * S] = nrm(blk + 0.5 * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    else:
        G = args.group if kind == "planted" else 1
        step = G if G > 1 else 400                          # (groups of one: many places per block)
        for p0 in range(0, n_img, step):                   # a place: its base rows, then every sibling's noisy copy of them
            sib = min(step, n_img - p0)
            if G > 1:
                blk = nrm(torch.randn(S, d, device="cuda:0", generator=g), dim=1).repeat(sib, 1)
            else:
                blk = nrm(torch.randn(sib * S, d, device="cuda:0", generator=g), dim=1)
            R[p0 * S:(p0 + sib) * S] = nrm(blk + args.sigma_r * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    return R


def run(args) -> dict:
    import torch

    from revisit_anything_amd.engine import SegVLADEngine

    n_img, S, d, k, m = args.n_ref_img, args.segs, args.d, args.k, args.per_image
    out = {"tool": "group_sim", "n_rows": n_img * S, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": args.n_q_img * S,
           "k": k, "per_image": m, "group": args.group, "sigma_r": args.sigma_r, "reps": args.reps,
           "guard": os.environ.get("SEGVLAD_GUARD", "0"), "runs": []}
    for kind in args.db:
        g = torch.Generator(device="cuda:0").manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        frames = np.sort(rng.choice(n_img, args.n_q_img, replace=False))
        R = _rows(kind, args, g)
        img = torch.arange(n_img, device="cuda:0", dtype=torch.int32).repeat_interleave(S)
        eng = SegVLADEngine(0)
        eng.db_add(R, img)
        rows = torch.from_numpy((frames[:, None] * S + np.arange(S)[None, :]).reshape(-1)).cuda()
        Q = torch.nn.functional.normalize(R[rows] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5, dim=1).contiguous()
        del R
        eng.hint_query_groups(np.arange(0, len(rows) + 1, S, dtype=np.int32))
        img_h = img.cpu().numpy()
        for fetch in args.fetch:
            eng.set_option("group_fetch", fetch)
            d2, idx = eng.search_grouped(Q, k, m)
            st = eng.group_stats()
            ids = idx.cpu().numpy()
            worst = 0                                      # (row, image) pairs over the cap among the first rows: must be 0
            for r in ids[:64]:
                gi = img_h[r[r >= 0]]
                worst += int((np.bincount(gi) > m).sum()) if gi.size else 0
            ms = _time(lambda: eng.search_grouped(Q, k, m), args.reps)
            base = _time(lambda: eng.search(Q, st["k_fetch"]), args.reps)
            plain_k = _time(lambda: eng.search(Q, k), args.reps)
            top = eng.search(Q, k)[1].cpu().numpy()
            distinct_plain = float(np.mean([len(np.unique(img_h[r])) for r in top]))
            out["runs"].append({"db": kind, "group_fetch": fetch, "grouped_ms": round(ms, 4), "search_k_fetch_ms": round(base, 4),
                                "ratio": round(ms / base, 4), "search_k_ms": round(plain_k, 4), "k_fetch": st["k_fetch"],
                                "tail_rows": st["tail_rows"], "max_read": st["max_read"], "images_over_cap": worst,
                                "distinct_images_in_plain_top_k": round(distinct_plain, 2)})
        eng.set_option("group_fetch", 0)
        eng.close()
        del Q, img
        torch.cuda.empty_cache()
    return out


def main(argv=None):
    print(json.dumps(run(parse(argv))))


if __name__ == "__main__":
    main()
