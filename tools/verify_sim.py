"""Timing of the spatial verification (segvlad_verify_pairs) behind the re-ranking it follows, at the bench geometry, on one MI355X.

Index and queries as tools/match_sim.py: 20 000 reference images x 50 segments = 1 M rows of d = 1024, image ids are frame
numbers; 200 of the map's own frames x 50 segments (noisy copies of their rows), as a batch and the first frame alone; per query
image its true frame at a random slot among C - 1 other frames, for every C of --cands.  Centroids: every index row gets a point
of a 320 x 240 frame; a query image's rows get the points of the rows they copy, moved by one similarity per image (scale
0.7 .. 1.4, rotation +-0.3 rad, a shift) plus 0.5 px of noise -- the true frame's pairs follow one similarity, the other frames'
pairs none.  Timed in one process (HIP events, warm, median of --reps), both through the C entry points on preallocated device
outputs: ONE segvlad_match_pairs call with every output asked for, and ONE segvlad_verify_pairs call on its fwd_idx / mutual with
every output asked for.  Beside them: their ratio, and the share of query images whose true frame the verification puts first.
One JSON line; --out also writes it to a file (run with SEGVLAD_GUARD=0)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import match_sim  # noqa: E402  (tools/match_sim.py: the candidates' generator, the timer, the list parser)


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--n-ref-img", type=int, default=20000)
    p.add_argument("--segs", type=int, default=50, help="segments per image (reference and query), at most 256")
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--n-q-img", type=int, default=200)
    p.add_argument("--cands", type=match_sim.int_list, default=[5, 20], help="candidate images per query image (C)")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--tol", type=float, default=3.0, help="inlier radius in pixels")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = p.parse_args(argv)
    if args.n_q_img > args.n_ref_img:
        p.error("--n-q-img exceeds --n-ref-img: the queries are frames of the map")
    if args.reps < 1 or min(args.cands, default=1) < 1 or max(args.cands, default=1) > 64 or max(args.cands, default=1) > args.n_ref_img:
        p.error("need reps >= 1 and 1 <= C <= min(64, --n-ref-img)")
    if not 1 <= args.segs <= 256 or not args.tol > 0:
        p.error("need 1 <= --segs <= 256 and --tol > 0")
    return args


def make_centroids(n_rows, rows_of_query, segs, rng, noise=0.5):
    """r_xy [n_rows][2]: a point of a 320 x 240 frame per index row; q_xy: query row i copies index row rows_of_query[i], and every
    run of `segs` query rows (one image) is moved by its own similarity, then jittered by `noise` pixels."""
    r_xy = rng.uniform([0.0, 0.0], [320.0, 240.0], (n_rows, 2))
    n_img = len(rows_of_query) // segs
    a = rng.uniform(0.7, 1.4, n_img) * np.exp(1j * rng.uniform(-0.3, 0.3, n_img))
    t = rng.uniform(-40.0, 40.0, n_img) + 1j * rng.uniform(-30.0, 30.0, n_img)
    s = r_xy[rows_of_query, 0] + 1j * r_xy[rows_of_query, 1]
    # the reference point is a p + t: the query point is (s - t) / a
    p = (s - np.repeat(t, segs)) / np.repeat(a, segs)
    q_xy = np.stack([p.real, p.imag], 1) + rng.normal(0.0, noise, (len(rows_of_query), 2))
    return np.ascontiguousarray(q_xy), np.ascontiguousarray(r_xy)


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
    eng.db_add(R, np.repeat(np.arange(n_img, dtype=np.int32), S))
    rows = (frames[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    Q = torch.nn.functional.normalize(R[torch.from_numpy(rows).cuda()] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5,
                                      dim=1).contiguous()
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    q_xy_h, r_xy_h = make_centroids(n, rows, S, rng)
    q_xy, r_xy = torch.from_numpy(q_xy_h).cuda(), torch.from_numpy(r_xy_h).cuda()
    out = {"tool": "verify_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": len(rows),
           "reps": args.reps, "tol": args.tol, "guard": os.environ.get("SEGVLAD_GUARD", "0"), "runs": []}
    for name, q, qo, fr, qxy in (("batch", Q, qoff, frames, q_xy),
                                 ("single", Q[:S].contiguous(), qoff[:2].copy(), frames[:1], q_xy[:S].contiguous())):
        nq, nb = q.shape[0], len(qo) - 1
        for C in args.cands:
            cand, slot = match_sim.make_candidates(fr, n_img, C, rng)
            mp = eng.match_pairs(q, qo, cand, want_rows=True)
            vp = eng.verify_pairs(qxy, r_xy, qo, mp["fwd_idx"], mp["mutual"], args.tol, want_rows=True)
            first = vp["order"][:, 0].cpu().numpy()
            n_inl = vp["n_inlier"].cpu().numpy()
            om = {k: torch.empty_like(v) for k, v in mp.items()}
            ov = {k: torch.empty_like(v) for k, v in vp.items()}

            def match_call():
                eng._stream()
                rc = eng.lib.segvlad_match_pairs(eng._h, _ptr(q), nq, _ptr(qo), nb, _ptr(cand), C, float("inf"), _ptr(om["n_mutual"]),
                                                 _ptr(om["score"]), _ptr(om["order"]), _ptr(om["fwd_idx"]), _ptr(om["fwd_d2"]), _ptr(om["mutual"]))
                assert rc == 0

            def verify_call():
                eng._stream()
                rc = eng.lib.segvlad_verify_pairs(eng._h, _ptr(qxy), nq, _ptr(r_xy), n, _ptr(qo), nb, C, _ptr(mp["fwd_idx"]), _ptr(mp["mutual"]),
                                                  args.tol, 0.5, 2.0, _ptr(ov["n_inlier"]), _ptr(ov["pair"]), _ptr(ov["model"]),
                                                  _ptr(ov["order"]), _ptr(ov["inlier"]))
                assert rc == 0

            match_ms = match_sim._time(match_call, args.reps)
            verify_ms = match_sim._time(verify_call, args.reps)
            assert all(torch.equal(ov[k], vp[k]) for k in vp if k != "model")   # (two calls, the same bits; the model holds NaN)
            assert torch.equal(ov["model"].view(torch.int64), vp["model"].view(torch.int64))
            out["runs"].append({"shape": name, "C": C, "verify_ms": round(verify_ms, 4), "match_ms": round(match_ms, 4),
                                "ratio": round(verify_ms / match_ms, 4), "true_first": round(float((first == slot).mean()), 4),
                                "n_inlier_true_mean": round(float(n_inl[np.arange(nb), slot].mean()), 2),
                                "n_inlier_other_max": int(np.where(np.arange(C)[None, :] == slot[:, None], -1, n_inl).max())})
    eng.close()
    return out


def main(argv=None):
    args = parse(argv)
    line = json.dumps(run(args))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
