"""Timing of the sequence re-ranking (segvlad_sequence_rerank) behind the vote that produces its input, at the bench geometry, on one MI355X.

Index as tools/match_sim.py: 20 000 reference images x 50 segments = 1 M rows of d = 1024, image ids are frame numbers.  Queries: a
traversal of --n-q-img consecutive map frames (velocity 1) x 50 segments, noisy copies of their rows; in a share --alias of the
frames 30 of the 50 segments copy the rows of ONE distant frame instead -- perceptual aliasing: the distractor out-votes the true
frame there and has no support in the frames around it.  Per C of --cands: search (k = --k) -> sims_from_d2 -> vote(n_top = C, with
scores) -> sequence_rerank(back, fwd, --n-vel velocities of 0.8 .. 1.2, tol) on the vote's tensors as they are.  Timed in one
process (HIP events, warm, median of --reps), both through the C entry points on preallocated device outputs: ONE segvlad_vote call
and ONE segvlad_sequence_rerank call with every output asked for.  Beside them: their ratio, and the share of frames whose true
frame comes first before and after the stage.  Then the heaviest legal shape on its own: --heavy-frames frames x --heavy-c slots,
back = fwd = --heavy-window, --heavy-vel velocities, ids drawn around the frame number so that most lookups hit (0 frames: skipped).
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

import match_sim  # noqa: E402  (tools/match_sim.py: the timer, the list parser)


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--n-ref-img", type=int, default=20000)
    p.add_argument("--segs", type=int, default=50, help="segments per image (reference and query)")
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--n-q-img", type=int, default=200, help="query frames: consecutive frames of the map")
    p.add_argument("--k", type=int, default=50, help="depth of the search and of the vote")
    p.add_argument("--cands", type=match_sim.int_list, default=[5, 20], help="candidates per frame (n_top of the vote = C)")
    p.add_argument("--back", type=int, default=5)
    p.add_argument("--fwd", type=int, default=5)
    p.add_argument("--n-vel", type=int, default=5, help="velocities, evenly spaced in 0.8 .. 1.2")
    p.add_argument("--tol", type=int, default=1)
    p.add_argument("--alias", type=float, default=0.2, help="share of the query frames a distant frame out-votes")
    p.add_argument("--heavy-frames", type=int, default=10000)
    p.add_argument("--heavy-c", type=int, default=64)
    p.add_argument("--heavy-window", type=int, default=32)
    p.add_argument("--heavy-vel", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = p.parse_args(argv)
    if args.n_q_img > args.n_ref_img or args.n_q_img < 1:
        p.error("need 1 <= --n-q-img <= --n-ref-img: the queries are frames of the map")
    if args.reps < 1 or min(args.cands, default=1) < 1 or max(args.cands, default=1) > 64 or max(args.cands, default=1) > args.n_ref_img:
        p.error("need reps >= 1 and 1 <= C <= min(64, --n-ref-img)")
    if not (0 <= args.back <= 32 and 0 <= args.fwd <= 32 and 1 <= args.n_vel <= 16 and 0 <= args.tol <= 2 ** 30 and args.k >= 1):
        p.error("need 0 <= --back, --fwd <= 32, 1 <= --n-vel <= 16, 0 <= --tol <= 2^30, --k >= 1")
    if not (0.0 <= args.alias <= 1.0 and args.heavy_frames >= 0 and 1 <= args.heavy_c <= 64 and 0 <= args.heavy_window <= 32
            and 1 <= args.heavy_vel <= 16):
        p.error("need 0 <= --alias <= 1, --heavy-frames >= 0, 1 <= --heavy-c <= 64, 0 <= --heavy-window <= 32, 1 <= --heavy-vel <= 16")
    return args


def make_heavy_lists(T, C, rng):
    """cand int32 [T][C]: frame t lists ids of t + 100 +- 100, so the frames around it hold ids near every line; score fp64 [T][C]
    in [0, 1).  Every slot is filled."""
    cand = (np.arange(T)[:, None] + rng.integers(0, 201, (T, C))).astype(np.int32)
    return np.ascontiguousarray(cand), np.ascontiguousarray(rng.random((T, C)))


def run(args) -> dict:
    import torch

    from revisit_anything_amd import _lib
    from revisit_anything_amd.engine import SegVLADEngine, _ptr, velocity_grid

    g = torch.Generator(device="cuda:0").manual_seed(args.seed)
    n_img, S, d, nf = args.n_ref_img, args.segs, args.d, args.n_q_img
    n = n_img * S
    rng = np.random.default_rng(args.seed)
    f0 = int(rng.integers(0, n_img - nf + 1))
    frames = f0 + np.arange(nf)
    eng = SegVLADEngine(0)
    centres = torch.nn.functional.normalize(torch.randn(n_img, d, device="cuda:0", generator=g), dim=1)
    R = torch.empty(n, d, device="cuda:0")
    for a in range(0, n_img, 2000):   # (in blocks: the noise of 1 M rows at once doubles the peak memory)
        b = min(n_img, a + 2000)
        blk = centres[a:b].repeat_interleave(S, dim=0)
        R[a * S:b * S] = torch.nn.functional.normalize(blk + 0.5 * torch.randn(blk.shape, device="cuda:0", generator=g) / d ** 0.5, dim=1)
    del centres
    eng.db_add(R, np.repeat(np.arange(n_img, dtype=np.int32), S))
    rows = (frames[:, None] * S + np.arange(S)[None, :])
    n_alias = min(S, 30)
    aliased = rng.random(nf) < args.alias
    for t in np.flatnonzero(aliased):   # a frame at least 1000 frames away (or the farthest there is) lends its rows
        far = (frames[t] + n_img // 2) % n_img if n_img < 4000 else int((frames[t] + rng.integers(1000, n_img - 1000)) % n_img)
        rows[t, :n_alias] = far * S + np.arange(n_alias)
    rows = rows.reshape(-1)
    Q = torch.nn.functional.normalize(R[torch.from_numpy(rows).cuda()] + 0.3 * torch.randn(len(rows), d, device="cuda:0", generator=g) / d ** 0.5,
                                      dim=1).contiguous()
    qoff = np.arange(0, len(rows) + 1, S, dtype=np.int32)
    nq = len(rows)
    vel = velocity_grid(0.8, 1.2, args.n_vel)
    so = np.array([0, nf], np.int32)
    out = {"tool": "sequence_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": nf, "nq": nq, "k": args.k,
           "back": args.back, "fwd": args.fwd, "n_vel": args.n_vel, "tol": args.tol, "alias": args.alias, "reps": args.reps,
           "guard": os.environ.get("SEGVLAD_GUARD", "0"), "runs": []}
    eng.hint_query_groups(qoff)
    d2, idx = eng.search(Q, args.k)
    sims, m = eng.sims_from_d2(d2, idx, args.k)
    for C in args.cands:
        pred, sc = eng.vote(m, sims, qoff, n_top=C, want_scores=True)
        res = eng.sequence_rerank(pred, sc, None, args.back, args.fwd, vel, args.tol)
        before = pred[:, 0].cpu().numpy()
        after = torch.gather(pred, 1, res["order"][:, :1].to(torch.int64))[:, 0].cpu().numpy()
        ov = (torch.empty_like(pred), torch.empty_like(sc))
        o = {k: torch.empty_like(v) for k, v in res.items()}

        def vote_call():
            eng._stream()
            rc = eng.lib.segvlad_vote(eng._h, _ptr(m), _ptr(sims), None, 0, _ptr(qoff), nf, args.k, float("nan"), float("nan"), C,
                                      int(_lib.VOTE_WT_BORDA_IM), _ptr(ov[0]), _ptr(ov[1]))
            assert rc == 0

        def sequence_call():
            eng._stream()
            rc = eng.lib.segvlad_sequence_rerank(eng._h, _ptr(pred), _ptr(sc), nf, C, _ptr(so), 1, args.back, args.fwd, _ptr(vel), len(vel),
                                                 args.tol, _ptr(o["seq_score"]), _ptr(o["n_hit"]), _ptr(o["vel"]), _ptr(o["order"]))
            assert rc == 0

        vote_ms = match_sim._time(vote_call, args.reps)
        seq_ms = match_sim._time(sequence_call, args.reps)
        assert torch.equal(ov[0], pred) and torch.equal(ov[1].view(torch.int64), sc.view(torch.int64))
        assert all(torch.equal(o[k], res[k]) for k in res if k != "seq_score")   # (two calls, the same bits)
        assert torch.equal(o["seq_score"].view(torch.int64), res["seq_score"].view(torch.int64))
        out["runs"].append({"shape": "batch", "C": C, "sequence_ms": round(seq_ms, 4), "vote_ms": round(vote_ms, 4),
                            "ratio": round(seq_ms / vote_ms, 4), "true_first_before": round(float((before == frames).mean()), 4),
                            "true_first_after": round(float((after == frames).mean()), 4),
                            "aliased_frames": int(aliased.sum())})
    if args.heavy_frames > 0:
        T, C, w = args.heavy_frames, args.heavy_c, args.heavy_window
        cand_h, score_h = make_heavy_lists(T, C, rng)
        cand, score = torch.from_numpy(cand_h).cuda(), torch.from_numpy(score_h).cuda()
        hv = velocity_grid(0.5, 2.0, args.heavy_vel)
        hso = np.array([0, T], np.int32)
        res = eng.sequence_rerank(cand, score, None, w, w, hv, args.tol)
        o = {k: torch.empty_like(v) for k, v in res.items()}

        def heavy_call():
            eng._stream()
            rc = eng.lib.segvlad_sequence_rerank(eng._h, _ptr(cand), _ptr(score), T, C, _ptr(hso), 1, w, w, _ptr(hv), len(hv), args.tol,
                                                 _ptr(o["seq_score"]), _ptr(o["n_hit"]), _ptr(o["vel"]), _ptr(o["order"]))
            assert rc == 0

        heavy_ms = match_sim._time(heavy_call, args.reps)
        assert torch.equal(o["order"], res["order"]) and torch.equal(o["seq_score"].view(torch.int64), res["seq_score"].view(torch.int64))
        out["heavy"] = {"T": T, "C": C, "back": w, "fwd": w, "n_vel": len(hv), "tol": args.tol, "sequence_ms": round(heavy_ms, 4),
                        "n_hit_mean": round(float(res["n_hit"].to(torch.float64).mean()), 2)}
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
