"""Timing of the mutual-nearest-segment re-ranking (segvlad_match_pairs) at the bench geometry, on one MI355X.

Index: 20 000 reference images x 50 segments = 1 M rows of d = 1024 (unit rows, each image's rows scattered around its own
centre); image ids are frame numbers.  Queries: 200 of the map's own frames x 50 segments (noisy copies of their rows), as a
batch and the first frame alone.  Candidates per query image: its true frame at a random slot among C - 1 other frames, for every
C of --cands.  Timed in one process (HIP events, warm, median of --reps): ONE segvlad_match_pairs call with every output asked
for, and the baseline -- C calls of segvlad_search_shortlist(M = 1, k = 1), one per slot column, which return only the forward
half (each row's nearest row of the candidate) and run code the re-ranking does not touch.  Both through the C entry points on
preallocated device outputs.  Beside them: the share of query images whose true frame the re-ranking puts first, and the call as
a fraction of a retrieve() (search 200 deep, vote) of the same queries.  One JSON line."""
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
    p.add_argument("--cands", type=int_list, default=[5, 20], help="candidate images per query image (C)")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if args.n_q_img > args.n_ref_img:
        p.error("--n-q-img exceeds --n-ref-img: the queries are frames of the map")
    if args.reps < 1 or min(args.cands, default=1) < 1 or max(args.cands, default=1) > 64 or max(args.cands, default=1) > args.n_ref_img:
        p.error("need reps >= 1 and 1 <= C <= min(64, --n-ref-img)")
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


def make_candidates(frames, n_ref_img, C, rng):
    """[len(frames)][C] int32: every row holds its frame at a random slot among C - 1 distinct other frames; and the slots."""
    cand = np.empty((len(frames), C), np.int32)
    slot = rng.integers(0, C, len(frames))
    for b, f in enumerate(frames):
        others = rng.choice(n_ref_img - 1, C - 1, replace=False)
        others = others + (others >= f)
        cand[b] = np.insert(others, slot[b], f)
    return cand, slot


def run(args) -> dict:
    import torch

    from revisit_anything_amd.engine import SegVLADEngine, _ptr
    from revisit_anything_amd.pipeline import SegVLADPipeline

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
    pipe = SegVLADPipeline(eng, 112, 140)
    out = {"tool": "match_sim", "n_rows": n, "n_ref_img": n_img, "segs": S, "d": d, "n_q_img": args.n_q_img, "nq": len(rows),
           "reps": args.reps, "guard": os.environ.get("SEGVLAD_GUARD", "0"), "colmin": "atomic", "runs": []}
    for name, q, qo, fr in (("batch", Q, qoff, frames), ("single", Q[:S].contiguous(), qoff[:2].copy(), frames[:1])):
        nq, nb = q.shape[0], len(qo) - 1
        retrieve_ms = _time(lambda: pipe.retrieve(q, qo), max(args.reps // 4, 3))
        for C in args.cands:
            cand, slot = make_candidates(fr, n_img, C, rng)
            res = eng.match_pairs(q, qo, cand, want_rows=True)
            first = res["order"][:, 0].cpu().numpy()
            n_mut = res["n_mutual"].cpu().numpy()
            o = {k: torch.empty_like(v) for k, v in res.items()}

            def one_call():
                eng._stream()
                rc = eng.lib.segvlad_match_pairs(eng._h, _ptr(q), nq, _ptr(qo), nb, _ptr(cand), C, float("inf"), _ptr(o["n_mutual"]),
                                                 _ptr(o["score"]), _ptr(o["order"]), _ptr(o["fwd_idx"]), _ptr(o["fwd_d2"]), _ptr(o["mutual"]))
                assert rc == 0

            match_ms = _time(one_call, args.reps)
            assert all(torch.equal(o[k], res[k]) for k in res)
            cols = [np.ascontiguousarray(cand[:, j:j + 1]) for j in range(C)]
            bd2 = torch.empty(C, nq, 1, dtype=torch.float32, device="cuda:0")
            bidx = torch.empty(C, nq, 1, dtype=torch.int64, device="cuda:0")

            def baseline():
                eng._stream()
                for j in range(C):
                    rc = eng.lib.segvlad_search_shortlist(eng._h, _ptr(q), nq, _ptr(qo), nb, _ptr(cols[j]), 1, 1, _ptr(bd2[j]), _ptr(bidx[j]))
                    assert rc == 0

            base_ms = _time(baseline, args.reps)
            assert torch.equal(bidx[:, :, 0].T.contiguous(), res["fwd_idx"]) and torch.equal(bd2[:, :, 0].T.contiguous(), res["fwd_d2"])
            out["runs"].append({"shape": name, "C": C, "match_ms": round(match_ms, 4), "shortlist_calls_ms": round(base_ms, 4),
                                "ratio": round(match_ms / base_ms, 4), "true_first": round(float((first == slot).mean()), 4),
                                "n_mutual_true_mean": round(float(n_mut[np.arange(nb), slot].mean()), 2),
                                "n_mutual_other_max": int(np.where(np.arange(C)[None, :] == slot[:, None], -1, n_mut).max()),
                                "retrieve_ms": round(retrieve_ms, 4), "fraction_of_retrieve": round(match_ms / retrieve_ms, 4)})
    eng.close()
    return out


def main(argv=None):
    print(json.dumps(run(parse(argv))))


if __name__ == "__main__":
    main()
