#!/usr/bin/env python3
"""One measurement for DESIGN.md ("Per-image cap in the vote"): segvlad_vote at 200 query images x 50 segments x k = 50 on concentrated
lists (the generator of tests/search_tail_ref.py's vote cases: half of every image's entries on four reference images of its own),
operands on the device -- mode 0 without a cap, with SEGVLAD_VOTE_PER_IMAGE(1) and with SEGVLAD_VOTE_PER_IMAGE(4).  Per run 10 warm-up
and 50 timed steps: the call by wall clock between two synchronisations, and its kernels by the library's stage timer ("vote") in a
second loop.  Every run is a fresh process; with --parent-lib (a build of the parent commit's library, which knows no cap) the runs of
the two libraries alternate, and the uncapped time is held against the parent's: the ratio of the medians next to the run-to-run
spread of each.  Reported, never asserted.

    python tools/measure_vote_cap.py [--runs 5] [--parent-lib PATH/libsegvlad_hip.so] [--out profiles/vote_cap.json]

Needs a GPU; there is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_IMG, SEGS, K, N_TOP = 200, 50, 50, 5


def lists():
    import search_tail_ref as R

    rng = np.random.default_rng(20050)
    im = R.ref_map()
    off = (np.arange(N_IMG + 1) * SEGS).astype(np.int32)
    matches, _ = R._concentrated(rng, off, K, im)
    sims = np.sort(rng.uniform(0.2, 1.9, size=matches.shape).astype(np.float32), axis=1)[:, ::-1].copy()
    return matches, sims, off, im


def one_run(caps, warmup, steps):
    """This process: one library (SEGVLAD_LIB_PATH or the tree's), every cap of `caps` (0 = no cap)."""
    import torch

    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    matches, sims, off, im = lists()
    dm, ds, di = (torch.from_numpy(x).to(eng.device) for x in (matches, sims, im))
    out = {}
    for m in caps:
        mode = m << 8

        def call():
            return eng.vote(dm, ds, off, n_top=N_TOP, mode=mode, img_of_seg=di)

        wall = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if i >= warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.profile_reset()
        for _ in range(steps):
            call()
        eng.synchronize()
        k_ms, n_launch = eng.stage_ms("vote")
        eng.set_profiling(False)
        out[str(m)] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)),
                       "stage_vote_ms_per_call": k_ms / steps, "launches_per_call": n_launch / steps}
    eng.close()
    return out


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(x), 5) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vote_cap.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(one_run([int(x) for x in args.child.split(",")], args.warmup, args.steps)))
        return

    def child(caps, lib):
        env = dict(os.environ)
        env.pop("SEGVLAD_LIB_PATH", None)
        if lib:
            env["SEGVLAD_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", caps, "--warmup", str(args.warmup), "--steps", str(args.steps)],
                           env=env, stdout=subprocess.PIPE, timeout=300, check=True)
        line = [x for x in r.stdout.decode().splitlines() if x.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    this, parent = [], []                                    # (this process opens the GPU only after its last child has ended)
    for _ in range(args.runs):
        this.append(child("0,1,4", None))
        if args.parent_lib:
            parent.append(child("0", os.path.abspath(args.parent_lib)))
    import torch
    import vote_cap_ref as V

    matches, _, _, im = lists()
    res = {
        "tool": "measure_vote_cap",
        "what": "segvlad_vote, mode WT_BORDA_IM, device operands, NaN extrema: wall clock between synchronisations and the 'vote' stage "
                "timer; one fresh process per run, this library and the parent commit's alternating",
        "device": torch.cuda.get_device_name(0),
        "n_img": N_IMG, "segs": SEGS, "k": K, "n_top": N_TOP, "warmup": args.warmup, "steps": args.steps, "runs": args.runs, "guard": "0",
        "blanked_share": {str(m): round(V.blanked_share(dict(matches=matches, img_of_seg=im), m), 4) for m in (1, 4)},
        "this": {f"m{m}": {"wall_ms": spread([r[str(m)]["wall_ms_median"] for r in this]),
                           "stage_vote_ms": spread([r[str(m)]["stage_vote_ms_per_call"] for r in this]),
                           "launches_per_call": this[0][str(m)]["launches_per_call"]} for m in (0, 1, 4)},
    }
    t0 = res["this"]["m0"]
    for m in (1, 4):
        res["this"][f"m{m}"]["stage_ratio_to_m0"] = round(res["this"][f"m{m}"]["stage_vote_ms"]["median"] / t0["stage_vote_ms"]["median"], 4)
        res["this"][f"m{m}"]["wall_ratio_to_m0"] = round(res["this"][f"m{m}"]["wall_ms"]["median"] / t0["wall_ms"]["median"], 4)
    if parent:
        p = {"wall_ms": spread([r["0"]["wall_ms_median"] for r in parent]),
             "stage_vote_ms": spread([r["0"]["stage_vote_ms_per_call"] for r in parent]),
             "launches_per_call": parent[0]["0"]["launches_per_call"]}
        res["parent_m0"] = p
        res["m0_vs_parent"] = {
            "wall_ratio": round(t0["wall_ms"]["median"] / p["wall_ms"]["median"], 4),
            "stage_ratio": round(t0["stage_vote_ms"]["median"] / p["stage_vote_ms"]["median"], 4),
            "parent_wall_spread": round(p["wall_ms"]["max"] / p["wall_ms"]["min"], 4),
            "this_wall_spread": round(t0["wall_ms"]["max"] / t0["wall_ms"]["min"], 4),
            "parent_stage_spread": round(p["stage_vote_ms"]["max"] / p["stage_vote_ms"]["min"], 4),
            "this_stage_spread": round(t0["stage_vote_ms"]["max"] / t0["stage_vote_ms"]["min"], 4),
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
