#!/usr/bin/env python3
"""One measurement for DESIGN.md ("One-to-one vote"): segvlad_vote at 200 query images x 50 segments x k = 50 on concentrated lists
(the lists of tools/measure_vote_cap.py: half of every image's entries on four reference images of its own), operands on the device
-- mode 0, with SEGVLAD_VOTE_UNIQUE_REF, and with SEGVLAD_VOTE_UNIQUE_REF | SEGVLAD_VOTE_PER_IMAGE(1).  Per run 10 warm-up and 50 timed
steps: the call by wall clock between two synchronisations, and its kernels by the library's stage timer ("vote") in a second loop.
Every run is a fresh process; with --parent-lib (a build of the parent commit's library, which refuses the flag) the runs of the two
libraries alternate, and the flag-clear time is held against the parent's: the ratio of the medians next to the run-to-run spread of
each, and whether the ratio lies inside it.  The flag's own cost is reported, never asserted.

    python tools/measure_vote_unique.py [--runs 5] [--parent-lib PATH/libsegvlad_hip.so] [--out profiles/vote_unique.json]

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

from measure_vote_cap import K, N_IMG, N_TOP, SEGS, lists  # noqa: E402  (the same 200 x 50 x k = 50 lists)

FLAG = 0x80
MODES = {"plain": 0, "unique": FLAG, "unique_cap1": FLAG | (1 << 8)}


def one_run(names, warmup, steps):
    """This process: one library (SEGVLAD_LIB_PATH or the tree's), every mode of `names`."""
    import torch

    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    matches, sims, off, im = lists()
    dm, ds, di = (torch.from_numpy(x).to(eng.device) for x in (matches, sims, im))
    out = {}
    for m in names:
        mode = MODES[m]

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
        out[m] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vote_unique.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(one_run(args.child.split(","), args.warmup, args.steps)))
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
        this.append(child(",".join(MODES), None))
        if args.parent_lib:
            parent.append(child("plain", os.path.abspath(args.parent_lib)))
    import torch
    import vote_cap_ref as V
    import vote_unique_ref as U

    matches, sims, off, im = lists()
    valid = (matches >= 0) & (matches < len(im))
    b = U.blank_unique(matches, sims, off, len(im))
    b1 = V.blank(b, im, 1)

    def side(runs, name):
        return {"wall_ms": spread([r[name]["wall_ms_median"] for r in runs]),
                "stage_vote_ms": spread([r[name]["stage_vote_ms_per_call"] for r in runs]),
                "launches_per_call": runs[0][name]["launches_per_call"]}

    res = {
        "tool": "measure_vote_unique",
        "what": "segvlad_vote, base WT_BORDA_IM, device operands, NaN extrema: wall clock between synchronisations and the 'vote' stage "
                "timer; one fresh process per run, this library and the parent commit's alternating",
        "device": torch.cuda.get_device_name(0),
        "n_img": N_IMG, "segs": SEGS, "k": K, "n_top": N_TOP, "warmup": args.warmup, "steps": args.steps, "runs": args.runs, "guard": "0",
        "entries_per_image": SEGS * K, "table": "LDS" if SEGS * K <= U.LDS_ENTRIES else "global",
        "blanked_share": {"unique": round(float((b != matches).sum()) / float(valid.sum()), 4),
                          "unique_cap1": round(float((b1 != matches).sum()) / float(valid.sum()), 4)},
        "this": {name: side(this, name) for name in MODES},
    }
    t0 = res["this"]["plain"]
    for name in ("unique", "unique_cap1"):
        t = res["this"][name]
        t["stage_ratio_to_plain"] = round(t["stage_vote_ms"]["median"] / t0["stage_vote_ms"]["median"], 4)
        t["wall_ratio_to_plain"] = round(t["wall_ms"]["median"] / t0["wall_ms"]["median"], 4)
        t["stage_added_ms"] = round(t["stage_vote_ms"]["median"] - t0["stage_vote_ms"]["median"], 5)
    if parent:
        p = side(parent, "plain")
        res["parent_plain"] = p
        v = {"wall_ratio": round(t0["wall_ms"]["median"] / p["wall_ms"]["median"], 4),
             "stage_ratio": round(t0["stage_vote_ms"]["median"] / p["stage_vote_ms"]["median"], 4),
             "parent_wall_spread": round(p["wall_ms"]["max"] / p["wall_ms"]["min"], 4),
             "this_wall_spread": round(t0["wall_ms"]["max"] / t0["wall_ms"]["min"], 4),
             "parent_stage_spread": round(p["stage_vote_ms"]["max"] / p["stage_vote_ms"]["min"], 4),
             "this_stage_spread": round(t0["stage_vote_ms"]["max"] / t0["stage_vote_ms"]["min"], 4)}
        # the condition on the flag-clear call: its ratio to the parent's lies inside the larger of the two run-to-run spreads
        for kind in ("wall", "stage"):
            s = max(v[f"parent_{kind}_spread"], v[f"this_{kind}_spread"])
            v[f"{kind}_ratio_inside_spread"] = bool(1.0 / s <= v[f"{kind}_ratio"] <= s)
        res["plain_vs_parent"] = v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
