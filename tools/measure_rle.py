#!/usr/bin/env python3
"""One measurement for DESIGN.md ("Run-length masks"): engine.incidence_rle next to engine.incidence_centroids (the dense kernel)
on the bench geometry -- 200 images x 50 blob masks of 240 x 320 at H x W = 480 x 640 -- in one process, the two calls alternating,
timed with device events around each call; and the bytes each form of the batch occupies.  Reported, never asserted.

    python tools/measure_rle.py [--reps 20] [--out profiles/rle_incidence.json]

The 10 000 masks are 500 distinct synth.make_blob_masks blobs (10 images' worth), repeated 20 times behind one another: every mask
has its own bytes / runs in memory, so neither kernel re-reads anything.  Needs a GPU; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_incidence.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_rle.py needs a GPU"
    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd import synth
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.rle import RleMasks

    B, S_img, Hm, Wm, H, W, distinct_imgs = 200, 50, 240, 320, 480, 640, 10
    part = np.concatenate([synth.make_blob_masks(S_img, Hm, Wm, seed=8800 + b) for b in range(distinct_imgs)]).astype(np.uint8)
    part_rle = RleMasks.from_dense(part)
    rep = B // distinct_imgs
    eng = SegVLADEngine(0)
    dense = torch.from_numpy(part).to(eng.device).repeat(rep, 1, 1).contiguous()
    rle = RleMasks.concat([part_rle] * rep).to(eng.device)
    S = B * S_img
    assert len(rle) == S and tuple(dense.shape) == (S, Hm, Wm)
    runs = np.diff(part_rle.run_offsets)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    t_rle, t_dense = [], []
    for i in range(args.warmup + args.reps):
        ms_r, (bits_r, cent_r) = timed(lambda: eng.incidence_rle(rle, H, W, 14))
        ms_d, (bits_d, cent_d) = timed(lambda: eng.incidence_centroids(dense, H, W, 14))
        if i >= args.warmup:
            t_rle.append(ms_r)
            t_dense.append(ms_d)
    same = bool(torch.equal(bits_r, bits_d) and torch.equal(cent_r.view(torch.int64), cent_d.view(torch.int64)))
    # the kernels alone: the library's stage timers (an event pair on the stream right around each launch), same alternation
    eng.set_profiling(True)
    eng.profile_reset()
    for _ in range(args.reps):
        eng.incidence_rle(rle, H, W, 14)
        eng.incidence_centroids(dense, H, W, 14)
    eng.synchronize()
    k_rle, n_rle = eng.stage_ms("incidence_rle")
    k_dense, n_dense = eng.stage_ms("incidence")
    eng.set_profiling(False)
    res = {
        "what": "incidence_rle vs incidence_centroids, one process, alternating calls, device events around each engine call",
        "device": torch.cuda.get_device_name(0),
        "geometry": {"images": B, "masks_per_image": S_img, "Hm": Hm, "Wm": Wm, "H": H, "W": W, "patch": 14, "distinct_masks": len(part)},
        "reps": args.reps,
        "incidence_rle_ms": {"median": float(np.median(t_rle)), "min": float(np.min(t_rle)), "max": float(np.max(t_rle))},
        "incidence_centroids_ms": {"median": float(np.median(t_dense)), "min": float(np.min(t_dense)), "max": float(np.max(t_dense))},
        "incidence_rle_kernel_ms_mean": k_rle / max(n_rle, 1),
        "incidence_fused_kernel_ms_mean": k_dense / max(n_dense, 1),
        "kernel_launches_timed": [n_rle, n_dense],
        "rle_bytes": rle.nbytes,
        "dense_bytes": int(dense.numel()),
        "dense_over_rle_bytes": float(dense.numel() / rle.nbytes),
        "runs_per_mask": {"mean": float(runs.mean()), "min": int(runs.min()), "max": int(runs.max())},
        "outputs_identical": same,
        "n_bad": int(eng.rle_n_bad.item()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
