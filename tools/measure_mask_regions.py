#!/usr/bin/env python3
"""One measurement for DESIGN.md ("Run-length masks", Small regions): engine.mask_regions on dense device masks next to the host
path it replaces -- masks.cpu() + producers.clean_small_regions (scipy.ndimage.label, twice per mask) -- on 100 masks of the stub
decoder (tests/regions_stub.py: ellipses with holes and far specks) at 240 x 320 and at 480 x 640.  One process, device and host
alternating; the device call by wall clock between two synchronisations and its kernels by the library's stage timer, the host
path by wall clock including the copy it needs.  Median and spread, and whether the results are equal.  Reported, never asserted.

    python tools/measure_mask_regions.py [--reps 7] [--min-area 100] [--out profiles/mask_regions.json]

Needs a GPU; there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stub_masks(n, H, W, seed):
    from regions_stub import stub_predict

    side = int(np.ceil(np.sqrt(n / 3.0)))
    c = (np.arange(side) + 0.5) / side
    gx, gy = np.meshgrid(c * W, c * H)
    pts = np.column_stack([gx.ravel(), gy.ravel()])
    out = []
    for p0 in range(0, len(pts), 8):
        lg, _ = stub_predict(pts[p0:p0 + 8], H, W, seed)
        out.append(lg.reshape(-1, H, W) > 0)
    return np.concatenate(out)[:n]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-area", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_regions.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_mask_regions.py needs a GPU"
    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd import producers as pr
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    res = {
        "what": "engine.mask_regions (wall clock between synchronisations; kernels by stage timer) vs masks.cpu() + "
                "producers.clean_small_regions (wall clock), one process, alternating",
        "device": torch.cuda.get_device_name(0),
        "reps": args.reps,
        "min_area": args.min_area,
        "shapes": [],
    }
    for (Hm, Wm) in ((240, 320), (480, 640)):
        S = 100
        m = stub_masks(S, Hm, Wm, 9600 + Hm)
        dense = torch.from_numpy(m).to(eng.device)
        t_dev, t_host, t_copy = [], [], []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.mask_regions(dense, args.min_area)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            on_host = dense.cpu().numpy()
            t2 = time.perf_counter()
            cleaned, changed = pr.clean_small_regions(on_host, args.min_area)
            t3 = time.perf_counter()
            if i >= args.warmup:
                t_dev.append((t1 - t0) * 1e3)
                t_host.append((t3 - t1) * 1e3)
                t_copy.append((t2 - t1) * 1e3)
        same = bool(np.array_equal(out["masks"].cpu().numpy() != 0, cleaned) and np.array_equal(out["changed"].cpu().numpy(), changed)
                    and np.array_equal(out["boxes"].cpu().numpy(), pr.mask_boxes(torch.from_numpy(cleaned)).numpy())
                    and np.array_equal(out["area"].cpu().numpy(), cleaned.reshape(S, -1).sum(1)))
        eng.set_profiling(True)
        eng.profile_reset()
        for _ in range(args.reps):
            eng.mask_regions(dense, args.min_area)
        eng.synchronize()
        k_ms, n_launch = eng.stage_ms("mask_regions")
        eng.set_profiling(False)
        res["shapes"].append({
            "masks": S, "Hm": Hm, "Wm": Wm,
            "mask_regions_call_ms": stats(t_dev),
            "mask_regions_kernels_ms_mean_per_call": k_ms / max(args.reps, 1),
            "kernel_launches_per_call": n_launch / max(args.reps, 1),
            "host_path_ms": stats(t_host),
            "host_path_copy_ms": stats(t_copy),
            "masks_changed": int((changed != 0).sum()),
            "scratch_bytes": 8 * S * Hm * Wm,
            "device_path_bytes_to_host": 0,
            "host_path_bytes_to_host": int(dense.numel()),
            "results_equal": same,
        })
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
