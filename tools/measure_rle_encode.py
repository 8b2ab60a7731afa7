#!/usr/bin/env python3
"""One measurement for DESIGN.md ("Run-length masks", Encoding): engine.rle_encode on dense device masks next to the host path it
replaces -- masks.cpu() + RleMasks.from_dense -- on tools/measure_rle.py's batch: 200 images x 50 blob masks of 240 x 320 on the
device.  One process, the two alternating; the device call timed with device events around it (it ends with its one wait for the
total), the host path by wall clock.  Times, the bytes each path moves to the host, and whether the results are equal.  Reported,
never asserted.

    python tools/measure_rle_encode.py [--reps 5] [--out profiles/rle_encode.json]

The device call is timed twice per round: with the default capacity S * (2 Wm + 2) -- these ragged synthetic blobs have more runs
than that, so the call is repeated with the total -- and with the capacity a caller who knows the total would pass (one call).
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_encode.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_rle_encode.py needs a GPU"
    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd import synth
    from revisit_anything_amd.engine import SegVLADEngine
    from revisit_anything_amd.rle import RleMasks

    B, S_img, Hm, Wm, distinct_imgs = 200, 50, 240, 320, 10
    part = np.concatenate([synth.make_blob_masks(S_img, Hm, Wm, seed=8800 + b) for b in range(distinct_imgs)]).astype(np.uint8)
    eng = SegVLADEngine(0)
    dense = torch.from_numpy(part).to(eng.device).repeat(B // distinct_imgs, 1, 1).contiguous()
    S = B * S_img
    assert tuple(dense.shape) == (S, Hm, Wm)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    t_default, t_known, t_host, t_copy = [], [], [], []
    total = None
    for i in range(args.warmup + args.reps):
        ms_a, (dev_rle, dev_areas) = timed(lambda: eng.rle_encode(dense, want_area=True))
        retried = bool(eng.rle_encode_retried)
        total = int(dev_rle.counts.shape[0])
        ms_b, _ = timed(lambda: eng.rle_encode(dense, want_area=True, capacity=total))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_host = dense.cpu()
        t1 = time.perf_counter()
        host_rle = RleMasks.from_dense(on_host)
        t2 = time.perf_counter()
        if i >= args.warmup:
            t_default.append(ms_a)
            t_known.append(ms_b)
            t_host.append((t2 - t0) * 1e3)
            t_copy.append((t1 - t0) * 1e3)
    same = bool(dev_rle == host_rle and np.array_equal(dev_areas.cpu().numpy(), host_rle.areas()))
    # the kernels alone: the library's stage timers (an event pair on the stream right around the launches of one call)
    eng.set_profiling(True)
    eng.profile_reset()
    for _ in range(args.reps):
        eng.rle_encode(dense, want_area=True, capacity=total)
    eng.synchronize()
    k_ms, n_launch = eng.stage_ms("rle_encode")
    eng.set_profiling(False)
    runs = np.diff(host_rle.run_offsets[:len(part) + 1])

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    res = {
        "what": "engine.rle_encode (device events around the call) vs masks.cpu() + RleMasks.from_dense (wall clock), one process, alternating",
        "device": torch.cuda.get_device_name(0),
        "geometry": {"images": B, "masks_per_image": S_img, "Hm": Hm, "Wm": Wm, "distinct_masks": len(part)},
        "reps": args.reps,
        "rle_encode_default_capacity_ms": stats(t_default),
        "default_capacity_slots": S * (2 * Wm + 2),
        "default_capacity_call_repeated": retried,
        "rle_encode_known_capacity_ms": stats(t_known),
        "rle_encode_kernels_ms_mean_per_call": k_ms / max(args.reps, 1),
        "kernel_launches_per_call": n_launch / max(args.reps, 1),
        "host_path_ms": stats(t_host),
        "host_path_copy_ms": stats(t_copy),
        "total_runs": total,
        "runs_per_mask": {"mean": float(runs.mean()), "min": int(runs.min()), "max": int(runs.max())},
        "mask_bytes_read_per_pass": int(dense.numel()),
        "device_path_bytes_to_host": 8,                               # the total; the runs stay on the device
        "device_path_bytes_to_host_if_the_runs_are_fetched": dev_rle.nbytes + 8 * S,
        "host_path_bytes_to_host": int(dense.numel()),
        "results_equal": same,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
