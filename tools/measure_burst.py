#!/usr/bin/env python3
"""Measurements for DESIGN.md ("Burst-discounted VLAD"): the describe stage (segvlad_describe, order 3, PCA 1024, planes form) at the
benchmark's shape -- 200 images x 50 segments, N = 1530, D = 1536, K = 64 -- and for one image, operands on the device, per-stage
times from segvlad_stage_ms.

  modes   hard | hard + vlad_burst=8:7:1 | soft:10 | soft:10 + vlad_burst=8:7:1, every mode in a fresh process of its own
  stages  describe (the whole call as the stream sees it), assign, prep, burst (burst_gram_kernel + burst_finish_kernel),
          aggregate, pca; the wall clock between synchronisations beside them
  rate    the Gram kernel's algorithmic rate B N^2 D 2 / time of the "burst" stage, against the fp32-MFMA peak (157 TF); the kernel
          runs the upper triangle of tiles only, so the MFMA work is about half of that
  parent  with --parent-lib, the same call on a build of the parent commit's library (which has no such option): the describe
          time the option-off path has to match

Reported, never asserted.  Recall under the discount is NOT measured: no real dataset is staged here.

    python tools/measure_burst.py [--runs 3] [--parent-lib PATH/libsegvlad_hip.so] [--out profiles/burst.json]

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

S, K, D, H, W, P, ORDER, TEMP = 50, 64, 1536, 480, 640, 1024, 3, 10.0
BURST = "8:7:1"
N, HM, WM = (H // 14) * (W // 14), H // 2, W // 2
STAGES = ("describe", "assign", "prep", "burst", "aggregate", "pca")
MODES = ("hard", "hard+burst", f"soft:{TEMP:g}", f"soft:{TEMP:g}+burst")
PEAK_TF = 157.0


def batch(dev, B):
    import torch

    from revisit_anything_amd import synth

    C = torch.from_numpy(synth.make_vocab(K, D, seed=1000)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    z = torch.randint(0, K, (B, N), device=dev, generator=g)
    x = torch.empty((B, D, N), device=dev)
    step = min(B, 20)
    for b0 in range(0, B, step):      # (in slices: the noise tensor of the whole batch is 1.9 GB twice over)
        t = torch.nn.functional.normalize(C[z[b0:b0 + step]] + 0.05 * torch.randn(step, N, D, device=dev, generator=g), dim=2)
        x[b0:b0 + step] = t.permute(0, 2, 1)
    n = B * S
    h, w = torch.randint(8, 61, (n,), device=dev, generator=g), torch.randint(8, 81, (n,), device=dev, generator=g)
    y0 = (torch.rand(n, device=dev, generator=g) * (HM - h + 1)).long().view(n, 1, 1)
    x0 = (torch.rand(n, device=dev, generator=g) * (WM - w + 1)).long().view(n, 1, 1)
    yy, xx = torch.arange(HM, device=dev).view(1, HM, 1), torch.arange(WM, device=dev).view(1, 1, WM)
    m = ((yy >= y0) & (yy < y0 + h.view(n, 1, 1)) & (xx >= x0) & (xx < x0 + w.view(n, 1, 1))).to(torch.uint8)
    return C, x, m, (np.arange(B + 1) * S).astype(np.int32)


def one_run(mode, B, warmup, steps, scope=None):
    """This process: one library (SEGVLAD_LIB_PATH or the tree's), one mode, one batch size; scope: the option vlad_burst_scope
    (tools/measure_burst_scope.py), None leaves the default."""
    import torch

    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd._lib import SegVLADError
    from revisit_anything_amd.engine import SegVLADEngine

    dev = torch.device("cuda:0")
    eng = SegVLADEngine(0)
    C, x, m, offs = batch(dev, B)
    eng.set_vocab(C)
    g = torch.Generator(device=dev)
    g.manual_seed(5000)
    comps = torch.randn(P, K * D, device=dev, generator=g) / (K * D) ** 0.5
    mean = torch.randn(K * D, device=dev, generator=g) * (0.2 / (K * D) ** 0.5)
    eng.pca_set(mean, comps, torch.logspace(-3, -6, P, device=dev), whiten=True)
    eng.set_option("pca_path", "planes")      # (one form for every mode: the weighted paths have no project form)
    assign, _, burst = mode.partition("+")
    if assign != "hard":
        eng.set_option("vlad_assign", assign)
    if burst:
        eng.set_option("vlad_burst", BURST)
    if scope:
        eng.set_option("vlad_burst_scope", scope)

    def call():
        return eng.describe(m, x, offs, H, W, 14, ORDER, pca=True, l2norm=True)

    wall = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_profiling(True)
    call()                      # (the first profiled call creates the stage timers' events: not counted)
    eng.synchronize()
    eng.profile_reset()
    for _ in range(steps):
        call()
    eng.synchronize()
    st = {}
    for s in STAGES:
        try:
            st[s] = eng.stage_ms(s)
        except SegVLADError:    # a stage this mode does not run
            st[s] = (0.0, 0)
    eng.set_profiling(False)
    eng.close()
    return {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)),
            "stage_ms_per_call": {s: v[0] / steps for s, v in st.items()}, "launches_per_call": {s: v[1] / steps for s, v in st.items()}}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--images", type=int, nargs="+", default=[200, 1])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burst.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-images", type=int, default=200, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(one_run(args.child, args.child_images, args.warmup, args.steps)))
        return

    def child(mode, B, lib):
        env = dict(os.environ)
        env.pop("SEGVLAD_LIB_PATH", None)
        if lib:
            env["SEGVLAD_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--child-images", str(B), "--warmup", str(args.warmup),
                            "--steps", str(args.steps)], env=env, stdout=subprocess.PIPE, timeout=280, check=True)
        line = [x for x in r.stdout.decode().splitlines() if x.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    def side(runs):
        d = {"wall_ms": spread([r["wall_ms_median"] for r in runs]), "launches_per_call": runs[0]["launches_per_call"]}
        d.update({f"stage_{s}_ms": spread([r["stage_ms_per_call"][s] for r in runs]) for s in STAGES})
        return d

    res = {"tool": "measure_burst",
           "what": "segvlad_describe (order 3, PCA 1024, planes form), device operands: wall clock between synchronisations and the stage "
                   "timers; one fresh process per run, mode and batch size (this process opens no GPU)",
           "segments_per_image": S, "N": N, "D": D, "K": K, "P": P, "order": ORDER, "vlad_burst": BURST, "warmup": args.warmup,
           "steps": args.steps, "runs": args.runs, "guard": "0", "recall": "not measured: no real dataset is staged", "images": {}}
    for B in args.images:
        runs = {mode: [] for mode in MODES}
        parent = []
        for _ in range(args.runs):
            for mode in MODES:
                runs[mode].append(child(mode, B, None))
            if args.parent_lib:
                parent.append(child("hard", B, os.path.abspath(args.parent_lib)))
        entry = {mode: side(r) for mode, r in runs.items()}
        if parent:
            entry["parent_hard"] = side(parent)
        for mode in MODES:
            if mode.endswith("+burst"):
                ms = entry[mode]["stage_burst_ms"]["median"]
                tf = 2.0 * B * N * N * D / ms / 1e9 if ms > 0 else 0.0
                entry[mode]["burst_algorithmic_tflops"] = tf
                entry[mode]["burst_fraction_of_fp32_mfma_peak"] = tf / PEAK_TF
        res["images"][str(B)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    print()
    for B, entry in res["images"].items():
        print(f"B = {B}:  " + "  ".join(f"{s:>9}" for s in ("wall",) + STAGES))
        for mode, e in entry.items():
            print(f"  {mode:>16}  " + "  ".join(f"{e[k]['median']:9.3f}" for k in ["wall_ms"] + [f"stage_{s}_ms" for s in STAGES]))


if __name__ == "__main__":
    main()
