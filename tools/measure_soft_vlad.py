#!/usr/bin/env python3
"""Measurements for DESIGN.md ("Soft-assignment VLAD"): the describe stage (segvlad_describe, order 3, PCA 1024) at the benchmark's
shape -- 200 images x 50 segments, N = 1530, D = 1536, K = 64 -- operands on the device, per-stage times from segvlad_stage_ms.

  (a) vlad_assign=hard on this library and, with --parent-lib, on a build of the parent commit's (which has no such option): fresh
      processes alternating; the two medians of the WALL CLOCK must agree within the larger run-to-run spread.  The only condition
      (the stage timers are reported beside it, their first profiled call left out).
  (b) vlad_assign=soft:10, in as many fresh processes of its own: the same stages, and the soft aggregation's algorithmic rate 2 S N K D / time as a fraction of a plain
      fp32 torch.matmul of the aggregation's size measured in the same process (tools/yardstick_gemm.py's method in fp32; that tool's
      own figure, profiles/r05_yardstick_gemm.json, is an fp16 product and is quoted beside it).
  (c) the torch formulation a user would otherwise write, on the same device tensors: per image the [N][K*D] weighted token tensor and
      one GEMM with the [S][N] union.  Its time per batch and its peak memory.
Reported, never asserted: (b) against (c).  Recall under soft assignment is NOT measured: no real dataset is staged here.

    python tools/measure_soft_vlad.py [--runs 3] [--parent-lib PATH/libsegvlad_hip.so] [--out profiles/soft_vlad.json]

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

B, S, K, D, H, W, P, ORDER, TEMP = 200, 50, 64, 1536, 480, 640, 1024, 3, 10.0
N, HM, WM = (H // 14) * (W // 14), H // 2, W // 2
STAGES = ("describe", "assign", "prep", "aggregate", "pca")


def batch(dev):
    import torch

    from revisit_anything_amd import synth

    C = torch.from_numpy(synth.make_vocab(K, D, seed=1000)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    z = torch.randint(0, K, (B, N), device=dev, generator=g)
    x = torch.empty((B, D, N), device=dev)
    for b0 in range(0, B, 20):      # (in slices: the [n][N][D] noise tensor of the whole batch is 1.9 GB twice over)
        t = torch.nn.functional.normalize(C[z[b0:b0 + 20]] + 0.05 * torch.randn(20, N, D, device=dev, generator=g), dim=2)
        x[b0:b0 + 20] = t.permute(0, 2, 1)
    # rectangles of 8 .. 60 x 8 .. 80 mask pixels, as bench.py draws them
    n = B * S
    h, w = torch.randint(8, 61, (n,), device=dev, generator=g), torch.randint(8, 81, (n,), device=dev, generator=g)
    y0 = (torch.rand(n, device=dev, generator=g) * (HM - h + 1)).long().view(n, 1, 1)
    x0 = (torch.rand(n, device=dev, generator=g) * (WM - w + 1)).long().view(n, 1, 1)
    yy, xx = torch.arange(HM, device=dev).view(1, HM, 1), torch.arange(WM, device=dev).view(1, 1, WM)
    m = ((yy >= y0) & (yy < y0 + h.view(n, 1, 1)) & (xx >= x0) & (xx < x0 + w.view(n, 1, 1))).to(torch.uint8)
    return C, x, m, (np.arange(B + 1) * S).astype(np.int32)


def one_run(modes, warmup, steps):
    """This process: one library (SEGVLAD_LIB_PATH or the tree's), every mode of `modes`."""
    import torch

    os.environ["SEGVLAD_GUARD"] = "0"
    from revisit_anything_amd.engine import SegVLADEngine

    dev = torch.device("cuda:0")
    eng = SegVLADEngine(0)
    C, x, m, offs = batch(dev)
    eng.set_vocab(C)
    g = torch.Generator(device=dev)
    g.manual_seed(5000)
    comps = torch.randn(P, K * D, device=dev, generator=g) / (K * D) ** 0.5
    mean = torch.randn(K * D, device=dev, generator=g) * (0.2 / (K * D) ** 0.5)
    eng.pca_set(mean, comps, torch.logspace(-3, -6, P, device=dev), whiten=True)
    eng.set_option("pca_path", "planes")      # (one form for both modes: soft has no project form)
    out = {}
    for mode in modes:
        if mode != "hard":
            eng.set_option("vlad_assign", mode)

        def call():
            return eng.describe(m, x, offs, H, W, 14, ORDER, pca=True, l2norm=True)

        wall = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            torch.cuda.synchronize()
            if i >= warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        r = call()                  # (the first profiled call creates the stage timers' events: not counted)
        eng.synchronize()
        eng.profile_reset()
        for _ in range(steps):
            r = call()
        eng.synchronize()
        st = {s: eng.stage_ms(s) for s in STAGES}
        eng.set_profiling(False)
        out[mode] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)),
                     "stage_ms_per_call": {s: v[0] / steps for s, v in st.items()},
                     "launches_per_call": {s: v[1] / steps for s, v in st.items()}}
        if mode != "hard":
            out[mode]["torch"] = torch_formulation(C, x, r, offs)
            out[mode]["fp32_matmul"] = fp32_yardstick(dev)
    eng.close()
    return out


def torch_formulation(C, x, r, offs):
    """(c): per image w [N][K] and x^ [N][D] -> the weighted token tensor [N][K*D], one GEMM with the union [S][N], the centre term,
    intra-normalisation, L2 -- fp32 torch on the device, the union taken from the library's own incidence and adjacency."""
    import torch

    dev = x.device
    ch = torch.nn.functional.normalize(C, dim=1)
    shifts = torch.arange(64, device=dev, dtype=torch.int64)
    inc = ((r["bits"][:, :, None] >> shifts) & 1).reshape(r["bits"].shape[0], -1)[:, :N].float()
    adj = r["adj"].float()

    def image(b):
        xh = torch.nn.functional.normalize(x[b].t(), dim=1)                        # [N][D]
        w = torch.softmax(TEMP * (xh @ ch.t()), dim=1)                             # [N][K]
        U = ((adj[b * S * S:(b + 1) * S * S].reshape(S, S) @ inc[offs[b]:offs[b + 1]]) > 0).float()
        V = (U @ (w[:, :, None] * xh[:, None, :]).reshape(N, K * D)).reshape(S, K, D) - (U @ w)[:, :, None] * C[None]
        V = torch.nn.functional.normalize(V, dim=2).reshape(S, K * D)
        return torch.nn.functional.normalize(V, dim=1)

    image(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for b in range(B):
        v = image(b)
    e1.record()
    torch.cuda.synchronize()
    del v
    return {"ms_per_batch": e0.elapsed_time(e1), "peak_extra_bytes": int(torch.cuda.max_memory_allocated() - base),
            "weighted_tensor_bytes": N * K * D * 4, "what": "descriptor only (no PCA), fp32, one image at a time"}


def fp32_yardstick(dev, reps=5):
    """A plain fp32 torch.matmul of the soft aggregation's size: [B S][N] x [N][K D] per image, as one batched product"""
    import torch

    nb = 8
    a = torch.randn(nb, S, N, device=dev)
    bm = torch.randn(nb, N, K * D, device=dev)
    o = torch.empty(nb, S, K * D, device=dev)
    torch.bmm(a, bm, out=o)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.bmm(a, bm, out=o)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = sorted(ts)[len(ts) // 2]
    return {"tflops": 2.0 * nb * S * N * K * D / ms / 1e9, "ms": ms, "shape": [nb, S, N, K * D], "what": "torch.bmm fp32 (hipBLASLt / rocBLAS)"}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_vlad.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(one_run(args.child.split(","), args.warmup, args.steps)))
        return

    def child(modes, lib):
        env = dict(os.environ)
        env.pop("SEGVLAD_LIB_PATH", None)
        if lib:
            env["SEGVLAD_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", modes, "--warmup", str(args.warmup), "--steps", str(args.steps)],
                           env=env, stdout=subprocess.PIPE, timeout=280, check=True)
        line = [x for x in r.stdout.decode().splitlines() if x.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    soft = f"soft:{TEMP:g}"
    this, parent = [], []                                    # (this process opens the GPU only after its last child has ended)
    for i in range(args.runs):
        this.append(child("hard", None))
        this.append(child(soft, None))
        if args.parent_lib:
            parent.append(child("hard", os.path.abspath(args.parent_lib)))
    import torch

    def side(runs, mode):
        runs = [r for r in runs if mode in r]
        d = {"wall_ms": spread([r[mode]["wall_ms_median"] for r in runs]), "launches_per_call": runs[0][mode]["launches_per_call"]}
        d.update({f"stage_{s}_ms": spread([r[mode]["stage_ms_per_call"][s] for r in runs]) for s in STAGES})
        return d

    res = {"tool": "measure_soft_vlad",
           "what": "segvlad_describe (order 3, PCA 1024, planes form), device operands: wall clock between synchronisations and the stage "
                   "timers; one fresh process per run and mode, this library (hard, soft) and the parent commit's alternating",
           "condition": "hard_vs_parent.wall_ms.ratio_inside_spread; the stage rows are reported, not a condition",
           "device": torch.cuda.get_device_name(0), "images": B, "segments_per_image": S, "N": N, "D": D, "K": K, "P": P, "order": ORDER,
           "warmup": args.warmup, "steps": args.steps, "runs": args.runs, "guard": "0",
           "recall": "not measured: no real dataset is staged", "this_hard": side(this, "hard")}
    s = side(this, soft)
    extras = [r[soft] for r in this if soft in r]
    extra = sorted(extras, key=lambda e: e["torch"]["ms_per_batch"])[len(extras) // 2]      # the run of the median torch time
    flops = 2.0 * B * S * N * K * D
    agg_ms = s["stage_aggregate_ms"]["median"]
    s["aggregate_stage_holds"] = "soft_aggregate_kernel + soft_finalize_kernel + the fp32 -> fp16 planes split"
    s["algorithmic_flops"] = flops
    s["aggregate_tflops"] = flops / agg_ms / 1e9
    s["fp32_matmul_yardstick"] = extra["fp32_matmul"]
    s["aggregate_fraction_of_fp32_matmul"] = s["aggregate_tflops"] / extra["fp32_matmul"]["tflops"]
    s["fp16_yardstick_of_profiles_r05_tflops"] = 1076.5
    s["torch_formulation"] = extra["torch"]
    s["assign_plus_aggregate_ms"] = s["stage_assign_ms"]["median"] + agg_ms
    s["torch_over_kernel"] = extra["torch"]["ms_per_batch"] / s["assign_plus_aggregate_ms"]
    res["this_soft"] = s
    if parent:
        p, t0 = side(parent, "hard"), res["this_hard"]
        res["parent_hard"] = p
        v = {}
        for kind in ("wall_ms", "stage_describe_ms"):
            ps, ts = p[kind]["max"] / p[kind]["min"], t0[kind]["max"] / t0[kind]["min"]
            ratio = t0[kind]["median"] / p[kind]["median"]
            v[kind] = {"ratio": round(ratio, 4), "parent_spread": round(ps, 4), "this_spread": round(ts, 4),
                       "ratio_inside_spread": bool(1.0 / max(ps, ts) <= ratio <= max(ps, ts))}
        res["hard_vs_parent"] = v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
