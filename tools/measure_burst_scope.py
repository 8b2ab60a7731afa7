#!/usr/bin/env python3
"""Measurements for DESIGN.md ("Burst discount over a segment's own tokens"): tools/measure_burst.py's describe call (segvlad_describe,
order 3, PCA 1024, planes form, 200 images x 50 segments, N = 1530, D = 1536, K = 64, operands on the device) under four settings,

    hard | hard + vlad_burst=8:7:1 (image scope) | hard + vlad_burst=8:7:1, vlad_burst_scope=segment | soft:10 + the same

in one session: every run takes the four settings in turn, each in a fresh process, so that the image scope -- the parent commit's
unchanged path -- and the segment scope alternate.  Printed per setting: the describe wall clock between synchronisations and the
"burst" and "aggregate" stage times of segvlad_stage_ms (medians over the runs, min .. max beside them); then the ratios DESIGN.md
quotes and the Gram kernel's share of the fp32-MFMA peak (157 TF).  Under segment scope the kernel runs the full square of 128 x 128
tiles once per 64 segments: its MFMA work is 2 (128 T)^2 D per image and chunk, T = ceil(N / 128), plus the mask product's
2 (128 T)^2 64.  Reported, never asserted.

    python tools/measure_burst_scope.py [--runs 3] [--images 200] [--out profiles/burst_scope.txt]

Needs a GPU; there is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_burst as MB  # noqa: E402

SETTINGS = (("hard", "hard", None), ("hard + burst (image)", "hard+burst", "image"), ("hard + burst (segment)", "hard+burst", "segment"),
            (f"soft:{MB.TEMP:g} + burst (segment)", f"soft:{MB.TEMP:g}+burst", "segment"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burst_scope.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-scope", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    B = args.images
    if args.child is not None:
        print("RESULT " + json.dumps(MB.one_run(args.child, B, args.warmup, args.steps, args.child_scope or None)))
        return

    def child(mode, scope):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--child-scope", scope or "", "--images", str(B),
                            "--warmup", str(args.warmup), "--steps", str(args.steps)], stdout=subprocess.PIPE, timeout=280, check=True)
        line = [x for x in r.stdout.decode().splitlines() if x.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    runs = {name: [] for name, _, _ in SETTINGS}
    for _ in range(args.runs):
        for name, mode, scope in SETTINGS:
            runs[name].append(child(mode, scope))

    def med(name, key, stage=None):
        v = [r[key] if stage is None else r[key][stage] for r in runs[name]]
        return float(np.median(v)), float(np.min(v)), float(np.max(v))

    lines = [f"segvlad_describe, {B} images x {MB.S} segments, N {MB.N}, D {MB.D}, K {MB.K}, order {MB.ORDER}, PCA {MB.P} (planes form), "
             f"vlad_burst={MB.BURST}; {args.runs} runs of {args.steps} calls after {args.warmup} warm-up calls, a fresh process per run and setting, "
             f"the four settings in turn; ms per call, median (min .. max)",
             f"{'setting':>28}  {'describe wall':>26}  {'burst stage':>26}  {'aggregate stage':>26}  launches burst / aggregate"]
    m = {}
    for name, _, _ in SETTINGS:
        wall, burst, agg = med(name, "wall_ms_median"), med(name, "stage_ms_per_call", "burst"), med(name, "stage_ms_per_call", "aggregate")
        m[name] = (wall[0], burst[0], agg[0])
        ln = runs[name][0]["launches_per_call"]
        lines.append(f"{name:>28}  " + "  ".join(f"{v[0]:9.3f} ({v[1]:6.3f} .. {v[2]:6.3f})" for v in (wall, burst, agg)) +
                     f"  {ln['burst']:g} / {ln['aggregate']:g}")
    hard, img, seg, soft = (m[name] for name, _, _ in SETTINGS)
    T = (MB.N + 127) // 128
    chunks = (MB.S + 63) // 64
    work = B * chunks * (2.0 * (128 * T) ** 2 * MB.D + 2.0 * (128 * T) ** 2 * 64)
    tf = work / seg[1] / 1e9 if seg[1] > 0 else 0.0
    lines += ["",
              f"describe wall, hard + burst: segment / image = {seg[0] / img[0]:.3f}",
              f"burst stage, segment / image = {seg[1] / img[1]:.3f} (the arithmetic predicts 2.08: twice the Gram flops + 4 % for the mask product)",
              f"aggregate stage, hard + burst (segment) / plain hard = {seg[2] / hard[2]:.3f}; / hard + burst (image) = {seg[2] / img[2]:.3f}",
              f"Gram kernel under segment scope: {work / 1e12:.3f} TFLOP of MFMA work per call in {seg[1]:.3f} ms = {tf:.1f} TFLOP/s, "
              f"{tf / MB.PEAK_TF:.3f} of the fp32-MFMA peak ({MB.PEAK_TF:g} TF); the stage holds that kernel alone",
              "not measured: hardware counters, recall"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
