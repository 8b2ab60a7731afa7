#!/usr/bin/env python3
"""tests/golden/rle_cases.npz: what the reference's OWN run-length functions -- mask_to_rle_pytorch and rle_to_mask,
sam/segment_anything/utils/amg.py:107-149 -- make of the masks already stored in tests/golden/incidence_cases.npz.

    python tools/make_golden_rle.py --reference <checkout of the reference>

The two function bodies are executed where they lie (parsed out of the reference's file with `ast`; no source is copied).  Per
case `name` of incidence_cases.npz the fixture holds data only:
    {name}_size     int64 [2]         (Hm, Wm)
    {name}_counts   int64 [n_runs]    the "counts" lists of mask_to_rle_pytorch(masks != 0), one mask after the other
    {name}_offsets  int64 [S + 1]     where each mask's counts start
    {name}_dense    uint8             np.packbits of rle_to_mask(record) per mask, [S, Hm, ceil(Wm / 8)]
tests/test_rle_host.py holds RleMasks.from_dense to the counts and RleMasks.from_sam(...).to_dense() to the masks."""
import argparse
import ast
import os
from typing import Any, Dict, List

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_amg(reference: str):
    path = os.path.join(reference, "sam", "segment_anything", "utils", "amg.py")
    want = {"mask_to_rle_pytorch", "rle_to_mask"}
    body = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert {n.name for n in body} == want, want - {n.name for n in body}
    ns = dict(np=np, torch=torch, Any=Any, Dict=Dict, List=List)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["mask_to_rle_pytorch"], ns["rle_to_mask"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    to_rle, to_mask = load_amg(args.reference)
    z = np.load(os.path.join(GOLDEN, "incidence_cases.npz"))
    out = {}
    names = sorted(k[:-len("_masks")] for k in z.files if k.endswith("_masks"))
    for name in names:
        S, Hm, Wm = (int(v) for v in z[name + "_shape"][:3])
        masks = np.unpackbits(z[name + "_masks"], axis=1)[:, :Hm * Wm].reshape(S, Hm, Wm) != 0   # (stored bit-packed per mask)
        recs = to_rle(torch.from_numpy(masks))
        assert all(r["size"] == [Hm, Wm] for r in recs)
        out[name + "_size"] = np.array([Hm, Wm], np.int64)
        out[name + "_counts"] = np.concatenate([np.asarray(r["counts"], np.int64) for r in recs])
        out[name + "_offsets"] = np.concatenate([[0], np.cumsum([len(r["counts"]) for r in recs])]).astype(np.int64)
        dense = np.stack([to_mask(r) for r in recs])
        assert dense.shape == masks.shape and np.array_equal(dense, masks), name   # (the reference's own round trip)
        out[name + "_dense"] = np.packbits(dense, axis=-1)
    path = os.path.join(GOLDEN, "rle_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
