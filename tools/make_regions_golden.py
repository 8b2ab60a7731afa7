#!/usr/bin/env python3
"""Golden vectors for small-region removal, from the REFERENCE's own function bodies (needs the reference checkout; the outputs
are committed under tests/golden/ as data -- no reference source is copied, the functions are executed where they lie):

  tests/golden/regions_cases.npz          utils/amg.py remove_small_regions, both modes, on masks of tests/regions_ref.py
  tests/golden/sam_generate_regions.npz   SamAutomaticMaskGenerator.generate with min_mask_region_area > 0 (generate ->
                                          postprocess_small_regions) on the stub predictor of tests/regions_stub.py

WHAT THESE PIN.  OpenCV is not installed here, so the reference is handed a `cv2` stand-in whose
connectedComponentsWithStats(img, 8) is scipy.ndimage.label (3 x 3 structure) plus a bincount; torchvision's batched_nms is
make_golden.py's restatement.  The fixtures therefore pin the reference's FLOW: the complement, the strict threshold, the fill
lists, keep-largest, the changed flag, the scoring, the second NMS, which runs and boxes are refreshed, the reordering and the
final area cut.  They do NOT pin OpenCV's labeller (its numbering decides a tie for the largest component)."""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import regions_ref as RR  # noqa: E402
import regions_stub  # noqa: E402
from make_golden import REF, torchvision_nms  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASE_SHAPES = [(33, 65), (64, 64)]
CASE_MIN_AREAS = [1, 2, 3, RR.PLANTED, RR.PLANTED + 1, RR.HOLE, RR.HOLE + 1, 40, 64 * 65 + 1]


def cv2_stand_in():
    """the one function remove_small_regions calls: (n_labels, labels, stats with the area in the last column, centroids)"""
    def connectedComponentsWithStats(img, connectivity):
        assert connectivity == 8 and img.dtype == np.uint8
        lab, n = ndimage.label(img, structure=np.ones((3, 3), dtype=np.uint8))
        stats = np.zeros((n + 1, 5), dtype=np.int32)
        stats[:, -1] = np.bincount(lab.ravel(), minlength=n + 1)
        return n + 1, lab.astype(np.int32), stats, None

    mod = types.ModuleType("cv2")
    mod.connectedComponentsWithStats = connectedComponentsWithStats
    return mod


def load_amg():
    sys.modules["cv2"] = cv2_stand_in()
    spec = importlib.util.spec_from_file_location("ref_amg", f"{REF}/sam/segment_anything/utils/amg.py")
    amg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(amg)
    return amg


def gen_cases(amg):
    out = {"shapes": np.array(CASE_SHAPES), "min_areas": np.array(CASE_MIN_AREAS)}
    for (H, W) in CASE_SHAPES:
        names, masks = RR.table(H, W)
        tag = f"{H}x{W}"
        out[f"{tag}_names"] = np.array(names)
        out[f"{tag}_masks"] = np.packbits(masks != 0, axis=-1)
        seen = set()
        for a in CASE_MIN_AREAS:
            res, chg = [], []
            for m in masks:
                b = m != 0
                h, c0 = amg.remove_small_regions(b, a, mode="holes")
                i, c1 = amg.remove_small_regions(h, a, mode="islands")
                res.append(np.stack([h, i]))
                chg.append([c0, c1])
                seen.add((bool(c0), bool(c1)))
            out[f"{tag}_a{a}_out"] = np.packbits(np.stack(res), axis=-1)          # [S, 2, H, W/8]: after holes, after islands
            out[f"{tag}_a{a}_changed"] = np.array(chg, dtype=bool)
        assert len(seen) == 4, seen
    np.savez_compressed(f"{OUT}/regions_cases.npz", **out)
    print("regions_cases.npz", os.path.getsize(f"{OUT}/regions_cases.npz"), "bytes")


def gen_generate(amg):
    from typing import Any, Dict, List, Optional, Tuple

    class StubPredictor:   # the five members the generator touches
        def __init__(self, model):
            self.model = model
            self.device = "cpu"
            self.transform = types.SimpleNamespace(apply_coords=lambda pts, im_size: np.asarray(pts, dtype=np.float64))
            self.im = None

        def set_image(self, im):
            self.im = im.shape[:2]

        def reset_image(self):
            self.im = None

        def predict_torch(self, pts, labels, multimask_output, return_logits):
            assert multimask_output and return_logits and pts.shape[1] == 1 and bool((labels == 1).all())
            lg, io = regions_stub.stub_predict(pts[:, 0, :].numpy(), self.im[0], self.im[1], self.model.seed)
            return torch.from_numpy(lg), torch.from_numpy(io), None

    log = {}

    def spy_remove(mask, area_thresh, mode):
        res, changed = amg.remove_small_regions(mask, area_thresh, mode)
        log["clean"].append((mode, np.array(mask, dtype=bool), np.array(res, dtype=bool), bool(changed)))
        return res, changed

    def spy_nms(boxes, scores, idxs, iou_threshold):
        keep = torchvision_nms(boxes, scores, iou_threshold)
        log["nms"].append((len(boxes), keep.tolist(), float(iou_threshold)))
        return keep

    ns = {k: getattr(amg, k) for k in dir(amg) if not k.startswith("__")}
    ns.update(np=np, torch=torch, Any=Any, Dict=Dict, List=List, Optional=Optional, Tuple=Tuple, Sam=object, SamPredictor=StubPredictor,
              batched_nms=spy_nms, remove_small_regions=spy_remove, box_area=lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    path = f"{REF}/sam/segment_anything/automatic_mask_generator.py"
    body = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "SamAutomaticMaskGenerator"]
    assert len(body) == 1
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    out = {"n_cases": np.array(len(regions_stub.CASES))}
    for c, (H, W, pps, ppb, kw, seed) in enumerate(regions_stub.CASES):
        log.update(clean=[], nms=[])
        model = types.SimpleNamespace(mask_threshold=0.0, seed=seed)
        gen = ns["SamAutomaticMaskGenerator"](model, points_per_side=pps, points_per_batch=ppb, **kw)
        recs = gen.generate(np.zeros((H, W, 3), dtype=np.uint8))
        # ---- what the fixture must show (the issue's list) ----
        holes = [e for e in log["clean"] if e[0] == "holes"]
        isl = [e for e in log["clean"] if e[0] == "islands"]
        n_first, (n_in, keep2, thr2) = log["nms"][0], log["nms"][1]
        assert len(log["nms"]) == 2 and len(holes) == len(isl) == n_in
        assert thr2 == max(kw.get("box_nms_thresh", 0.7), kw.get("crop_nms_thresh", 0.7))
        n_filled = sum(1 for e in holes if e[3] and (e[1] != e[2]).any())
        n_stripped = sum(1 for e in isl if e[3] and (e[1] != e[2]).any())
        n_flag_only = sum(1 for h, i in zip(holes, isl) if (h[3] or i[3]) and not (h[1] != i[2]).any())
        assert n_filled >= 1, "no hole-filled mask"
        assert n_stripped >= 1, "no island-stripped mask"
        assert n_flag_only >= 1, "no mask flagged changed but identical"
        assert len(keep2) < n_in, "the second NMS dropped nothing"
        assert keep2 != sorted(keep2), "the output order is the input order"
        assert len(recs) < len(keep2), "the final area cut removed nothing"
        assert len(recs) >= 3
        print(f"sam_generate_regions case {c}: first NMS kept {n_in} of {n_first[0]}, {n_filled} filled, {n_stripped} stripped, "
              f"{n_flag_only} flagged only, second NMS kept {len(keep2)}, {len(recs)} records")
        out[f"c{c}_args"] = np.array([H, W, pps, ppb, seed], dtype=np.int64)
        out[f"c{c}_seg"] = np.packbits(np.stack([r["segmentation"] for r in recs]), axis=-1)
        out[f"c{c}_area"] = np.array([r["area"] for r in recs], dtype=np.int64)
        out[f"c{c}_bbox"] = np.array([r["bbox"] for r in recs], dtype=np.int64)
        out[f"c{c}_iou"] = np.array([r["predicted_iou"] for r in recs], dtype=np.float64)
        out[f"c{c}_pts"] = np.array([r["point_coords"][0] for r in recs], dtype=np.float64)
        out[f"c{c}_stab"] = np.array([r["stability_score"] for r in recs], dtype=np.float64)
        out[f"c{c}_crop"] = np.array([r["crop_box"] for r in recs], dtype=np.int64)
    np.savez_compressed(f"{OUT}/sam_generate_regions.npz", **out)
    print("sam_generate_regions.npz", os.path.getsize(f"{OUT}/sam_generate_regions.npz"), "bytes")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    amg = load_amg()
    gen_cases(amg)
    gen_generate(amg)
