"""A second deterministic stand-in for SAM's mask decoder, made for postprocess_small_regions (tests/sam_stub.py produces
islands but no holes, and no pair of masks that the second box NMS separates).  Prompt points -> three mask-logit maps and three
predicted IoUs per point, a pure function of (seed, point coordinates).  tools/make_regions_golden.py feeds it to the reference's
vendored SamAutomaticMaskGenerator through a stub predictor; the tests feed the same function to SamAutoMasks.

Per point:
  mask 0  a small ellipse near the point; one in four is TINY (a few pixels: its only island is smaller than min_mask_region_area,
          so the islands pass returns it unchanged but flagged, and the final area cut removes its record);
  mask 1  a medium ellipse, half of them with one to three small round HOLES;
  mask 2  a large ellipse that depends on the point's coarse CELL only (neighbouring points propose the same ellipse), half of
          them with a small SPECK far away in the image: the speck's box differs from the plain ellipse's, so the first NMS keeps
          both; once the speck is removed the boxes coincide and the second NMS drops the repaired mask.
Logits are (1 - rho) r / s with a small s: steep edges, so holes and specks survive the threshold exactly as drawn."""
import numpy as np


def _disc(xx, yy, cx, cy, r, s):
    return (1.0 - np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2) / r) * (r / s)


def stub_predict(points_xy: np.ndarray, H: int, W: int, seed: int):
    """points_xy [n, 2] (x, y) in image pixels -> (logits float32 [n, 3, H, W], ious float32 [n, 3])."""
    pts = np.asarray(points_xy, dtype=np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    side = float(min(H, W))
    cell = side / 2.0
    logits = np.empty((len(pts), 3, H, W), dtype=np.float32)
    ious = np.empty((len(pts), 3), dtype=np.float32)
    for j, (px, py) in enumerate(pts):
        rng = np.random.Generator(np.random.PCG64([int(seed), int(round(px * 4096.0)), int(round(py * 4096.0))]))
        # ---- mask 0: small, or tiny
        tiny = rng.random() < 0.25
        r = rng.uniform(1.3, 2.2) if tiny else 0.08 * side * rng.uniform(0.8, 1.4)
        asp = rng.uniform(0.8, 1.25)
        cx, cy = px + rng.uniform(-1.0, 1.0), py + rng.uniform(-1.0, 1.0)
        s = r * rng.uniform(0.002, 0.02)
        rho = np.sqrt(((xx - cx) / asp) ** 2 + ((yy - cy) * asp) ** 2) / r
        logits[j, 0] = ((1.0 - rho) * (r / s)).astype(np.float32)
        # ---- mask 1: medium, with holes
        r = 0.16 * side * rng.uniform(0.8, 1.3)
        asp = rng.uniform(0.7, 1.4)
        cx, cy = px + rng.uniform(-2.0, 2.0), py + rng.uniform(-2.0, 2.0)
        s = r * rng.uniform(0.002, 0.02)
        rho = np.sqrt(((xx - cx) / asp) ** 2 + ((yy - cy) * asp) ** 2) / r
        lg = (1.0 - rho) * (r / s)
        if rng.random() < 0.5:
            for _ in range(int(rng.integers(1, 4))):
                ang, dist, hr = rng.uniform(0, 2 * np.pi), rng.uniform(0.0, 0.45) * r, rng.uniform(0.8, 2.4)
                lg = np.minimum(lg, -_disc(xx, yy, cx + dist * np.cos(ang), cy + dist * np.sin(ang), hr, s))
        logits[j, 1] = lg.astype(np.float32)
        # ---- mask 2: the cell's large ellipse, with a far speck
        ci, cj = int(px // cell), int(py // cell)
        crng = np.random.Generator(np.random.PCG64([int(seed), 7919, ci, cj]))
        r = 0.22 * side * crng.uniform(0.9, 1.2)
        asp = crng.uniform(0.8, 1.25)
        cx, cy = (ci + 0.5) * cell + crng.uniform(-3.0, 3.0), (cj + 0.5) * cell + crng.uniform(-3.0, 3.0)
        s = r * crng.uniform(0.002, 0.01)
        rho = np.sqrt(((xx - cx) / asp) ** 2 + ((yy - cy) * asp) ** 2) / r
        lg = (1.0 - rho) * (r / s)
        if rng.random() < 0.5:
            # far: in the opposite quarter of the image, a couple of pixels inside its corner
            bx = rng.uniform(2.0, 6.0) if cx > W / 2.0 else W - 1 - rng.uniform(2.0, 6.0)
            by = rng.uniform(2.0, 6.0) if cy > H / 2.0 else H - 1 - rng.uniform(2.0, 6.0)
            lg = np.maximum(lg, _disc(xx, yy, bx, by, rng.uniform(1.0, 1.8), s))
        logits[j, 2] = lg.astype(np.float32)
        ious[j] = rng.uniform(0.78, 1.0, size=3).astype(np.float32)
    return logits, ious


# (H, W, points_per_side, points_per_batch, generator keyword arguments, seed): the cases of tests/golden/sam_generate_regions.npz
CASES = [
    (72, 96, 8, 24, {"min_mask_region_area": 30}, 9501),
    (100, 128, 9, 64, {"min_mask_region_area": 45, "box_nms_thresh": 0.5, "crop_nms_thresh": 0.8, "stability_score_thresh": 0.9}, 9502),
]


def stubbed_generator(seed: int, points_per_side: int, points_per_batch: int, kw: dict, device="cpu", output_mode="binary_mask",
                      rle_engine=None, regions_engine=None):
    """A SamAutoMasks whose network half is stub_predict (built without __init__, as the other stubbed generators of the suite)."""
    import torch

    from revisit_anything_amd import producers as pr

    class Stubbed(pr.SamAutoMasks):
        def __init__(self):
            self.device = torch.device(device)
            self.points_per_batch = points_per_batch
            self.pred_iou_thresh = kw.get("pred_iou_thresh", 0.88)
            self.stability_score_thresh = kw.get("stability_score_thresh", 0.95)
            self.stability_score_offset = kw.get("stability_score_offset", 1.0)
            self.box_nms_thresh = kw.get("box_nms_thresh", 0.7)
            self.min_mask_region_area = kw.get("min_mask_region_area", 0)
            self.mask_threshold = 0.0
            self.point_grid = pr.build_point_grid(points_per_side)
            self.output_mode = output_mode
            if "crop_nms_thresh" in kw:
                self.crop_nms_thresh = kw["crop_nms_thresh"]
            if rle_engine is not None:
                self.rle_engine = rle_engine
            if regions_engine is not None:
                self.regions_engine = regions_engine

        def _embed(self, img_rgb):
            return None

        def _predict(self, state, pts_img, out_hw):
            lg, io = stub_predict(pts_img, out_hw[0], out_hw[1], seed)
            return torch.from_numpy(lg).to(self.device), torch.from_numpy(io).to(self.device)

    return Stubbed()
