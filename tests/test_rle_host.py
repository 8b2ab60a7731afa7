"""Run-length masks on the host (revisit_anything_amd/rle.py, and their users store.py / producers.py): the encoder against the
reference's own mask_to_rle_pytorch / rle_to_mask (tests/golden/rle_cases.npz, tools/make_golden_rle.py), the invariants of SAM's
convention over the mask branch's shape table, validation, the store's two formats and the producer's output mode.  No GPU; every
comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_branch_cases as T  # noqa: E402

from revisit_anything_amd import store as st  # noqa: E402
from revisit_anything_amd.rle import RLE_CHUNK_RUNS, RleMasks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = ("same", "x2", "x2clip", "nonint", "down")


# ---- the shape table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.INC_NAMES)
def test_round_trip_over_the_shape_table(name):
    m = T.build_masks(name)[0]
    r = RleMasks.from_dense(m)
    assert len(r) == len(m) and (r.Hm, r.Wm) == m.shape[1:] and r.counts.dtype == np.uint32 and r.run_offsets.dtype == np.int64
    d = r.to_dense()
    assert d.dtype == bool and d.shape == m.shape and np.array_equal(d, m != 0)


@pytest.mark.parametrize("name", T.INC_NAMES)
def test_invariants_of_sams_convention(name):
    m, where = T.build_masks(name)
    r = RleMasks.from_dense(m)
    c, o = r.arrays()
    P = r.Hm * r.Wm
    assert o[0] == 0 and o[-1] == len(c) and (np.diff(o) >= 0).all() and len(o) == len(m) + 1
    for s in range(len(m)):
        runs = c[o[s]:o[s + 1]]
        assert int(runs.astype(np.int64).sum()) == P, (name, s)
        assert (runs[1:] > 0).all(), (name, s)          # only the first count may be 0 in the encoder's output
    if "zeros" in where:
        s = where["zeros"]
        assert c[o[s]:o[s + 1]].tolist() == [P]
        s = where["ones"]
        assert c[o[s]:o[s + 1]].tolist() == [0, P]
        s = where["corner0"]
        assert c[o[s]:o[s + 1]].tolist() == [0, 1, P - 1]
        s = where["corner3"]
        assert c[o[s]:o[s + 1]].tolist() == [P - 1, 1]
        s = where["corner2"]                             # (Hm - 1, 0): the last pixel of the first COLUMN
        assert c[o[s]:o[s + 1]].tolist() == [r.Hm - 1, 1, P - r.Hm]


def test_one_mask_and_no_mask():
    r = RleMasks.from_dense(np.eye(3, 4, dtype=np.uint8) * 200)
    assert len(r) == 1 and np.array_equal(r.to_dense()[0], np.eye(3, 4) != 0)
    e = RleMasks.from_dense(np.zeros((0, 5, 6), np.uint8))
    assert len(e) == 0 and e.to_dense().shape == (0, 5, 6) and e.run_offsets.tolist() == [0] and e.nbytes == 8
    with pytest.raises(ValueError):
        RleMasks.from_dense(np.zeros((2, 3, 4, 5)))


def test_concat_to_and_equality():
    import torch

    a, b = (RleMasks.from_dense(np.array(T.build_masks(n)[0])) for n in ("fused_ranges_small", "s1"))
    ab = RleMasks.concat([a, b])
    assert len(ab) == len(a) + len(b)
    assert np.array_equal(ab.to_dense(), np.concatenate([a.to_dense(), b.to_dense()]))
    assert ab == RleMasks.from_dense(np.concatenate([T.build_masks("fused_ranges_small")[0], T.build_masks("s1")[0]]))
    assert ab != a and RleMasks.concat([a]) == a
    with pytest.raises(ValueError):
        RleMasks.concat([a, RleMasks.from_dense(np.zeros((1, 8, 8)))])
    with pytest.raises(ValueError):
        RleMasks.concat([])
    t = ab.to("cpu")
    assert isinstance(t.counts, torch.Tensor) and t.counts.dtype == torch.uint32 and t.run_offsets.dtype == torch.int64
    assert t == ab and len(t) == len(ab) and np.array_equal(t.to_dense(), ab.to_dense()) and t.nbytes == ab.nbytes


# ---- the reference's functions -------------------------------------------------------------------------------------------------
def _golden_masks(golden_dir, name):
    zi = np.load(os.path.join(golden_dir, "incidence_cases.npz"))
    S, Hm, Wm = (int(v) for v in zi[name + "_shape"][:3])
    return np.unpackbits(zi[name + "_masks"], axis=1)[:, :Hm * Wm].reshape(S, Hm, Wm)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_from_dense_emits_the_references_counts(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "rle_cases.npz"))
    r = RleMasks.from_dense(_golden_masks(golden_dir, name))
    assert r.size == z[name + "_size"].tolist()
    assert np.array_equal(r.run_offsets, z[name + "_offsets"]) and np.array_equal(r.counts, z[name + "_counts"])


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_from_sam_decodes_to_the_references_masks(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "rle_cases.npz"))
    Hm, Wm = (int(v) for v in z[name + "_size"])
    c, o = z[name + "_counts"], z[name + "_offsets"]
    recs = [{"size": [Hm, Wm], "counts": c[o[s]:o[s + 1]].tolist()} for s in range(len(o) - 1)]
    want = np.unpackbits(z[name + "_dense"], axis=-1)[..., :Wm].astype(bool)
    for records in (recs, [{"segmentation": r, "area": 1} for r in recs]):
        r = RleMasks.from_sam(records)
        assert np.array_equal(r.to_dense(), want)
        assert all(np.array_equal(r.mask(j), want[j]) for j in range(len(r)))
        assert r.to_sam() == recs


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_constructors_refuse_what_is_not_a_batch():
    ok = {"size": [4, 5], "counts": [3, 2, 15]}
    assert len(RleMasks.from_sam([ok, ok])) == 2
    assert len(RleMasks.from_sam([], size=(4, 5))) == 0
    for bad in ([ok, {"size": [5, 4], "counts": [20]}],            # two sizes
                [{"size": [4, 5], "counts": [3, 2, 14]}],          # short
                [{"size": [4, 5], "counts": [3, 2, 16]}],          # long
                [ok, {"size": [4, 5], "counts": []}],              # no runs
                [{"size": [4, 5], "counts": [21, -1]}],            # a negative count
                [{"size": [4, 5], "counts": "52203"}],             # COCO's compressed string
                [{"counts": [20]}], [np.zeros((4, 5), bool)], []):
        with pytest.raises(ValueError):
            RleMasks.from_sam(bad)
    RleMasks([3, 2, 15, 20], [0, 3, 4], 4, 5)
    for counts, offs, Hm, Wm in (([3, 2, 15, 19], [0, 3, 4], 4, 5), ([3, 2, 15, 20], [0, 3, 3], 4, 5), ([3, 2, 15, 20], [1, 3, 4], 4, 5),
                                 ([3, 2, 15, 20], [0, 4, 3, 4], 4, 5), ([20], [0, 1], 0, 20), ([2 ** 32], [0, 1], 2 ** 16, 2 ** 16)):
        with pytest.raises(ValueError):
            RleMasks(counts, offs, Hm, Wm)
    # the constructor takes zero-length runs anywhere (the kernels do too): they decode to nothing
    z = RleMasks([0, 0, 3, 0, 0, 2, 0, 0, 15], [0, 9], 4, 5)      # (pairs of them: the parity of the runs behind is kept)
    assert np.array_equal(z.to_dense(), RleMasks([3, 2, 15], [0, 3], 4, 5).to_dense())


def test_the_python_constant_is_the_kernels_chunk():
    src = open(os.path.join(ROOT, "revisit-anything_amd", "csrc", "rle_kernels.hip")).read()
    assert int(re.search(r"constexpr int RLE_CHUNK = (\d+);", src).group(1)) == RLE_CHUNK_RUNS
    from revisit_anything_amd import build

    assert "rle_kernels.hip" in build.SOURCES


# ---- the store -----------------------------------------------------------------------------------------------------------------
def test_store_keeps_runs_and_serves_dense_masks(tmp_path):
    from revisit_anything_amd import synth
    from revisit_anything_amd.func_vpr import preload_masks

    blobs = synth.make_blob_masks(12, 240, 320, seed=5).astype(bool)
    recs = [{"segmentation": b, "area": int(b.sum()), "bbox": [0, 0, 3, 4], "predicted_iou": 0.9, "point_coords": [[1.0, 2.0]],
             "stability_score": 0.97, "crop_box": [0, 0, 320, 240]} for b in blobs]
    d_path = st.write_masks(str(tmp_path / "dense"), "a.jpg", recs)                 # the call as it was
    r_path = st.write_masks(str(tmp_path / "rle"), "a.jpg", recs, rle=True)
    assert "segmentation" in np.load(d_path).files and "segmentation" not in np.load(r_path).files
    assert sorted(f for f in np.load(r_path).files if f not in st.MASK_FIELDS) == ["counts", "run_offsets", "size"]
    assert os.path.getsize(r_path) < os.path.getsize(d_path)
    want = RleMasks.from_dense(blobs)
    for root in ("dense", "rle"):
        fs = st.FeatureStore(str(tmp_path / root), "masks")
        grp = fs["a.jpg/masks/"]
        assert grp.keys() == [str(j) for j in range(12)]
        for j in range(12):
            seg = fs[f"a.jpg/masks/{j}"]["segmentation"][()]
            assert seg.dtype == bool and seg.shape == (240, 320) and np.array_equal(seg, blobs[j])
            assert int(fs["a.jpg"]["masks"][str(j)]["area"][()]) == recs[j]["area"]
        back = preload_masks(fs, "a.jpg")
        assert len(back) == 12 and all(np.array_equal(b, m) for b, m in zip(back, blobs))
        got = fs.masks_rle("a.jpg")
        assert isinstance(got, RleMasks) and got == want
    # handed runs: an RleMasks batch, and SAM's records in the run-length mode
    sam = [dict(r, segmentation=s) for r, s in zip(recs, want.to_sam())]
    for k, (key, masks) in enumerate((("b.jpg", want), ("c.jpg", sam))):
        p = st.write_masks(str(tmp_path / "rle"), key, masks)
        assert "counts" in np.load(p).files
        fs = st.FeatureStore(str(tmp_path / "rle"), "masks")
        assert fs.masks_rle(key) == want and np.array_equal(fs[f"{key}/masks/3"]["segmentation"][()], blobs[3])
        assert ("area" in np.load(p).files) == (k == 1)
    # a plain stack, and the dense default for it
    p = st.write_masks(str(tmp_path / "stack"), "s", blobs.astype(np.uint8) * 255, rle=True)
    assert st.FeatureStore(str(tmp_path / "stack"), "masks").masks_rle("s") == want and "counts" in np.load(p).files
    assert "segmentation" in np.load(st.write_masks(str(tmp_path / "stack2"), "s", blobs)).files
    with pytest.raises(ValueError):
        st.FeatureStore(str(tmp_path / "rle"), "dino").masks_rle("a.jpg")


# ---- the producer --------------------------------------------------------------------------------------------------------------
def test_sam_auto_masks_emits_run_length_records():
    import torch
    from sam_stub import stub_predict

    from revisit_anything_amd import producers as pr

    class Stubbed(pr.SamAutoMasks):
        def __init__(self, seed, output_mode):
            self.device = torch.device("cpu")
            self.points_per_batch = 16
            self.pred_iou_thresh, self.stability_score_thresh = 0.88, 0.95
            self.stability_score_offset, self.box_nms_thresh = 1.0, 0.7
            self.min_mask_region_area, self.mask_threshold = 0, 0.0
            self.point_grid = pr.build_point_grid(6)
            self.seed, self.output_mode = seed, output_mode

        def _embed(self, img_rgb):
            return None

        def _predict(self, state, pts_img, out_hw):
            lg, io = stub_predict(pts_img, out_hw[0], out_hw[1], self.seed)
            return torch.from_numpy(lg), torch.from_numpy(io)

    img = np.zeros((72, 96, 3), np.uint8)
    dense = Stubbed(9401, "binary_mask").generate(img)
    runs = Stubbed(9401, "uncompressed_rle").generate(img)
    assert len(dense) == len(runs) >= 3
    for d, r in zip(dense, runs):
        seg = r["segmentation"]
        assert sorted(seg) == ["counts", "size"] and seg["size"] == [72, 96] and all(isinstance(c, int) for c in seg["counts"])
        assert sum(seg["counts"][1::2]) == d["area"] == r["area"]                    # area_from_rle
        assert {k: v for k, v in d.items() if k != "segmentation"} == {k: v for k, v in r.items() if k != "segmentation"}
    assert np.array_equal(RleMasks.from_sam(runs).to_dense(), np.stack([d["segmentation"] for d in dense]))
    assert pr.OUTPUT_MODES == ("binary_mask", "uncompressed_rle")
    with pytest.raises(ValueError):
        pr.SamAutoMasks(None, output_mode="coco_rle")
