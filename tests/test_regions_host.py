"""Small-region removal without a device: the NumPy + scipy restatement (tests/regions_ref.py) and the host path
(producers.remove_small_regions / clean_small_regions) against the reference's own remove_small_regions
(tests/golden/regions_cases.npz), and SamAutoMasks.generate with min_mask_region_area > 0 against the reference's own generate
(tests/golden/sam_generate_regions.npz), both made by tools/make_regions_golden.py.

What the fixtures pin: the reference ran with a `cv2` stand-in whose connectedComponentsWithStats is scipy.ndimage.label plus a
bincount (OpenCV is not installed where they were made) and with the restated torchvision NMS of tools/make_golden.py.  So they
pin the reference's flow -- the complement, the strict threshold, the fill lists, keep-largest, the changed flag, the scoring, the
second NMS, which runs and boxes are refreshed, the reordering, the final area cut -- and not OpenCV's labeller.  Every comparison
is exact."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as RR  # noqa: E402
import regions_stub  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(golden_dir):
    return np.load(os.path.join(golden_dir, "regions_cases.npz"))


@pytest.mark.parametrize("shape", ["33x65", "64x64"])
def test_the_restatement_and_the_host_path_reproduce_the_reference(golden_dir, shape):
    from revisit_anything_amd import producers as pr

    z = _cases(golden_dir)
    H, W = (int(v) for v in shape.split("x"))
    names, masks = RR.table(H, W)
    assert list(z[shape + "_names"]) == names
    assert np.array_equal(np.unpackbits(z[shape + "_masks"], axis=-1)[..., :W], masks != 0)     # the table is the fixture's
    both = set()
    for a in (int(v) for v in z["min_areas"]):
        want = np.unpackbits(z[f"{shape}_a{a}_out"], axis=-1)[..., :W].astype(bool)              # [S, 2, H, W]
        chg = z[f"{shape}_a{a}_changed"]                                                         # [S, 2]
        for j, name in enumerate(names):
            m = masks[j] != 0
            tag = (shape, a, name)
            # the two passes of the restatement
            h, c0 = RR.fill_holes(m, a)
            i, c1 = RR.strip_islands(h, a)
            assert np.array_equal(h, want[j, 0]) and np.array_equal(i, want[j, 1]) and (c0, c1) == tuple(chg[j]), tag
            out, bits, box, area = RR.clean(masks[j], a)
            assert out.dtype == np.uint8 and np.array_equal(out, want[j, 1]) and bits == int(chg[j, 0]) | (int(chg[j, 1]) << 1), tag
            assert area == int(want[j, 1].sum()), tag
            # the host path, mode by mode
            ph, pc0 = pr.remove_small_regions(m, a, "holes")
            pi, pc1 = pr.remove_small_regions(ph, a, "islands")
            assert np.array_equal(ph, want[j, 0]) and np.array_equal(pi, want[j, 1]) and (pc0, pc1) == tuple(chg[j]), tag
            both.add((bool(c0), bool(c1)))
        cleaned, changed = pr.clean_small_regions(masks, a)                                      # non-0/1 bytes included
        assert cleaned.dtype == bool and np.array_equal(cleaned, want[:, 1]) and changed.dtype == np.int32
        assert np.array_equal(changed, chg[:, 0].astype(np.int32) | (chg[:, 1].astype(np.int32) << 1))
    assert len(both) == 4                                                                        # every combination of the flags


def test_boxes_of_the_restatement_are_mask_boxes():
    import torch

    from revisit_anything_amd import producers as pr

    names, masks = RR.table(33, 65)
    out, _, boxes, area = RR.clean_batch(masks, 7)
    assert np.array_equal(boxes, pr.mask_boxes(torch.from_numpy(out != 0)).numpy()) and np.array_equal(area, out.reshape(len(out), -1).sum(1))
    assert boxes[names.index("zero")].tolist() == [0, 0, 0, 0]


def test_the_cases_the_contract_names():
    """by hand, at 33 x 65: the things the contract spells out"""
    names, masks = RR.table(33, 65)
    g = lambda n: masks[names.index(n)]                                                      # noqa: E731
    # a mask whose only island is small comes back identical and flagged changed (islands only)
    out, bits, _, _ = RR.clean(g("one_small_island"), 5)
    assert np.array_equal(out, g("one_small_island")) and bits == 2
    # strictly <: a component of exactly min_area stays and nothing is flagged
    out, bits, _, _ = RR.clean(g("one_small_island"), 4)
    assert np.array_equal(out, g("one_small_island")) and bits == 0
    # the tie for the largest goes to the earlier first pixel: the run in row 0, not the column that starts in row 3
    out, bits, box, area = RR.clean(g("small_islands_tie"), 4)
    assert area == 3 and box == [6, 0, 8, 0] and bits == 2
    # the diamond ring's inside is no hole under 8-connectivity; the square ring's is
    out, bits, _, _ = RR.clean(g("diamond_ring"), 4)
    assert np.array_equal(out, g("diamond_ring")) and bits == 0
    out, bits, _, area = RR.clean(g("square_ring"), RR.HOLE + 1)
    assert bits == 1 and area == 64
    assert RR.clean(g("square_ring"), RR.HOLE)[1] == 0
    # the outer background is filled like any hole when it is small; then the full mask is one island below P + 1
    out, bits, _, area = RR.clean(g("small_background"), 5)
    assert bits == 1 and area == 33 * 65
    out, bits, _, area = RR.clean(g("zero"), 33 * 65 + 1)
    assert bits == 3 and area == 33 * 65
    # an all-zero mask under islands and an all-ones mask under holes have no components
    assert RR.clean(g("zero"), 7)[1] == 0 and RR.clean(g("ones"), 7)[1] == 0


def _records_equal(got, z, c, H, W):
    seg = np.unpackbits(z[f"c{c}_seg"], axis=-1)[..., :W].astype(bool)
    assert len(got) == len(seg), (len(got), len(seg))
    for j, r in enumerate(got):
        assert sorted(r) == ["area", "bbox", "crop_box", "point_coords", "predicted_iou", "segmentation", "stability_score"]
        assert r["segmentation"].dtype == bool and np.array_equal(r["segmentation"], seg[j]), (c, j)
        assert r["area"] == int(z[f"c{c}_area"][j]) and r["bbox"] == z[f"c{c}_bbox"][j].tolist(), (c, j)
        assert r["predicted_iou"] == float(z[f"c{c}_iou"][j]) and r["stability_score"] == float(z[f"c{c}_stab"][j]), (c, j)
        assert r["point_coords"] == [z[f"c{c}_pts"][j].tolist()] and r["crop_box"] == z[f"c{c}_crop"][j].tolist(), (c, j)


@pytest.mark.parametrize("c", range(len(regions_stub.CASES)))
def test_generate_reproduces_the_references_records(golden_dir, c):
    """same records, same order, every field.  (Without postprocess_small_regions in generate this fails: the reference's
    output was asserted, when the fixture was made, to hold a filled hole, a stripped island, a mask flagged but identical, a
    mask the second NMS dropped, a changed order and a record the final area cut removed.)"""
    from revisit_anything_amd.rle import RleMasks

    z = np.load(os.path.join(golden_dir, "sam_generate_regions.npz"))
    H, W, pps, ppb, kw, seed = regions_stub.CASES[c]
    assert int(z["n_cases"]) == len(regions_stub.CASES) and z[f"c{c}_args"].tolist() == [H, W, pps, ppb, seed]
    img = np.zeros((H, W, 3), np.uint8)
    got = regions_stub.stubbed_generator(seed, pps, ppb, kw).generate(img)
    _records_equal(got, z, c, H, W)
    ious = [r["predicted_iou"] for r in got]
    assert ious != sorted(ious, reverse=True)                       # unchanged masks first: no longer the order of the first NMS
    assert all(r["area"] > kw["min_mask_region_area"] for r in got)
    # run-length mode: the same records with the runs of the cleaned masks
    rle = regions_stub.stubbed_generator(seed, pps, ppb, kw, output_mode="uncompressed_rle").generate(img)
    assert len(rle) == len(got)
    dense = RleMasks.from_sam(rle).to_dense()
    for j, (a, b) in enumerate(zip(rle, got)):
        assert np.array_equal(np.asarray(dense[j]) != 0, b["segmentation"]) and {k: v for k, v in a.items() if k != "segmentation"} == \
            {k: v for k, v in b.items() if k != "segmentation"}, (c, j)


def test_a_stand_in_engine_cleans_for_the_generator():
    """regions_engine, and rle_engine as its fall-back: the generator hands the kept masks over and reads back flags and boxes"""
    import torch

    from revisit_anything_amd.rle import RleMasks

    class StandIn:
        def __init__(self):
            self.calls = []

        def mask_regions(self, masks, min_area, want_boxes=True, want_area=True, chunk=None):
            assert isinstance(masks, torch.Tensor) and masks.dtype == torch.bool and masks.dim() == 3
            self.calls.append((tuple(masks.shape), min_area))
            out, chg, boxes, area = RR.clean_batch(masks.numpy(), min_area)
            return {"masks": torch.from_numpy(out), "changed": torch.from_numpy(chg), "boxes": torch.from_numpy(boxes)}

        def rle_encode(self, masks, want_area=False, capacity=None):
            r = RleMasks.from_dense(masks)
            return (r, torch.from_numpy(r.areas())) if want_area else r

    H, W, pps, ppb, kw, seed = regions_stub.CASES[0]
    img = np.zeros((H, W, 3), np.uint8)
    host = regions_stub.stubbed_generator(seed, pps, ppb, kw).generate(img)
    eng = StandIn()
    got = regions_stub.stubbed_generator(seed, pps, ppb, kw, regions_engine=eng).generate(img)
    assert len(eng.calls) == 1 and eng.calls[0][1] == kw["min_mask_region_area"]
    assert len(got) == len(host) and all(np.array_equal(a.pop("segmentation"), b["segmentation"]) and a == {k: v for k, v in b.items() if k != "segmentation"}
                                         for a, b in zip(got, host))
    host_rle = regions_stub.stubbed_generator(seed, pps, ppb, kw, output_mode="uncompressed_rle").generate(img)
    eng = StandIn()
    got = regions_stub.stubbed_generator(seed, pps, ppb, kw, output_mode="uncompressed_rle", rle_engine=eng).generate(img)
    assert len(eng.calls) == 1 and got == host_rle
    # the parameter at 0: nobody is asked
    idle = StandIn()
    kw0 = dict(kw, min_mask_region_area=0)
    a = regions_stub.stubbed_generator(seed, pps, ppb, kw0, regions_engine=idle).generate(img)
    assert idle.calls == [] and len(a) > len(host)


def test_the_surface():
    from revisit_anything_amd import _lib, build
    from revisit_anything_amd import producers as pr

    hdr = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    decl = re.search(r"^int segvlad_mask_regions\((.*?)\);", hdr, flags=re.S | re.M).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    assert args == ["segvlad_ctx* ctx", "const uint8_t* masks", "int S", "int Hm", "int Wm", "int min_area", "uint8_t* masks_out",
                    "int32_t* changed_out", "int32_t* boxes_out", "int64_t* area_out"]
    assert "amg.py:267-291" in hdr and "automatic_mask_generator.py:325-376" in hdr and '"mask_regions"' in hdr
    res, argtypes = _lib.SIGNATURES["segvlad_mask_regions"]
    assert len(argtypes) == 10
    assert re.search(r"Each of the (\d+) entry points", hdr).group(1) == str(len(_lib.SIGNATURES))
    assert "regions_kernels.hip" in build.SOURCES
    p = inspect.signature(pr.SamAutoMasks.__init__).parameters
    assert list(p)[-2:] == ["crop_nms_thresh", "regions_engine"] and p["crop_nms_thresh"].default == 0.7 and p["regions_engine"].default is None
    with pytest.raises(ValueError):
        pr.remove_small_regions(np.zeros((3, 3), bool), 2, "both")
