"""The device run-length encoder without a device: the NumPy restatement of its plan (tests/rle_encode_ref.py) against
RleMasks.from_dense -- which tests/test_rle_host.py pins to the reference's own counts --, RleMasks.areas (area_from_rle), the
constant, the header and the table, and the producer's `rle_engine` keyword with a stand-in engine.  No GPU; every comparison is
exact."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_branch_cases as T  # noqa: E402
import rle_encode_ref as R  # noqa: E402

from revisit_anything_amd.rle import RleMasks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = ("same", "x2", "x2clip", "nonint", "down")


def _rows():
    from revisit_anything_amd.rle import RLE_ENCODE_ROWS

    return RLE_ENCODE_ROWS


def _model_equals_from_dense(m, rows, tag):
    want = RleMasks.from_dense(m)
    counts, offs, areas = R.encode_model(m, rows)
    assert offs.dtype == np.int64 and np.array_equal(offs, want.run_offsets), tag
    assert counts.dtype == np.uint32 and np.array_equal(counts, want.counts), tag
    assert np.array_equal(areas, (np.asarray(m) != 0).sum(axis=(1, 2))), tag
    assert np.array_equal(want.areas(), areas), tag
    # the capacity protocol: one slot short -> no counts, the same offsets
    if len(counts):
        none, offs2, _ = R.encode_model(m, rows, capacity=len(counts) - 1)
        assert none is None and np.array_equal(offs2, offs), tag
        assert R.encode_model(m, rows, capacity=len(counts))[0] is not None, tag


@pytest.mark.parametrize("name", T.INC_NAMES)
def test_the_plan_emits_from_denses_counts_over_the_shape_table(name):
    m = T.build_masks(name)[0]
    _model_equals_from_dense(m, _rows(), name)
    if m.size <= 1 << 20 and len(m):     # several row blocks per column as well
        _model_equals_from_dense(m, 32, (name, 32))


@pytest.mark.parametrize("Hm,Wm", R.RUN_GEOMETRIES, ids=["%dx%d" % g for g in R.RUN_GEOMETRIES])
def test_the_plan_on_run_structures(Hm, Wm):
    m, names = R.run_structure_masks(Hm, Wm)
    P = Hm * Wm
    r = RleMasks.from_dense(m)
    runs = dict(zip(names, np.diff(r.run_offsets).tolist()))
    assert runs["alternate"] == P and runs["alternate_from_one"] == P + 1 and runs["first_pixel"] == 3 and runs["last_pixel"] == 2
    assert runs["one_whole_column"] == 3 and runs["isolated"] >= 401
    for rows in (_rows(), 32):
        _model_equals_from_dense(m, rows, (Hm, Wm, rows))


@pytest.mark.parametrize("Wm", R.LANE_WIDTHS)
def test_the_plan_on_lane_edges(Wm):
    _model_equals_from_dense(R.lane_edge_masks(Wm), _rows(), Wm)


@pytest.mark.parametrize("Wm", (1, 3))
def test_the_plan_on_block_edges(Wm):
    """The tall shapes of the device test, 2 * rows + 33 rows, with 32-row units: three blocks per column at no cost"""
    m = R.block_edge_masks(32, Wm)
    assert m.shape[1] == 97
    _model_equals_from_dense(m, 32, Wm)
    _model_equals_from_dense(m, 64, (Wm, 64))                   # the same masks, the boundaries now inside a block
    big = R.block_edge_masks(_rows(), Wm)                      # what the device test encodes
    assert big.shape[1] == 2 * _rows() + 33
    _model_equals_from_dense(big, _rows(), (Wm, "device shape"))


def _golden_masks(golden_dir, name):
    zi = np.load(os.path.join(golden_dir, "incidence_cases.npz"))
    S, Hm, Wm = (int(v) for v in zi[name + "_shape"][:3])
    return np.unpackbits(zi[name + "_masks"], axis=1)[:, :Hm * Wm].reshape(S, Hm, Wm)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_areas_are_the_dense_sums_on_the_references_cases(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "rle_cases.npz"))
    m = _golden_masks(golden_dir, name)
    Hm, Wm = (int(v) for v in z[name + "_size"])
    r = RleMasks(z[name + "_counts"], z[name + "_offsets"], Hm, Wm)          # the reference's own counts
    a = r.areas()
    assert a.dtype == np.int64 and np.array_equal(a, m.reshape(len(m), -1).sum(1))
    counts, offs, areas = R.encode_model(m, _rows())
    assert np.array_equal(counts, z[name + "_counts"]) and np.array_equal(offs, z[name + "_offsets"]) and np.array_equal(areas, a)


def test_areas_of_a_set_first_pixel_of_no_mask_and_of_tensors():
    import torch

    m = np.zeros((3, 5, 4), np.uint8)
    m[0, 0, 0] = 7                                               # [0, 1, 19]
    m[1] = 1                                                     # [0, 20]
    m[2, 2:, 1:3] = 200
    r = RleMasks.from_dense(m)
    assert r.to_sam()[0]["counts"] == [0, 1, 19] and r.areas().tolist() == [1, 20, 6]
    assert r.to("cpu").areas().tolist() == [1, 20, 6] and isinstance(r.to("cpu").counts, torch.Tensor)
    e = RleMasks.from_dense(np.zeros((0, 5, 4), np.uint8))
    assert e.areas().shape == (0,) and e.areas().dtype == np.int64
    counts, offs, areas = R.encode_model(np.zeros((0, 5, 4), np.uint8), 32)
    assert len(counts) == 0 and offs.tolist() == [0] and len(areas) == 0


def test_the_python_constant_is_the_kernels_unit():
    from revisit_anything_amd import build, engine

    src = open(os.path.join(ROOT, "revisit-anything_amd", "csrc", "rle_encode_kernels.hip")).read()
    assert int(re.search(r"constexpr int RLE_ENCODE_ROWS = (\d+);", src).group(1)) == _rows() == engine.RLE_ENCODE_ROWS
    assert _rows() % 32 == 0 and "rle_encode_kernels.hip" in build.SOURCES


def test_the_header_declares_the_entry_and_the_table_binds_ten_arguments():
    from revisit_anything_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    decl = re.search(r"^int segvlad_rle_encode\((.*?)\);", hdr, flags=re.S | re.M).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    assert len(args) == 10 and args[0] == "segvlad_ctx* ctx" and args[-1] == "int64_t* n_runs_out" and args[7] == "int64_t capacity"
    res, argtypes = _lib.SIGNATURES["segvlad_rle_encode"]
    assert len(argtypes) == 10
    assert "amg.py:107-135" in hdr and "area_from_rle" in hdr and '"rle_encode"' in hdr
    assert re.search(r"Each of the (\d+) entry points", hdr).group(1) == str(len(_lib.SIGNATURES))


def test_the_producer_takes_its_runs_from_the_engine_it_is_given():
    import torch
    from sam_stub import stub_predict

    from revisit_anything_amd import producers as pr

    class StandIn:
        """an engine whose rle_encode is the host encoder"""

        def __init__(self):
            self.calls = []

        def rle_encode(self, masks, want_area=False, capacity=None):
            assert isinstance(masks, torch.Tensor) and masks.dtype == torch.bool and masks.dim() == 3
            self.calls.append((tuple(masks.shape), want_area))
            r = RleMasks.from_dense(masks)
            return (r, torch.from_numpy(r.areas())) if want_area else r

    class Stubbed(pr.SamAutoMasks):
        def __init__(self, seed, output_mode, rle_engine=None):
            self.device = torch.device("cpu")
            self.points_per_batch = 16
            self.pred_iou_thresh, self.stability_score_thresh = 0.88, 0.95
            self.stability_score_offset, self.box_nms_thresh = 1.0, 0.7
            self.min_mask_region_area, self.mask_threshold = 0, 0.0
            self.point_grid = pr.build_point_grid(6)
            self.seed, self.output_mode = seed, output_mode
            if rle_engine is not None:
                self.rle_engine = rle_engine

        def _embed(self, img_rgb):
            return None

        def _predict(self, state, pts_img, out_hw):
            lg, io = stub_predict(pts_img, out_hw[0], out_hw[1], self.seed)
            return torch.from_numpy(lg), torch.from_numpy(io)

    img = np.zeros((72, 96, 3), np.uint8)
    host = Stubbed(9401, "uncompressed_rle").generate(img)
    eng = StandIn()
    got = Stubbed(9401, "uncompressed_rle", eng).generate(img)
    assert len(host) >= 3 and eng.calls == [((len(host), 72, 96), True)]
    assert got == host                                           # key for key, value for value
    assert all(type(g["area"]) is int and all(type(c) is int for c in g["segmentation"]["counts"]) for g in got)
    # the dense mode never asks the engine
    idle = StandIn()
    dense = Stubbed(9401, "binary_mask", idle).generate(img)
    assert idle.calls == [] and all(d["segmentation"].dtype == bool for d in dense) and len(dense) == len(host)
    # the keyword of the real constructor
    import inspect

    assert inspect.signature(pr.SamAutoMasks.__init__).parameters["rle_engine"].default is None
    assert pr.OUTPUT_MODES == ("binary_mask", "uncompressed_rle")
