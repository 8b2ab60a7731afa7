"""The device run-length encoder (csrc/rle_encode_kernels.hip, segvlad_rle_encode / SegVLADEngine.rle_encode) against the host
encoder RleMasks.from_dense, which tests/test_rle_host.py pins to the reference's own counts: over the mask branch's shape table,
over masks built for the run bookkeeping, at the edges of a lane, a wave and a row block, through the capacity protocol of the raw
C ABI, its refusals, the producer and the store.  Every comparison is exact; the masks are those of tests/rle_encode_ref.py, whose
NumPy model of the plan tests/test_rle_encode_host.py holds against the same encoder."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from conftest import engine_scope

import mask_branch_cases as T
import rle_encode_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _R():
    from revisit_anything_amd.rle import RleMasks

    return RleMasks


def _check(tag, got, areas, m):
    """an RleMasks with device tensors (+ device areas) against the host encoder of the host masks m"""
    want = _R().from_dense(m)
    assert isinstance(got.counts, torch.Tensor) and got.counts.is_cuda and got.counts.dtype == torch.uint32, tag
    assert isinstance(got.run_offsets, torch.Tensor) and got.run_offsets.is_cuda and got.run_offsets.dtype == torch.int64, tag
    c, o = got.arrays()
    assert got.size == want.size and len(got) == len(want), tag
    assert np.array_equal(o, want.run_offsets), (tag, "offsets", np.argwhere(o != want.run_offsets)[:5].tolist())
    assert c.shape == want.counts.shape, tag
    assert np.array_equal(c, want.counts), (tag, "first wrong runs", np.argwhere(c != want.counts)[:5].tolist())
    if areas is not None:
        assert areas.is_cuda and areas.dtype == torch.int64 and tuple(areas.shape) == (len(want),), tag
        assert np.array_equal(areas.cpu().numpy(), (np.asarray(m) != 0).sum(axis=(1, 2))), tag
    return want


def _encode_and_check(eng, tag, m):
    md = torch.tensor(np.array(m)).to(eng.device)
    got, areas = eng.rle_encode(md, want_area=True)
    return md, got, _check(tag, got, areas, m)


# ---- 1. the shape table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.INC_NAMES)
def test_shape_table(eng, name):
    c = T.INC_BY_NAME[name]
    m = T.build_masks(name)[0]
    buf = torch.zeros(c["offset"] + m.size + 16, dtype=torch.uint8, device=eng.device)
    buf[c["offset"]:c["offset"] + m.size] = torch.tensor(m.reshape(-1)).to(eng.device)
    md = buf[c["offset"]:c["offset"] + m.size].view(m.shape)     # (unfused_misaligned: one byte into the buffer -> the byte loads)
    assert md.is_contiguous() and md.data_ptr() % 16 == c["offset"] % 16
    got, areas = eng.rle_encode(md, want_area=True)
    _check(name, got, areas, m)
    if m.size <= 1 << 20:                                          # host masks, staged by the library
        for host in (np.array(m), torch.tensor(np.array(m))):
            got, areas = eng.rle_encode(host, want_area=True)
            _check((name, type(host).__name__), got, areas, m)
        _check((name, "no areas"), eng.rle_encode(md), None, m)


# ---- 2. run structures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hm,Wm", R.RUN_GEOMETRIES, ids=["%dx%d" % g for g in R.RUN_GEOMETRIES])
def test_run_structures(eng, Hm, Wm):
    m, names = R.run_structure_masks(Hm, Wm)
    H, W = (126, 150) if (Hm, Wm) == (64, 96) else (70, 84)
    md, got, want = _encode_and_check(eng, (Hm, Wm), m)
    runs = dict(zip(names, np.diff(want.run_offsets).tolist()))
    assert runs["alternate_from_one"] == Hm * Wm + 1 and eng.rle_encode_retried     # more runs than a column-convex blob's
    c, o = got.arrays()
    bad = sorted({names[s] for s in range(len(m)) if not np.array_equal(c[o[s]:o[s + 1]], want.counts[o[s]:o[s + 1]])})
    assert not bad, bad
    back, n_bad = eng.rle_decode(got, want_bad=True)
    assert back.cpu().numpy().tobytes() == (m != 0).astype(np.uint8).tobytes() and int(n_bad.item()) == 0
    bits, cent = eng.incidence_rle(got, H, W, 14)
    db, dc = eng.incidence_centroids(md, H, W, 14)
    assert bits.cpu().numpy().tobytes() == db.cpu().numpy().tobytes() and cent.cpu().numpy().tobytes() == dc.cpu().numpy().tobytes()


# ---- 3. lane and block edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wm", R.LANE_WIDTHS)
def test_lane_edges(eng, Wm):
    _encode_and_check(eng, Wm, R.lane_edge_masks(Wm))


@pytest.mark.parametrize("Wm", (1, 3))
def test_block_edges(eng, Wm):
    from revisit_anything_amd.rle import RLE_ENCODE_ROWS

    m = R.block_edge_masks(RLE_ENCODE_ROWS, Wm)
    assert m.shape[1] == 2 * RLE_ENCODE_ROWS + 33
    _encode_and_check(eng, Wm, m)


# ---- 4. the capacity protocol, through the raw C ABI -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _protocol_case():
    m = R.run_structure_masks(33, 40)[0]
    return m, _R().from_dense(m)


def _raw(eng, masks, S, Hm, Wm, offs, counts, capacity, areas, total):
    from revisit_anything_amd.engine import _ptr

    eng._stream()
    return eng.lib.segvlad_rle_encode(eng._h, _ptr(masks), S, Hm, Wm, _ptr(offs), _ptr(counts), capacity, _ptr(areas),
                                      C.byref(total) if total is not None else None)


@pytest.mark.parametrize("where", ["device", "host"])
def test_capacity_protocol(eng, where):
    m, want = _protocol_case()
    S, Hm, Wm = m.shape
    n = len(want.counts)
    md = torch.tensor(m).to(eng.device)

    def buffers(slots):
        if where == "device":
            return (torch.full((S + 1,), -7, dtype=torch.int64, device=eng.device), torch.full((slots,), SENTINEL, dtype=torch.int32, device=eng.device),
                    torch.full((S,), -7, dtype=torch.int64, device=eng.device))
        return np.full(S + 1, -7, np.int64), np.full(slots, SENTINEL, np.int32), np.full(S, -7, np.int64)

    def host(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else x

    # one slot short: nothing is written to the counts, everything else is true, and the call succeeds
    offs, counts, areas = buffers(n + 5)
    total = C.c_int64(-1)
    eng._check(_raw(eng, md, S, Hm, Wm, offs, counts, n - 1, areas, total), "rle_encode")
    eng.synchronize()
    assert total.value == n and np.array_equal(host(offs), want.run_offsets) and (host(counts) == SENTINEL).all()
    assert np.array_equal(host(areas), (m != 0).sum(axis=(1, 2)))
    # exactly enough: the runs, and the slots behind them untouched
    offs, counts, areas = buffers(n + 5)
    total = C.c_int64(-1)
    eng._check(_raw(eng, md, S, Hm, Wm, offs, counts, n, None, total), "rle_encode")
    eng.synchronize()
    got = host(counts)
    assert total.value == n and np.array_equal(got[:n].view(np.uint32), want.counts) and (got[n:] == SENTINEL).all()
    assert np.array_equal(host(offs), want.run_offsets) and (host(areas) == -7).all()
    # a count-only call
    offs, _, areas = buffers(1)
    total = C.c_int64(-1)
    eng._check(_raw(eng, md, S, Hm, Wm, offs, None, 0, areas, total), "rle_encode")
    eng.synchronize()
    assert total.value == n and np.array_equal(host(offs), want.run_offsets) and np.array_equal(host(areas), (m != 0).sum(axis=(1, 2)))
    # without the host total: device outputs, no n_runs_out
    if where == "device":
        offs, counts, areas = buffers(n + 5)
        eng._check(_raw(eng, md, S, Hm, Wm, offs, counts, n + 5, areas, None), "rle_encode")
        eng.synchronize()
        got = host(counts)
        assert np.array_equal(got[:n].view(np.uint32), want.counts) and (got[n:] == SENTINEL).all() and np.array_equal(host(offs), want.run_offsets)


def test_the_engine_repeats_the_call_with_the_total(eng):
    m, want = _protocol_case()
    md = torch.tensor(m).to(eng.device)
    got = eng.rle_encode(md[:1], capacity=1)                       # the alternating mask: P runs
    assert eng.rle_encode_retried and len(got.counts) == 33 * 40
    _check("capacity=1", got, None, m[:1])
    got = eng.rle_encode(md, capacity=len(want.counts))
    assert not eng.rle_encode_retried
    _check("capacity=total", got, None, m)
    with pytest.raises(ValueError):
        eng.rle_encode(md, capacity=-1)


# ---- 5. the forms of the input ---------------------------------------------------------------------------------------------------
def test_bool_single_and_strided_masks(eng):
    m = R.lane_edge_masks(65)                                      # uint8 [4, 33, 65]
    b = torch.tensor(m != 0).to(eng.device)
    assert b.dtype == torch.bool
    got, areas = eng.rle_encode(b, want_area=True)
    _check("bool", got, areas, m)
    assert eng._keep[0].data_ptr() == b.data_ptr()                 # viewed as bytes, not copied
    _check("bool, host", eng.rle_encode(m != 0), None, m)
    one = eng.rle_encode(torch.tensor(m[2]).to(eng.device))        # a single [Hm, Wm]
    assert len(one) == 1
    _check("2-D", one, None, m[2:3])
    wide = torch.tensor(np.concatenate([m, m[:, :, ::-1]], axis=2)).to(eng.device)
    view = wide[:, :, 65:]                                         # not contiguous
    assert not view.is_contiguous()
    _check("strided", eng.rle_encode(view), None, m[:, :, ::-1])
    _check("transposed", eng.rle_encode(wide.transpose(1, 2)), None, wide.cpu().numpy().transpose(0, 2, 1))
    with pytest.raises(TypeError):
        eng.rle_encode(torch.zeros(1, 4, 4, dtype=torch.float32, device=eng.device))
    with pytest.raises(ValueError):
        eng.rle_encode(torch.zeros(4, dtype=torch.uint8, device=eng.device))


def test_no_masks(eng):
    got, areas = eng.rle_encode(torch.zeros((0, 64, 96), dtype=torch.uint8, device=eng.device), want_area=True)
    assert len(got) == 0 and got.run_offsets.cpu().tolist() == [0] and got.counts.shape[0] == 0 and areas.shape[0] == 0 and got.size == [64, 96]
    # the raw call: offsets[0] and the total are written, nothing else
    for offs in (torch.full((2,), -7, dtype=torch.int64, device=eng.device), np.full(2, -7, np.int64)):
        counts = torch.full((4,), SENTINEL, dtype=torch.int32, device=eng.device)
        areas = torch.full((2,), -7, dtype=torch.int64, device=eng.device)
        total = C.c_int64(-1)
        eng._check(_raw(eng, None, 0, 64, 96, offs, counts, 4, areas, total), "rle_encode")
        eng.synchronize()
        o = offs.cpu().numpy() if isinstance(offs, torch.Tensor) else offs
        assert total.value == 0 and o.tolist() == [0, -7] and (counts == SENTINEL).all() and (areas == -7).all()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_LIMIT, SEGVLAD_ERR_STATE, SegVLADError

    m, want = _protocol_case()
    S, Hm, Wm = m.shape
    md = torch.tensor(m).to(eng.device)
    offs = torch.zeros(S + 1, dtype=torch.int64, device=eng.device)
    counts = torch.full((8,), SENTINEL, dtype=torch.int32, device=eng.device)
    one = torch.zeros(1, dtype=torch.uint8, device=eng.device)

    def code(rc):
        with pytest.raises(SegVLADError) as e:
            eng._check(rc, "refused")
        return e.value.code

    for args in ((md, -1, Hm, Wm, offs, counts, 8), (md, S, 0, Wm, offs, counts, 8), (md, S, Hm, -3, offs, counts, 8), (md, S, Hm, Wm, offs, counts, -1),
                 (md, S, Hm, Wm, None, counts, 8), (None, S, Hm, Wm, offs, counts, 8), (md, S, Hm, Wm, offs, None, 8)):
        assert code(_raw(eng, *args, None, None)) == SEGVLAD_ERR_ARG, args[1:4]
    # 2^32 pixels: refused from the shape alone (the one byte behind the pointer is never read)
    assert code(_raw(eng, one, 1, 65536, 65536, offs, counts, 8, None, None)) == SEGVLAD_ERR_LIMIT
    eng.synchronize()
    assert (counts == SENTINEL).all() and (offs == 0).all()
    with pytest.raises(SegVLADError) as e:
        eng.rle_encode(torch.zeros((0, 65536, 65536), dtype=torch.uint8, device=eng.device))   # (no bytes: the shape alone)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    # an open describe
    from revisit_anything_amd import synth

    Hd, Wd, H, W, K, D = 64, 96, 126, 150, 8, 64
    Cc = synth.make_vocab(K, D, seed=700)
    eng.set_vocab(Cc)
    N = (H // 14) * (W // 14)
    sizes = (4, 6)
    tok = torch.tensor(np.stack([synth.make_tokens(Cc, N, seed=701 + b, noise=0.2) for b in range(len(sizes))])).to(eng.device)
    dm = torch.tensor(np.concatenate([synth.make_blob_masks(s, Hd, Wd, seed=750 + b) for b, s in enumerate(sizes)]).astype(np.uint8)).to(eng.device)
    so = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    h = eng.describe_begin(dm, tok, so, H, W, 14, 3, pca=False)
    with pytest.raises(SegVLADError) as e:
        eng.rle_encode(md)
    assert e.value.code == SEGVLAD_ERR_STATE
    out = eng.describe_end(h, None, None)["out"]
    assert torch.isfinite(out).all()
    _check("after the open describe", eng.rle_encode(md), None, m)   # and the context is free again


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------
def test_two_calls_write_the_same_bytes(eng):
    m = T.build_masks("unfused_wm_down_gridy2")[0]
    md = torch.tensor(np.array(m)).to(eng.device)
    a, aa = eng.rle_encode(md, want_area=True)
    b, ba = eng.rle_encode(md, want_area=True)
    assert a.counts.cpu().numpy().tobytes() == b.counts.cpu().numpy().tobytes() and torch.equal(a.run_offsets, b.run_offsets) and torch.equal(aa, ba)


# ---- 8. the producer ---------------------------------------------------------------------------------------------------------------
def test_the_producer_encodes_on_the_device(eng, monkeypatch):
    from sam_stub import stub_predict

    from revisit_anything_amd import producers as pr

    class Stubbed(pr.SamAutoMasks):
        def __init__(self, seed, device, rle_engine=None):
            self.device = torch.device(device)
            self.points_per_batch = 16
            self.pred_iou_thresh, self.stability_score_thresh = 0.88, 0.95
            self.stability_score_offset, self.box_nms_thresh = 1.0, 0.7
            self.min_mask_region_area, self.mask_threshold = 0, 0.0
            self.point_grid = pr.build_point_grid(6)
            self.seed, self.output_mode = seed, "uncompressed_rle"
            if rle_engine is not None:
                self.rle_engine = rle_engine

        def _embed(self, img_rgb):
            return None

        def _predict(self, state, pts_img, out_hw):
            lg, io = stub_predict(pts_img, out_hw[0], out_hw[1], self.seed)
            return torch.from_numpy(lg).to(self.device), torch.from_numpy(io).to(self.device)

    img = np.zeros((72, 96, 3), np.uint8)
    host = Stubbed(9401, "cpu").generate(img)
    assert len(host) >= 3

    def refuse(*a, **k):
        raise AssertionError("the host encoder was called")

    with monkeypatch.context() as mp:
        mp.setattr(_R(), "from_dense", refuse)
        got = Stubbed(9401, eng.device, eng).generate(img)
    assert got == host


# ---- 9. the store ------------------------------------------------------------------------------------------------------------------
def test_the_store_takes_the_device_batch(eng, tmp_path):
    from revisit_anything_amd import store as st
    from revisit_anything_amd import synth

    blobs = synth.make_blob_masks(12, 240, 320, seed=5).astype(np.uint8)
    rle = eng.rle_encode(torch.tensor(blobs).to(eng.device))
    st.write_masks(str(tmp_path), "a.jpg", rle)
    back = st.FeatureStore(str(tmp_path), "masks").masks_rle("a.jpg")
    assert back == _R().from_dense(blobs) and isinstance(back.counts, np.ndarray)
