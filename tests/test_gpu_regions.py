"""Small-region removal on the device (csrc/regions_kernels.hip, segvlad_mask_regions / SegVLADEngine.mask_regions) against the
NumPy + scipy restatement of its contract (tests/regions_ref.py, which tests/test_regions_host.py holds to the reference's own
remove_small_regions): masks, changed bits, boxes and areas, exactly.  The shapes cross tiles of 16, 32 and 64 in both axes with
widths that are no multiple of 4; the masks are the table of regions_ref.patterns -- lines that are 8-connected only, pixel pairs
on every tile corner in both diagonal orientations, a serpentine (the longest chain) and its complement, rings, nesting, small
backgrounds, ties -- crossed with min_area = 1, 2, 3, a planted component's size and that + 1, and a value above P.  Then batch
isolation, in place, determinism, chunking, pointer kinds, NULL outputs, S == 0, every refusal and the generator."""
import numpy as np
import pytest
import torch
from conftest import engine_scope

import regions_ref as RR
import regions_stub

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _compare(tag, out, want, names=None):
    """the dict of mask_regions against (masks, changed, boxes, area) of the restatement; names the masks that differ"""
    wm, wc, wb, wa = want
    S = len(wm)
    name = (lambda s: names[s]) if names is not None else (lambda s: s)
    assert out["masks"].is_cuda and out["masks"].dtype == torch.uint8 and tuple(out["masks"].shape) == wm.shape, tag
    assert out["changed"].dtype == torch.int32 and tuple(out["changed"].shape) == (S,), tag
    gm, gc = out["masks"].cpu().numpy(), out["changed"].cpu().numpy()
    bad = [name(s) for s in range(S) if not np.array_equal(gm[s], wm[s])]
    assert not bad, (tag, "masks differ", bad)
    bad = [(name(s), int(gc[s]), int(wc[s])) for s in range(S) if gc[s] != wc[s]]
    assert not bad, (tag, "changed bits differ (name, got, want)", bad)
    if "boxes" in out:
        assert out["boxes"].dtype == torch.int32 and tuple(out["boxes"].shape) == (S, 4), tag
        gb = out["boxes"].cpu().numpy()
        bad = [(name(s), gb[s].tolist(), wb[s].tolist()) for s in range(S) if not np.array_equal(gb[s], wb[s])]
        assert not bad, (tag, "boxes differ", bad)
    if "area" in out:
        assert out["area"].dtype == torch.int64 and tuple(out["area"].shape) == (S,), tag
        ga = out["area"].cpu().numpy()
        bad = [(name(s), int(ga[s]), int(wa[s])) for s in range(S) if ga[s] != wa[s]]
        assert not bad, (tag, "areas differ", bad)


# ---- 1. the table: shapes x patterns x min_area --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", RR.SHAPES, ids=["%dx%d" % s for s in RR.SHAPES])
def test_table(eng, H, W):
    names, masks = RR.table(H, W)
    md = torch.tensor(masks).to(eng.device)
    for a in RR.min_areas(H, W):
        _compare((H, W, a), eng.mask_regions(md, a), RR.expected(H, W, a), names)
    assert torch.equal(md.cpu(), torch.tensor(masks))              # the input is not written


# ---- 2. batch isolation, in place, determinism, chunking -------------------------------------------------------------------------
@pytest.mark.parametrize("a", [2, 11, 40 * 70 + 1])
def test_a_batch_is_its_masks_one_by_one(eng, a):
    b = RR.isolation_batch()
    assert len(b) >= 8 and not b[0].any() and b[1].all() and b[2, -1, 10:20].all() and b[3, 0, 10:20].all()
    md = torch.tensor(b).to(eng.device)
    want = RR.clean_batch(b, a)
    whole = eng.mask_regions(md, a)
    _compare(("batch", a), whole, want)
    for s in range(len(b)):
        one = eng.mask_regions(md[s], a)
        _compare(("alone", a, s), one, tuple(w[s:s + 1] for w in want))
    # chunk = 3 on the batch: three calls, the same result
    parts = eng.mask_regions(md, a, chunk=3)
    assert all(torch.equal(parts[k], whole[k]) for k in whole)
    with pytest.raises(ValueError):
        eng.mask_regions(md, a, chunk=0)


def _raw(eng, masks, S, Hm, Wm, a, out, changed, boxes, area):
    from revisit_anything_amd.engine import _ptr

    eng._stream()
    return eng.lib.segvlad_mask_regions(eng._h, _ptr(masks), S, Hm, Wm, a, _ptr(out), _ptr(changed), _ptr(boxes), _ptr(area))


def test_in_place_and_two_calls(eng):
    H, W = 97, 131
    names, masks = RR.table(H, W)
    S = len(masks)
    for a in (7, 17):
        md = torch.tensor(masks).to(eng.device)
        first = eng.mask_regions(md, a)
        second = eng.mask_regions(md, a)
        assert all(first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes() for k in first)
        chg = torch.zeros(S, dtype=torch.int32, device=eng.device)
        box = torch.zeros((S, 4), dtype=torch.int32, device=eng.device)
        area = torch.zeros(S, dtype=torch.int64, device=eng.device)
        eng._check(_raw(eng, md, S, H, W, a, md, chg, box, area), "mask_regions")     # masks_out == masks
        _compare(("in place", a), {"masks": md, "changed": chg, "boxes": box, "area": area}, RR.expected(H, W, a), names)
        assert torch.equal(md, first["masks"])


# ---- 3. the raw entry: pointer kinds, NULL outputs, S == 0 -----------------------------------------------------------------------
def test_host_pointers_equal_device_pointers(eng):
    H, W = 33, 65
    names, masks = RR.table(H, W)
    S = len(masks)
    for a in (1, 7):
        want = RR.expected(H, W, a)
        out, chg, box, area = np.full((S, H, W), SENTINEL, np.uint8), np.full(S, -7, np.int32), np.full((S, 4), -7, np.int32), np.full(S, -7, np.int64)
        eng._check(_raw(eng, masks, S, H, W, a, out, chg, box, area), "mask_regions")          # every pointer on the host
        assert np.array_equal(out, want[0]) and np.array_equal(chg, want[1]) and np.array_equal(box, want[2]) and np.array_equal(area, want[3])
        inplace = masks.copy()
        eng._check(_raw(eng, inplace, S, H, W, a, inplace, None, None, None), "mask_regions")  # in place on the host, no optional output
        assert np.array_equal(inplace, want[0])
        # mixed: device masks, host flags; and the NULL outputs one by one
        md = torch.tensor(masks).to(eng.device)
        od = torch.full((S, H, W), SENTINEL, dtype=torch.uint8, device=eng.device)
        chg = np.full(S, -7, np.int32)
        eng._check(_raw(eng, md, S, H, W, a, od, chg, None, None), "mask_regions")
        assert np.array_equal(od.cpu().numpy(), want[0]) and np.array_equal(chg, want[1])
        bd = torch.full((S, 4), -7, dtype=torch.int32, device=eng.device)
        eng._check(_raw(eng, md, S, H, W, a, od, None, bd, None), "mask_regions")
        eng.synchronize()
        assert np.array_equal(bd.cpu().numpy(), want[2])
        ad = torch.full((S,), -7, dtype=torch.int64, device=eng.device)
        eng._check(_raw(eng, md, S, H, W, a, od, None, None, ad), "mask_regions")
        eng.synchronize()
        assert np.array_equal(ad.cpu().numpy(), want[3])
    got = eng.mask_regions(masks != 0, 7, want_boxes=False, want_area=False)                    # host bool through the engine
    assert sorted(got) == ["changed", "masks"]
    _compare("host bool", got, RR.clean_batch(masks != 0, 7), names)


def test_no_masks(eng):
    got = eng.mask_regions(torch.zeros((0, 64, 96), dtype=torch.uint8, device=eng.device), 5)
    assert tuple(got["masks"].shape) == (0, 64, 96) and got["changed"].shape[0] == 0 and tuple(got["boxes"].shape) == (0, 4) and got["area"].shape[0] == 0
    out = torch.full((4,), SENTINEL, dtype=torch.uint8, device=eng.device)
    chg = torch.full((2,), -7, dtype=torch.int32, device=eng.device)
    eng._check(_raw(eng, None, 0, 64, 96, 5, None, chg, None, None), "mask_regions")
    eng._check(_raw(eng, out, 0, 2, 2, 5, out, chg, None, None), "mask_regions")
    eng.synchronize()
    assert (out == SENTINEL).all() and (chg == -7).all()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from revisit_anything_amd import synth
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SEGVLAD_ERR_LIMIT, SEGVLAD_ERR_STATE, SegVLADError

    H, W = 33, 65
    names, masks = RR.table(H, W)
    S = len(masks)
    md = torch.tensor(masks).to(eng.device)
    buf = torch.full((2 * S * H * W,), SENTINEL, dtype=torch.uint8, device=eng.device)
    od = buf[:S * H * W]
    one = torch.zeros(1, dtype=torch.uint8, device=eng.device)

    def code(rc):
        with pytest.raises(SegVLADError) as e:
            eng._check(rc, "refused")
        return e.value.code

    for args in ((md, -1, H, W, 5, od), (md, S, 0, W, 5, od), (md, S, H, -3, 5, od), (md, S, H, W, -1, od), (None, S, H, W, 5, od), (md, S, H, W, 5, None)):
        assert code(_raw(eng, *args, None, None, None)) == SEGVLAD_ERR_ARG, args[1:5]
    # masks_out overlaps masks without being masks: one byte in, and one mask in
    buf[:S * H * W] = md.reshape(-1)
    for shift in (1, H * W):
        assert code(_raw(eng, buf[:S * H * W], S, H, W, 5, buf[shift:shift + S * H * W], None, None, None)) == SEGVLAD_ERR_ARG
    assert code(_raw(eng, buf[H * W:(S + 1) * H * W], S, H, W, 5, buf[:S * H * W], None, None, None)) == SEGVLAD_ERR_ARG
    eng.synchronize()
    assert torch.equal(buf[:S * H * W], md.reshape(-1)) and (buf[S * H * W:] == SENTINEL).all()
    # 2^31 pixels: refused from the shape alone (the one byte behind the pointers is never read); 2^31 - 1 would be accepted
    assert code(_raw(eng, one, 1, 32768, 65536, 5, one, None, None, None)) == SEGVLAD_ERR_LIMIT
    with pytest.raises(SegVLADError) as e:
        eng.mask_regions(torch.zeros((0, 65536, 65536), dtype=torch.uint8, device=eng.device), 5)
    assert e.value.code == SEGVLAD_ERR_LIMIT
    with pytest.raises(TypeError):
        eng.mask_regions(torch.zeros(1, 4, 4, dtype=torch.float32, device=eng.device), 5)
    with pytest.raises(ValueError):
        eng.mask_regions(torch.zeros(4, dtype=torch.uint8, device=eng.device), 5)
    # an open describe
    Hd, Wd, Hi, Wi, K, D = 64, 96, 126, 150, 8, 64
    Cc = synth.make_vocab(K, D, seed=700)
    eng.set_vocab(Cc)
    N = (Hi // 14) * (Wi // 14)
    sizes = (4, 6)
    tok = torch.tensor(np.stack([synth.make_tokens(Cc, N, seed=701 + b, noise=0.2) for b in range(len(sizes))])).to(eng.device)
    dm = torch.tensor(np.concatenate([synth.make_blob_masks(s, Hd, Wd, seed=750 + b) for b, s in enumerate(sizes)]).astype(np.uint8)).to(eng.device)
    so = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    h = eng.describe_begin(dm, tok, so, Hi, Wi, 14, 3, pca=False)
    with pytest.raises(SegVLADError) as e:
        eng.mask_regions(md, 5)
    assert e.value.code == SEGVLAD_ERR_STATE
    out = eng.describe_end(h, None, None)["out"]
    assert torch.isfinite(out).all()
    _compare("after the open describe", eng.mask_regions(md, 7), RR.expected(H, W, 7), names)   # and the context is free again


# ---- 5. the generator ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), k
            else:
                assert x[k] == y[k], k


@pytest.mark.parametrize("c", range(len(regions_stub.CASES)))
def test_the_generator_cleans_on_the_device(eng, monkeypatch, c):
    from revisit_anything_amd import producers as pr

    H, W, pps, ppb, kw, seed = regions_stub.CASES[c]
    img = np.zeros((H, W, 3), np.uint8)
    host = regions_stub.stubbed_generator(seed, pps, ppb, kw).generate(img)
    host_rle = regions_stub.stubbed_generator(seed, pps, ppb, kw, output_mode="uncompressed_rle").generate(img)
    assert len(host) >= 3

    def refuse(*a, **k):
        raise AssertionError("the host path was called")

    with monkeypatch.context() as mp:
        mp.setattr(pr, "clean_small_regions", refuse)
        mp.setattr(pr, "remove_small_regions", refuse)
        got = regions_stub.stubbed_generator(seed, pps, ppb, kw, device=eng.device, regions_engine=eng).generate(img)
        _same(got, host)
        # run-length mode with rle_engine alone: it cleans too, and neither the host cleaner nor the host encoder runs
        from revisit_anything_amd.rle import RleMasks

        mp.setattr(RleMasks, "from_dense", refuse)
        got = regions_stub.stubbed_generator(seed, pps, ppb, kw, device=eng.device, output_mode="uncompressed_rle", rle_engine=eng).generate(img)
        assert got == host_rle
