"""Run-length masks on the device (csrc/rle_kernels.hip): segvlad_incidence_rle and segvlad_rle_decode over the mask branch's shape
table (tests/mask_branch_cases.py), over masks built for the run walk, over malformed batches through the raw C ABI, and through
SegVLADPipeline.describe.  Every comparison is exact: incidence bits bit for bit against the oracle AND byte for byte against the
dense kernels, centroids as fp64 values (NaN = NaN) and as bytes, decoded masks byte for byte.

The run-length kernel keeps a mask as a COLUMN-major bitmap, Wm * ceil(Hm / 32) * 4 bytes, bounded by 150 KiB: of the table,
`unfused_lds_152k` (1216 x 1024) and `fused_lds_150k` (1200 x 1024: 38 words per column as well) are both 152 KiB there, so both
are refused with SEGVLAD_ERR_LIMIT and both take rle_decode + the dense entry -- and its column windows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from conftest import engine_scope

import mask_branch_cases as T

pytestmark = pytest.mark.gpu

KIB = 1024
GEOMETRIES = [(64, 96, 126, 150)] + [(Hm, 40, 70, 84) for Hm in (31, 32, 33, 64, 65)]


@pytest.fixture(scope=engine_scope)
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


def _O():
    from oracle import segvlad_oracle as O

    return O


def _R():
    from revisit_anything_amd.rle import RleMasks

    return RleMasks


@functools.lru_cache(maxsize=None)
def _rle(name):
    return _R().from_dense(T.build_masks(name)[0])


def _refused(c):
    return c["Wm"] * ((c["Hm"] + 31) // 32) * 4 > 150 * KIB


def _limit(call):
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    with pytest.raises(SegVLADError) as e:
        call()
    assert e.value.code == SEGVLAD_ERR_LIMIT, e.value
    return str(e.value)


def _check_bits_and_centroids(tag, bits, cent, inc, cent_ref):
    """bits int64 [S, nw] and cent fp64 [S, 2] (host arrays) against bool [S, N] and fp64 [S, 2]"""
    S, N = inc.shape
    nw = (N + 63) // 64
    assert bits.shape == (S, nw) and cent.shape == (S, 2), tag
    every = _O().unpack_bits_u64(bits.view(np.uint64), nw * 64)
    wrong = np.argwhere(every[:, :N] != inc)
    assert len(wrong) == 0, (tag, "first wrong (mask, token):", wrong[:5].tolist())
    assert not every[:, N:].any(), (tag, "pad bits set")
    assert np.array_equal(cent, cent_ref, equal_nan=True), (tag, np.argwhere(~((cent == cent_ref) | np.isnan(cent_ref)))[:5].tolist())


def _oracle_of(dense, H, W, patch=14):
    import warnings

    O = _O()
    inc = O.incidence(dense.astype(np.uint8), H, W, patch)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (the mean of an empty mask's coordinates: NaN, as in the reference)
        cent = np.asarray(O.mask_centroids(list(dense.astype(np.uint8))), np.float64).reshape(len(dense), 2)
    return inc, cent


# ---- 1. the shape table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.INC_NAMES)
def test_incidence_rle_equals_the_oracle_and_the_dense_kernels(eng, name):
    c = T.INC_BY_NAME[name]
    H, W, patch = c["H"], c["W"], c["patch"]
    m = T.build_masks(name)[0]
    inc, cent_ref = T.incidence_reference(name)
    rle = _rle(name)
    dev = rle.to(eng.device)
    md = torch.tensor(np.array(m)).to(eng.device)
    dense_bits, dense_cent = (x.cpu().numpy() for x in eng.incidence_centroids(md, H, W, patch))
    if _refused(c):
        assert name in ("unfused_lds_152k", "fused_lds_150k")
        for r in (dev, rle):
            msg = _limit(lambda: eng.incidence_rle(r, H, W, patch))
            assert "segvlad_rle_decode" in msg and "segvlad_incidence_centroids" in msg
            small = _rle("fused_ranges_small")            # the next call on the same context succeeds
            cs = T.INC_BY_NAME["fused_ranges_small"]
            b, ce = eng.incidence_rle(small, cs["H"], cs["W"], cs["patch"])
            _check_bits_and_centroids("after " + name, b.cpu().numpy(), ce.cpu().numpy(), *T.incidence_reference("fused_ranges_small"))
        b, ce = eng.incidence_centroids(eng.rle_decode(dev), H, W, patch)
        _check_bits_and_centroids(name, b.cpu().numpy(), ce.cpu().numpy(), inc, cent_ref)
        assert b.cpu().numpy().tobytes() == dense_bits.tobytes() and ce.cpu().numpy().tobytes() == dense_cent.tobytes()
        return
    for tag, r in (("device", dev), ("host", rle)):
        bits, cent, n_bad = eng.incidence_rle(r, H, W, patch, want_bad=True)
        assert n_bad is eng.rle_n_bad and n_bad.is_cuda
        bits, cent = bits.cpu().numpy(), cent.cpu().numpy()
        _check_bits_and_centroids((name, tag), bits, cent, inc, cent_ref)
        assert bits.tobytes() == dense_bits.tobytes(), (name, tag)
        assert cent.tobytes() == dense_cent.tobytes(), (name, tag)
        assert int(n_bad.item()) == 0, (name, tag)
    only_bits, none = eng.incidence_rle(dev, H, W, patch, centroids=False)
    assert none is None and only_bits.cpu().numpy().tobytes() == dense_bits.tobytes()


def test_no_masks_write_nothing(eng):
    """S == 0 through the raw C ABI: both calls return OK and leave pre-filled outputs alone"""
    from revisit_anything_amd.engine import _ptr

    c = T.INC_BY_NAME["s0"]
    assert len(_rle("s0")) == 0
    offs = torch.zeros(1, dtype=torch.int64, device=eng.device)
    counts = torch.zeros(4, dtype=torch.int32, device=eng.device)
    bits = torch.full((4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=eng.device)
    cent = torch.full((4,), 7.5, dtype=torch.float64, device=eng.device)
    out = torch.full((64,), 9, dtype=torch.uint8, device=eng.device)
    n_bad = torch.full((1,), 3, dtype=torch.int32, device=eng.device)
    eng._stream()
    eng._check(eng.lib.segvlad_incidence_rle(eng._h, _ptr(counts), _ptr(offs), 0, c["Hm"], c["Wm"], c["H"], c["W"], c["patch"], _ptr(bits),
                                             _ptr(cent), _ptr(n_bad)), "incidence_rle")
    eng._check(eng.lib.segvlad_rle_decode(eng._h, _ptr(counts), _ptr(offs), 0, c["Hm"], c["Wm"], _ptr(out), _ptr(n_bad)), "rle_decode")
    eng.synchronize()
    assert (bits == 0x5A5A5A5A5A5A5A5A).all() and (cent == 7.5).all() and (out == 9).all() and int(n_bad.item()) == 3
    b, ce = eng.incidence_rle(_rle("s0"), c["H"], c["W"], c["patch"])
    assert b.shape == (0, 2) and ce.shape == (0, 2) and eng.rle_decode(_rle("s0")).shape == (0, c["Hm"], c["Wm"])


# ---- 2. decode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.INC_NAMES)
def test_rle_decode_equals_the_masks(eng, name):
    m = T.build_masks(name)[0]
    want = (m != 0).astype(np.uint8)
    rle = _rle(name)
    out, n_bad = eng.rle_decode(rle.to(eng.device), want_bad=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == want.shape
    got = out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:5].tolist())
    assert int(n_bad.item()) == 0
    if m.size <= 1 << 20:      # host runs, staged by the library
        assert eng.rle_decode(rle).cpu().numpy().tobytes() == want.tobytes(), name


def test_rle_decode_into_host_and_unaligned_memory(eng):
    """The raw call: a host output array, and a device output one byte off a word (the byte stores instead of the wide ones)"""
    from revisit_anything_amd.engine import _ptr

    name = "fused_ranges_small"
    want = (T.build_masks(name)[0] != 0).astype(np.uint8)
    rle = _rle(name)
    c, o = rle.arrays()
    host = np.full(want.shape, 9, np.uint8)
    eng._stream()
    eng._check(eng.lib.segvlad_rle_decode(eng._h, _ptr(c), _ptr(o), len(rle), rle.Hm, rle.Wm, _ptr(host), None), "rle_decode")
    assert host.tobytes() == want.tobytes()
    buf = torch.full((want.size + 8,), 9, dtype=torch.uint8, device=eng.device)
    view = buf[1:1 + want.size]
    eng._check(eng.lib.segvlad_rle_decode(eng._h, _ptr(c), _ptr(o), len(rle), rle.Hm, rle.Wm, view.data_ptr(), None), "rle_decode")
    got = buf.cpu().numpy()
    assert got[1:1 + want.size].tobytes() == want.tobytes() and got[0] == 9 and (got[1 + want.size:] == 9).all()


# ---- 3. masks built for the run walk ---------------------------------------------------------------------------------------------
def _with_zero_runs(counts, rng, pairs):
    """The same mask with `pairs` pairs of zero-length runs inserted (a pair keeps the parity of the runs behind it)"""
    out = [int(v) for v in counts]
    for _ in range(pairs):
        k = int(rng.integers(1, len(out) + 1))
        out[k:k] = [0, 0]
    return out


@functools.lru_cache(maxsize=None)
def _run_masks(Hm, Wm):
    """(RleMasks, dense bool [S, Hm, Wm], names)"""
    from revisit_anything_amd import synth
    from revisit_anything_amd.engine import RLE_CHUNK_RUNS as CH

    RleMasks = _R()
    P = Hm * Wm
    rng = np.random.Generator(np.random.PCG64(7700 + Hm))
    flat, names = [], []              # column-major pixel vectors

    def add(name, f):
        names.append(name)
        flat.append(np.asarray(f, bool))

    p = np.arange(P)
    add("alternate", p & 1)                                  # P runs
    add("alternate_from_one", (p & 1) == 0)                  # P + 1 runs, the first of length 0
    add("checkerboard", ((p // Hm) + (p % Hm)) & 1)
    add("columns_then_mid", (p >= Hm // 2 + 3) & (p < 4 * Hm + Hm // 3))
    add("three_whole_columns", (p >= 2 * Hm) & (p < 5 * Hm))
    add("one_whole_column", (p >= 7 * Hm) & (p < 8 * Hm))
    add("ends_on_column_ends", ((p % Hm) >= 5) & ((p // Hm) % 3 == 0))
    add("starts_on_column_starts", ((p % Hm) < Hm - 4) & ((p // Hm) % 2 == 1))
    add("last_pixel", p == P - 1)
    add("first_pixel", p == 0)
    add("all_but_the_ends", (p > 0) & (p < P - 1))
    half = rng.permutation(P // 2)                           # isolated pixels: odd positions, never neighbours
    ladder = sorted({k * CH // 2 + d for k in range(1, 9) for d in (-1, 0, 1)})
    assert {k * CH + d for k in range(1, 5) for d in (-1, 0, 1)} <= set(ladder)
    for r in ladder:
        if r <= P // 2:
            f = np.zeros(P, bool)
            f[2 * half[:r] + 1] = True
            add("isolated_%d" % r, f)
    dense = np.stack(flat).reshape(len(flat), Wm, Hm).transpose(0, 2, 1)
    base = RleMasks.from_dense(dense)
    # zero-length runs in the middle: a blob mask's runs with a few pairs of them, with more than two chunks of them, and the
    # alternating mask with one pair per chunk
    blob = synth.make_blob_masks(1, Hm, Wm, seed=Hm)[0]
    bc = RleMasks.from_dense(blob).to_sam()[0]["counts"]
    extra, extra_dense = [], []
    for nm, cnts, d in (("blob_zero_runs", _with_zero_runs(bc, rng, 5), blob), ("blob_many_zero_runs", _with_zero_runs(bc, rng, CH + 40), blob),
                        ("alternate_zero_runs", _with_zero_runs(base.to_sam()[0]["counts"], rng, 2 * P // CH + 3), dense[0])):
        names.append(nm)
        extra.append({"size": [Hm, Wm], "counts": cnts})
        extra_dense.append(d)
    rle = RleMasks.concat([base, RleMasks.from_sam(extra)])
    dense = np.concatenate([dense, np.stack(extra_dense)])
    assert np.array_equal(rle.to_dense(), dense)
    return rle, dense, names


@pytest.mark.parametrize("Hm,Wm,H,W", GEOMETRIES, ids=["%dx%d" % g[:2] for g in GEOMETRIES])
def test_run_structures(eng, Hm, Wm, H, W):
    from revisit_anything_amd.engine import RLE_CHUNK_RUNS as CH

    rle, dense, names = _run_masks(Hm, Wm)
    c, o = rle.arrays()
    runs = np.diff(o)
    assert runs.max() >= Hm * Wm and (CH == 512)
    if (Hm, Wm) == (64, 96):      # the ladder reaches four chunks, and run counts on both sides of every chunk boundary up to there
        assert {"isolated_%d" % (k * CH + d) for k in range(1, 5) for d in (-1, 0, 1)} <= set(names)
    inc, cent_ref = _oracle_of(dense, H, W)
    for tag, r in (("device", rle.to(eng.device)), ("host", rle)):
        bits, cent, n_bad = eng.incidence_rle(r, H, W, 14, want_bad=True)
        bits, cent = bits.cpu().numpy(), cent.cpu().numpy()
        S, N = inc.shape
        every = _O().unpack_bits_u64(bits.view(np.uint64), bits.shape[1] * 64)
        bad = sorted({names[s] for s in np.argwhere(every[:, :N] != inc)[:, 0]})
        assert not bad, (tag, "masks with wrong bits:", bad)
        _check_bits_and_centroids((Hm, Wm, tag), bits, cent, inc, cent_ref)
        assert int(n_bad.item()) == 0
        got = eng.rle_decode(r).cpu().numpy()
        bad = sorted({names[s] for s in np.argwhere(got != dense.astype(np.uint8))[:, 0]})
        assert not bad, (tag, "masks decoded wrong:", bad)
    db, dc = eng.incidence_centroids(torch.tensor(dense.astype(np.uint8)).to(eng.device), H, W, 14)
    assert db.cpu().numpy().tobytes() == bits.tobytes() and dc.cpu().numpy().tobytes() == cent.tobytes()


# ---- 4. malformed masks, through the raw C ABI -----------------------------------------------------------------------------------
def _clipped_decode(lists, Hm, Wm):
    """rle_to_mask with the runs clipped at Hm * Wm and the pixels they do not reach left zero; (masks, which are malformed)"""
    P = Hm * Wm
    out = np.zeros((len(lists), Hm, Wm), np.uint8)
    bad = []
    for s, runs in enumerate(lists):
        flat = np.zeros(P, np.uint8)
        pos = 0
        for k, n in enumerate(runs):
            if k & 1:
                flat[min(pos, P):min(pos + int(n), P)] = 1
            pos += int(n)
        bad.append(pos != P)
        out[s] = flat.reshape(Wm, Hm).T
    return out, bad


def test_malformed_masks_are_clipped_counted_and_leave_the_others_alone(eng):
    from revisit_anything_amd import synth
    from revisit_anything_amd.engine import _ptr

    Hm, Wm, H, W = 64, 96, 126, 150
    P = Hm * Wm
    good = _R().from_dense(synth.make_blob_masks(2, Hm, Wm, seed=41))
    g0, g1 = (r["counts"] for r in good.to_sam())
    big = 0xFFFFFFFF
    lists = [
        [100, 300, 1000, 77, 50],                                  # short: 1527 pixels
        g0,
        [10, 20, P, 400, 9],                                       # long: the third run crosses the end, two more follow
        [],                                                        # no runs
        [5, 60, 3, big, 11, 12],                                   # 0xFFFFFFFF as a ones-run
        g1,
        [200, 1000, 0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF0, 7, P],   # the sums pass 2^32 (and 2^33, 2^34): nothing may wrap back
    ]
    want, bad = _clipped_decode(lists, Hm, Wm)
    assert bad == [True, False, True, True, True, False, True]
    assert np.array_equal(want[1], good.to_dense()[0]) and np.array_equal(want[5], good.to_dense()[1]) and not want[3].any()
    assert want[4].sum() == 60 + (P - 68) and want[6].sum() == 1000 and want[2].sum() == 20 and want[0].sum() == 377
    inc, cent_ref = _oracle_of(want, H, W)
    counts = np.array([v for runs in lists for v in runs], np.uint32)
    offs = np.concatenate([[0], np.cumsum([len(runs) for runs in lists])]).astype(np.int64)
    S, N = inc.shape
    nw = (N + 63) // 64
    for tag, (cc, oo) in (("host", (counts, offs)), ("device", (torch.tensor(counts.view(np.int32)).to(eng.device), torch.tensor(offs).to(eng.device)))):
        bits = torch.full((S, nw), -1, dtype=torch.int64, device=eng.device)
        cent = torch.full((S, 2), -1.0, dtype=torch.float64, device=eng.device)
        masks = torch.full((S, Hm, Wm), 9, dtype=torch.uint8, device=eng.device)
        n_bad = torch.zeros(2, dtype=torch.int32, device=eng.device)
        eng._stream()
        # (a guarded context -- the suite's default -- checks every fence at the end of each call and fails it when one is trampled)
        eng._check(eng.lib.segvlad_incidence_rle(eng._h, _ptr(cc), _ptr(oo), S, Hm, Wm, H, W, 14, _ptr(bits), _ptr(cent), _ptr(n_bad[:1])),
                   "incidence_rle")
        eng._check(eng.lib.segvlad_rle_decode(eng._h, _ptr(cc), _ptr(oo), S, Hm, Wm, _ptr(masks), n_bad[1:].data_ptr()), "rle_decode")
        eng.synchronize()
        assert n_bad.cpu().tolist() == [5, 5], tag
        _check_bits_and_centroids(tag, bits.cpu().numpy(), cent.cpu().numpy(), inc, cent_ref)
        assert masks.cpu().numpy().tobytes() == want.tobytes(), tag
    # the dense kernels on the clipped masks: the same bytes
    db, dc = eng.incidence_centroids(torch.tensor(want).to(eng.device), H, W, 14)
    assert db.cpu().numpy().tobytes() == bits.cpu().numpy().tobytes() and dc.cpu().numpy().tobytes() == cent.cpu().numpy().tobytes()
    # the arguments the entry refuses
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    host_bad = (C.c_uint32 * 1)(0)
    for call in (lambda: eng.lib.segvlad_incidence_rle(eng._h, _ptr(counts), _ptr(offs), S, Hm, Wm, H, W, 14, _ptr(bits), None, C.cast(host_bad, C.c_void_p)),
                 lambda: eng.lib.segvlad_incidence_rle(eng._h, _ptr(counts), _ptr(offs[::-1].copy()), S, Hm, Wm, H, W, 14, _ptr(bits), None, None),
                 lambda: eng.lib.segvlad_incidence_rle(eng._h, _ptr(counts), _ptr(offs), S, Hm, 0, H, W, 14, _ptr(bits), None, None),
                 lambda: eng.lib.segvlad_rle_decode(eng._h, _ptr(counts), None, S, Hm, Wm, _ptr(masks), None)):
        with pytest.raises(SegVLADError) as e:
            eng._check(call(), "refused")
        assert e.value.code == SEGVLAD_ERR_ARG


# ---- 5. the pipeline -------------------------------------------------------------------------------------------------------------
def _pipeline_batch(eng, sizes, Hm, Wm, H, W, seed, K=8, D=64):
    from revisit_anything_amd import synth

    Cc = synth.make_vocab(K, D, seed=seed)
    eng.set_vocab(Cc)
    N = (H // 14) * (W // 14)
    tok = torch.tensor(np.stack([synth.make_tokens(Cc, N, seed=seed + 1 + b, noise=0.2) for b in range(len(sizes))])).to(eng.device)
    masks = np.concatenate([synth.make_blob_masks(s, Hm, Wm, seed=seed + 50 + b) for b, s in enumerate(sizes)]).astype(np.uint8)
    return tok, masks, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


@pytest.mark.parametrize("order", [0, 3])
@pytest.mark.parametrize("pca", [False, True])
def test_pipeline_describe_takes_run_length_masks(eng, order, pca):
    from revisit_anything_amd import synth
    from revisit_anything_amd.pipeline import SegVLADPipeline

    Hm, Wm, H, W, K, D, P = 64, 96, 126, 150, 8, 64, 16
    tok, masks, so = _pipeline_batch(eng, (1, 3, 7, 12), Hm, Wm, H, W, seed=300)
    if pca:
        eng.pca_set(*synth.make_pca_model(K * D, P, seed=5300), whiten=True)
    pipe = SegVLADPipeline(eng, H, W, 14, order=order, use_pca=pca)
    want = pipe.describe(tok, torch.tensor(masks).to(eng.device), so)
    assert tuple(want.shape) == (23, P if pca else K * D) and torch.isfinite(want).all()
    rle = _R().from_dense(masks)
    assert torch.equal(pipe.describe(tok, rle.to(eng.device), so), want)
    assert torch.equal(pipe.describe(tok, rle, so), want)                       # host runs
    # an all-zero mask: the same ValueError from both forms
    empty = masks.copy()
    empty[5] = 0
    if order:
        for form in (torch.tensor(empty).to(eng.device), _R().from_dense(empty).to(eng.device)):
            with pytest.raises(ValueError, match="empty mask"):
                pipe.describe(tok, form, so)
            torch.cuda.synchronize()
    assert torch.equal(pipe.describe(tok, rle.to(eng.device), so), want)       # and the context goes on


def test_pipeline_describe_inflates_masks_above_the_bound(eng):
    """1216 x 1024 masks: incidence_rle reports SEGVLAD_ERR_LIMIT, the pipeline decodes on the device and takes the dense entry"""
    from revisit_anything_amd.pipeline import SegVLADPipeline

    Hm, Wm, H, W = 1216, 1024, 224, 322
    tok, masks, so = _pipeline_batch(eng, (2, 3), Hm, Wm, H, W, seed=400)
    rle = _R().from_dense(masks).to(eng.device)
    _limit(lambda: eng.incidence_rle(rle, H, W))
    pipe = SegVLADPipeline(eng, H, W, 14, order=2, use_pca=False)
    assert torch.equal(pipe.describe(tok, rle, so), pipe.describe(tok, torch.tensor(masks).to(eng.device), so))


# ---- 6. an open describe ---------------------------------------------------------------------------------------------------------
def test_rle_entries_refuse_while_a_describe_is_open(eng):
    from revisit_anything_amd._lib import SEGVLAD_ERR_STATE, SegVLADError

    Hm, Wm, H, W = 64, 96, 126, 150
    tok, masks, so = _pipeline_batch(eng, (4, 6, 5), Hm, Wm, H, W, seed=500)
    md = torch.tensor(masks).to(eng.device)
    rle = _R().from_dense(masks).to(eng.device)
    bits, cent = eng.incidence_rle(rle, H, W)
    adj, _ = eng.adjacency_flagged(cent, so, 3, device_flags=True)
    ref = eng.seg_vlad(tok, bits, so, adj)["out"]
    h = eng.describe_begin(md, tok, so, H, W, 14, 3, pca=False)
    for call in (lambda: eng.incidence_rle(rle, H, W), lambda: eng.rle_decode(rle)):
        with pytest.raises(SegVLADError) as e:
            call()
        assert e.value.code == SEGVLAD_ERR_STATE
    assert torch.equal(eng.describe_end(h, None, None)["out"], ref)
    b2, c2 = eng.incidence_rle(rle, H, W)                                        # and the context is free again
    assert torch.equal(b2, bits) and torch.equal(c2.view(torch.int64), cent.view(torch.int64))
