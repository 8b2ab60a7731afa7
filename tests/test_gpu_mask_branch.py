"""The mask branch on the device, over the table of tests/mask_branch_cases.py (qualified on the CPU by
tests/test_mask_branch_cases.py): segvlad_incidence, segvlad_incidence_centroids and segvlad_mask_centroids against the oracle's
bits and centroids, segvlad_adjacency and segvlad_adjacency_flagged against the exact empty-circle rule -- through the engine and so
through the C ABI.  Every comparison is exact: bits bit for bit, centroids as fp64 bit patterns, adjacency blocks byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch
from conftest import engine_scope

import mask_branch_cases as T

pytestmark = pytest.mark.gpu


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


# ---- incidence and centroids ------------------------------------------------------------------------------------------------
def _device_masks(eng, name):
    """The case's masks on the device, at the byte offset the case asks for (a contiguous view: the engine passes it through)"""
    c = T.INC_BY_NAME[name]
    m = T.build_masks(name)[0]
    buf = torch.zeros(c["offset"] + m.size + 16, dtype=torch.uint8, device=eng.device)
    buf[c["offset"]:c["offset"] + m.size] = torch.tensor(m.reshape(-1)).to(eng.device)
    md = buf[c["offset"]:c["offset"] + m.size].view(m.shape)
    assert md.is_contiguous() and md.data_ptr() % 16 == c["offset"] % 16 and md.to(torch.uint8).contiguous().data_ptr() == md.data_ptr()
    return md


def _mask_calls(eng, name, masks):
    """(bits of segvlad_incidence, bits and centroids of segvlad_incidence_centroids, centroids of segvlad_mask_centroids)"""
    c = T.INC_BY_NAME[name]
    a = eng.incidence(masks, c["H"], c["W"], c["patch"])
    b, cb = eng.incidence_centroids(masks, c["H"], c["W"], c["patch"])
    cc = eng.mask_centroids(masks)
    return [x.cpu().numpy() for x in (a, b, cb, cc)]


def _same(xs, ys):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(xs, ys))


def _check_against_oracle(name, got):
    c = T.INC_BY_NAME[name]
    inc, cent = T.incidence_reference(name)
    N = inc.shape[1]
    nw = (N + 63) // 64
    bits_a, bits_b, cent_b, cent_c = got
    S = len(inc)
    assert bits_a.shape == bits_b.shape == (S, nw) and cent_b.shape == cent_c.shape == (S, 2)
    assert bits_a.tobytes() == bits_b.tobytes(), name
    if S == 0:
        return
    every = _O().unpack_bits_u64(bits_a.view(np.uint64), nw * 64)
    wrong = np.argwhere(every[:, :N] != inc)
    assert len(wrong) == 0, (name, "first wrong (mask, token):", wrong[:5].tolist())
    assert not every[:, N:].any(), (name, "pad bits set")
    empty = np.isnan(cent).all(1)
    for what, g in (("incidence_centroids", cent_b), ("mask_centroids", cent_c)):
        assert np.isnan(g[empty]).all(), (name, what)
        assert g[~empty].tobytes() == cent[~empty].tobytes(), (name, what, np.argwhere(g[~empty] != cent[~empty])[:5].tolist())
    if c["specials"]:
        assert empty.sum() == 1 and empty[T.build_masks(name)[1]["zeros"]]


@pytest.mark.parametrize("name", T.INC_NAMES)
def test_incidence_and_centroids_equal_the_oracle(eng, name):
    facts = T.launch_facts(T.INC_BY_NAME[name])
    md = _device_masks(eng, name)
    mh = np.array(T.build_masks(name)[0])
    dev = _mask_calls(eng, name, md)
    _check_against_oracle(name, dev)
    host = _mask_calls(eng, name, mh)        # (staged by the library: the copy is aligned, so the misaligned case's host form is fused)
    assert _same(dev, host), name
    # scratch reuse: a case of another branch on the same context, from host arrays (the staging buffers move), then the same calls again
    other = "unfused_wm_down_gridy2" if facts["fused"] else "fused_n1530"
    _check_against_oracle(other, _mask_calls(eng, other, np.array(T.build_masks(other)[0])))
    assert _same(dev, _mask_calls(eng, name, md)), name
    assert _same(host, _mask_calls(eng, name, mh)), name


def test_no_masks_is_a_call_that_writes_nothing(eng):
    c = T.INC_BY_NAME["s0"]
    for masks in (np.zeros((0, c["Hm"], c["Wm"]), np.uint8), torch.zeros((0, c["Hm"], c["Wm"]), dtype=torch.uint8, device=eng.device)):
        a, b, cb, cc = _mask_calls(eng, "s0", masks)
        assert a.shape == b.shape == (0, 2) and cb.shape == cc.shape == (0, 2)


# ---- adjacency --------------------------------------------------------------------------------------------------------------
def _raw_counts(eng, cat, offs, order):
    """segvlad_adjacency's counter word (what check_empty reads): low 16 bits NaN centroids, bits 16.. degenerate images"""
    from revisit_anything_amd.engine import _ptr

    so = np.ascontiguousarray(offs, np.int32)
    sizes = (so[1:] - so[:-1]).astype(np.int64)
    out = torch.empty(int((sizes * sizes).sum()), dtype=torch.uint8, device=eng.device)
    n_bad = (C.c_uint32 * 1)(0xFFFFFFFF)
    eng._stream()
    eng._check(eng.lib.segvlad_adjacency(eng._h, _ptr(cat), _ptr(so), len(so) - 1, int(order), _ptr(out), C.cast(n_bad, C.c_void_p)),
               "adjacency")
    return int(n_bad[0]), out.cpu().numpy()


def _blocks(adj, images):
    _, _, starts = T.pack_centroids(images)
    return [adj[starts[i]:starts[i + 1]].reshape(len(img), len(img)) for i, img in enumerate(images)]


def _run_batch(eng, images, order):
    cat, offs, _ = T.pack_centroids(images)
    adj, flags = eng.adjacency_flagged(cat, offs, order)
    adj = adj.cpu().numpy()
    assert adj.tobytes() == eng.adjacency(cat, offs, order).cpu().numpy().tobytes()
    return adj, np.asarray(flags).copy()


CASES = [(n, o) for n in T.ADJ_NAMES for o in T.adjacency_batches()[n]["orders"]]


@pytest.mark.parametrize("name,order", CASES, ids=["%s-o%d" % c for c in CASES])
def test_adjacency_equals_the_exact_rule(eng, name, order):
    from revisit_anything_amd._lib import SegVLADDegenerateError

    b = T.adjacency_batches()[name]
    images = b["images"]
    classes = [cl for cl, _, _ in T.batch_classes(name)]
    want = T.adjacency_reference(name, order)
    adj, flags = _run_batch(eng, images, order)
    assert len(flags) == len(images) and set(np.unique(adj)) <= {0, 1}
    got = _blocks(adj, images)
    for i, (cl, blk) in enumerate(zip(classes, got)):
        if cl in ("generic", "small", "empty"):
            wrong = np.argwhere(blk.astype(bool) != want[i])
            assert len(wrong) == 0, (name, order, i, len(images[i]), "first wrong (row, col):", wrong[:5].tolist())
            assert flags[i] == 0, (name, order, i, int(flags[i]))
        elif cl == "degenerate":      # reported, and (integer coordinates: exact arithmetic) the exact rule's block with every tie kept
            assert flags[i] & 2 and not flags[i] & 1, (name, order, i, int(flags[i]))
            assert np.array_equal(blk.astype(bool), want[i]), (name, order, i, np.argwhere(blk.astype(bool) != want[i])[:5].tolist())
        else:
            assert cl == "nan" and flags[i] & 1, (name, order, i, int(flags[i]))
    # device centroids give the same bytes
    cat, offs, _ = T.pack_centroids(images)
    adj_d, flags_d = eng.adjacency_flagged(torch.tensor(cat).to(eng.device), offs, order, device_flags=True)
    assert adj_d.cpu().numpy().tobytes() == adj.tobytes() and flags_d.cpu().numpy().tobytes() == flags.tobytes()
    # the counter of segvlad_adjacency agrees with the flags, and the engine raises what the reference / the pipeline expect
    n_bad, adj_c = _raw_counts(eng, cat, offs, order)
    n_nan = int(sum(int(np.isnan(i[:, 0]).sum()) for i in images))
    assert adj_c.tobytes() == adj.tobytes()
    assert (n_bad & 0xFFFF, n_bad >> 16) == (n_nan, int((flags & 2).astype(bool).sum())), (name, order, hex(n_bad), flags.tolist())
    assert int((flags & 1).astype(bool).sum()) == sum(cl == "nan" for cl in classes)
    if n_nan:
        with pytest.raises(ValueError):
            eng.adjacency(cat, offs, order, check_empty=True)
    elif "degenerate" in classes:
        with pytest.raises(SegVLADDegenerateError):
            eng.adjacency(cat, offs, order, check_empty=True)
    else:
        assert eng.adjacency(cat, offs, order, check_empty=True).cpu().numpy().tobytes() == adj.tobytes()
    # the neighbours of a flagged image get the block they get alone
    for i, cl in enumerate(classes):
        if cl in ("degenerate", "nan"):
            for j in (i - 1, i + 1):
                assert classes[j] == "generic"
                alone, f = _run_batch(eng, [images[j]], order)
                assert alone.tobytes() == got[j].tobytes() and f.tolist() == [0], (name, order, i, j)


def test_the_mask_centroid_batch_is_what_the_device_computes(eng):
    """The 'mask_centroids' batch holds the oracle's centroids of the s300 case's blobs: segvlad_mask_centroids returns those bytes"""
    cent = eng.mask_centroids(np.array(T.build_masks("s300")[0][:80])).cpu().numpy()
    imgs = T.adjacency_batches()["mask_centroids"]["images"]
    assert cent[:30].tobytes() == imgs[0].tobytes() and cent[30:].tobytes() == imgs[1].tobytes()


@pytest.mark.parametrize("order", T.ORDERS)
def test_the_two_block_sizes_write_the_same_blocks(eng, order):
    """65 images run with 256 threads per image, the first 64 of them alone with 1024: the same bytes and flags"""
    i65, i64 = T.adjacency_batches()["b65"]["images"], T.adjacency_batches()["b64"]["images"]
    a65, f65 = _run_batch(eng, i65, order)
    a64, f64 = _run_batch(eng, i64, order)
    assert a65[:len(a64)].tobytes() == a64.tobytes() and f65[:64].tobytes() == f64.tobytes() and len(a65) == len(a64) + len(i65[64]) ** 2


def test_small_images_ignore_the_order(eng):
    images = [i for i in T.adjacency_batches()["ladder"]["images"] if len(i) <= 3]
    assert sorted(len(i) for i in images) == [0, 0, 1, 2, 3, 3]
    for order in T.ORDERS:
        adj, flags = _run_batch(eng, images, order)
        for img, blk in zip(images, _blocks(adj, images)):
            assert np.array_equal(blk.astype(bool), _O().adjacency_from_centroids(img, order)), (order, len(img))
        assert not flags.any()


def _refused_with_limit(call):
    from revisit_anything_amd._lib import SEGVLAD_ERR_LIMIT, SegVLADError

    with pytest.raises(SegVLADError) as e:
        call()
    assert e.value.code == SEGVLAD_ERR_LIMIT, e.value


def test_one_segment_past_the_bound_is_refused_and_the_context_goes_on(eng):
    rng = np.random.Generator(np.random.PCG64(4600))
    big = T._int_points(rng, T.S_LIMIT + 1)
    offs = np.array([0, len(big)], np.int32)
    small = T.adjacency_batches()["nan"]["images"][0]
    want = T.adjacency_reference("nan", 2)[0]
    for call in (lambda: eng.adjacency(big, offs, 2), lambda: eng.adjacency_flagged(big, offs, 2),
                 # ... and under a batch of small images
                 lambda: eng.adjacency(np.concatenate([small, big, small]), np.array([0, 5, 5 + len(big), 10 + len(big)], np.int32), 1)):
        _refused_with_limit(call)
        adj, flags = _run_batch(eng, [small], 2)
        assert np.array_equal(adj.reshape(5, 5).astype(bool), want) and flags.tolist() == [0]


def test_the_one_call_describe_has_the_same_bound(eng):
    """segvlad_describe / segvlad_describe_begin refuse an image that sv_launch_adjacency refuses (SEGVLAD_ERR_LIMIT) and take the
    largest one it takes: one-pixel masks on a 28 x 42 raster, pixel s of mask s."""
    from revisit_anything_amd import synth

    K, D, H, W, Hm, Wm = 2, 32, 56, 84, 28, 42
    N = (H // 14) * (W // 14)
    eng.set_vocab(synth.make_vocab(K, D, seed=3))
    tok = torch.tensor(synth.make_tokens(synth.make_vocab(K, D, seed=3), N, seed=4, noise=0.1)[None]).to(eng.device)

    def masks(S):
        m = np.zeros((S, Hm * Wm), np.uint8)
        m[np.arange(S), np.arange(S)] = 1
        return torch.tensor(m.reshape(S, Hm, Wm)).to(eng.device)

    over, offs_over = masks(T.S_LIMIT + 1), np.array([0, T.S_LIMIT + 1], np.int32)
    _refused_with_limit(lambda: eng.describe(over, tok, offs_over, H, W, order=1, pca=False))
    _refused_with_limit(lambda: eng.describe_begin(over, tok, offs_over, H, W, order=1, pca=False))
    fits, offs = masks(T.S_LIMIT), np.array([0, T.S_LIMIT], np.int32)
    r = eng.describe(fits, tok, offs, H, W, order=1, pca=False)
    s = np.arange(T.S_LIMIT)
    assert r["cent"].cpu().numpy().tobytes() == np.stack([s % Wm, s // Wm], 1).astype(np.float64).tobytes()
    adj, flags = eng.adjacency_flagged(r["cent"], offs, 1)
    assert r["adj"].cpu().numpy().tobytes() == adj.cpu().numpy().tobytes() and r["flags"].cpu().numpy().tolist() == flags.tolist()
    h = eng.describe_begin(fits, tok, offs, H, W, order=1, pca=False)
    assert eng.describe_end(h)["out"].cpu().numpy().tobytes() == r["out"].cpu().numpy().tobytes()
