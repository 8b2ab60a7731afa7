"""Stream order of the UNGUARDED library: the table of cases and the harness of tests/test_gpu_async_order.py.

The `-m gpu` run is guarded (conftest.py): every call of a guarded context synchronises the device, so the suite's exact
arithmetic checks never meet the library its users run -- plain contexts, whose correctness rests on stream order alone.  Here
every device-work entry of include/segvlad.h runs on a plain context under conditions where a missing dependency gives a
WRONG VALUE, not a lucky right one:

  decoy and truth    every input exists twice, same shape and dtype, different content; any mixture of decoy and true buffers
                     is itself a valid input (same seg_offsets, same run_offsets, ids in range under both), so a mis-ordered
                     read is a wrong result and never an out-of-range access (`Case.valid`, checked on the CPU over all mixtures)
  warm-up            one call on ready DECOY inputs: sizes the scratch, loads the code objects and leaves decoy results in the
                     blocks torch's allocator hands out next
  delayed truth      the device inputs hold the decoy; on a non-blocking stream S: a delay, the copies of the truth, then the
                     call under torch.cuda.stream(S).  A launch or copy on another stream without a dependency on S, or a host
                     read of a value its stream has not produced yet, sees the decoy
  overwrite on return  the decoy goes back over every device input (on S), every host input array is overwritten in place, and
                     decoy-filled tensors of every input's size are allocated on S (the allocator is free to hand out any
                     conversion copy the engine no longer holds); the next call follows without a synchronisation
  three legs         guarded serial == plain serial == plain delayed, bit for bit

Nothing here needs a GPU to import: the builders and references are NumPy; torch and the engine are imported by the functions
that run on the device.  tests/test_async_order_cases.py checks the table on the CPU."""
from __future__ import annotations

import functools
import itertools
import math
import os
import re
import sys
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WHICH = ("truth", "decoy")
MIN_DELAY_MS = 20.0


def O():
    from oracle import segvlad_oracle

    return segvlad_oracle


def _seed(which):
    return {"truth": 1, "decoy": 2}[which]


def _unit32(x):
    x = np.asarray(x, dtype=np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- shapes: the smallest that still reach each path ---------------------------------------------------------------------------
S, HM, WM, H, W, PATCH = 12, 32, 48, 56, 84, 14      # the smallest mask size of tests/mask_branch_cases.py (s300)
N_TOK = (H // PATCH) * (W // PATCH)                  # 24 tokens
SEG_OFF = np.array([0, 8, 9, 12], dtype=np.int32)    # B = 3 images, the second with a single segment
B = len(SEG_OFF) - 1
K, D, P = 8, 64, 16
ORDER = 1                # (the second power of a Delaunay graph of 8 points is complete: no input would show in it)
MIN_AREA = 4
WIDTHS = 2 + np.arange(S) % 5   # columns of mask s's rectangle, the same under truth and decoy: 2 w + 1 runs either way


@functools.lru_cache(None)
def vocab():
    from revisit_anything_amd import synth

    return synth.make_vocab(K, D, seed=1)


@functools.lru_cache(None)
def pca_model(p=P):
    from revisit_anything_amd import synth

    return synth.make_pca_model(K * D, p, seed=7)


@functools.lru_cache(None)
def rect_masks(which, seed=0, specks=False, n=S):
    """n rectangles that touch neither the first nor the last pixel, mask s of WIDTHS[s % S] columns: the column-major run-length
    form holds 2 w + 1 runs whatever the position.  specks: a one-pixel hole and a one-pixel island per mask (mask_regions)."""
    r = np.random.default_rng([_seed(which), seed, 77])
    m = np.zeros((n, HM, WM), np.uint8)
    for s in range(n):
        w = int(WIDTHS[s % S])
        x0 = int(r.integers(0, WM - w + 1))
        y0, y1 = int(r.integers(1, HM // 2 - 2)), int(r.integers(HM // 2 + 2, HM - 1))
        m[s, y0:y1 + 1, x0:x0 + w] = 1
        if specks:
            m[s, int(r.integers(y0 + 1, y1)), x0 + (1 if w > 2 else 0)] = 0
            m[s, int(r.integers(0, HM)), (x0 + w + 3 + int(r.integers(0, 8))) % WM] = 1
    m.setflags(write=False)
    return m


def rle_of(which):
    from revisit_anything_amd.rle import RleMasks

    r = RleMasks.from_dense(rect_masks(which))
    return np.asarray(r.counts).astype(np.int32), np.asarray(r.run_offsets, dtype=np.int64)   # (counts < 2^31: int32 storage, viewed as uint32)


def centroids_of(which, n=S):
    """Distinct integer coordinates (exact in fp32 and fp64), generic with overwhelming odds: the Delaunay triangulation is unique."""
    r = np.random.default_rng([_seed(which), 5])
    return np.stack([r.permutation(2048)[:n], r.permutation(2048)[:n]], axis=1).astype(np.float64)


def adjacency_ref(cent, so=SEG_OFF, order=ORDER):
    return np.concatenate([O().adjacency_from_centroids(cent[so[b]:so[b + 1]], order).astype(np.uint8).reshape(-1)
                           for b in range(len(so) - 1)])


def random_adjacency(which, so=SEG_OFF):
    """Any 0 / 1 blocks are valid adjacency INPUT of the aggregation: random ones with a unit diagonal."""
    r = np.random.default_rng([_seed(which), 6])
    out = []
    for b in range(len(so) - 1):
        n = int(so[b + 1] - so[b])
        blk = (r.random((n, n)) < 0.3).astype(np.uint8)
        blk[np.arange(n), np.arange(n)] = 1
        out.append(blk.reshape(-1))
    return np.concatenate(out)


def tokens_of(which, seed=0, n_img=B):
    from revisit_anything_amd import synth

    return np.stack([synth.make_tokens(vocab(), N_TOK, seed=100 * _seed(which) + 10 * seed + b, noise=0.2) for b in range(n_img)])


def bits_of(masks):
    return O().pack_bits_u64(O().incidence(masks, H, W, PATCH)).view(np.int64)


def centroid_ref(masks):
    out = np.empty((len(masks), 2), np.float64)
    for s, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        out[s] = (np.float64(xs.sum()) / len(xs), np.float64(ys.sum()) / len(ys))
    return out


# ---- the index and the queries ---------------------------------------------------------------------------------------------------
ROWS_PER_IMAGE = 20
DUP0, N_DUP = 20_000, 600


@functools.lru_cache(None)
def index_rows(n, d, dup=False):
    r = np.random.default_rng([n, d, 31])
    R = _unit32(r.standard_normal((n, d)))
    if dup:
        R[DUP0:DUP0 + N_DUP] = R[DUP0]     # (tests/test_gpu_refine_group.py's duplicate block, shrunk)
    R.setflags(write=False)
    return R, (np.arange(n) // ROWS_PER_IMAGE).astype(np.int32)


@functools.lru_cache(None)
def queries(n, d, nq, which, dup=False):
    R, _ = index_rows(n, d, dup)
    r = np.random.default_rng([n, d, nq, _seed(which), 32])
    if dup and which == "truth":
        rows, sigma = np.arange(DUP0 - 10, DUP0 - 10 + nq), 0.05 / math.sqrt(d)
    else:
        rows, sigma = r.choice(n, nq, replace=False), 0.05
    Q = _unit32(R[rows] + sigma * r.standard_normal((nq, d)).astype(np.float32))
    Q.setflags(write=False)
    return Q


@functools.lru_cache(None)
def knn_ref(n, d, nq, which, k, dup=False):
    return O().knn_l2(index_rows(n, d, dup)[0], queries(n, d, nq, which, dup), k)


@functools.lru_cache(None)
def d2_matrix(n, d, nq, which):
    """fp64 squared distances of the query rows to every index row (the derived searches' references)."""
    R, Q = index_rows(n, d)[0].astype(np.float64), queries(n, d, nq, which).astype(np.float64)
    return np.maximum((Q * Q).sum(1)[:, None] + (R * R).sum(1)[None, :] - 2.0 * Q @ R.T, 0.0)


def topk_masked(d2, allowed, k):
    """Per row the k smallest distances among the allowed columns, ties to the lower id; (+inf, -1) beyond them."""
    d = np.where(allowed, d2, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    dd = np.take_along_axis(d, idx, axis=1)
    return dd.astype(np.float32), np.where(np.isfinite(dd), idx, -1).astype(np.int64)


# ---- a case ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str                  # "mask" | "describe" | "search"
    entries: tuple              # the entries of include/segvlad.h (without the prefix) the case's steps call
    build: Callable             # which -> {name: ndarray}: every input, truth or decoy
    steps: list                 # [(fn(eng, a, st) -> {name: output} | None, names the caller may overwrite after it | None = all)]
    ref: Callable               # inputs -> {name: ndarray}: a plain NumPy / fp64 reference of the result (or of part of it)
    valid: Callable             # inputs (any mixture) -> None; asserts what the entry demands of its arguments
    host: tuple = ()            # inputs handed over as host arrays (the rest are device tensors)
    fixed: tuple = ()           # inputs whose truth and decoy MUST agree (offsets)
    fixture: str = ""           # FIXTURES key: what the context holds before the call (vocabulary, PCA model, index)
    convert: dict = field(default_factory=dict)   # name -> "bool" | "strided" | "f32": the storage that forces the engine's conversion copy
    options: tuple = ()         # ((key, value for the call, value afterwards), ...)
    check: Optional[Callable] = None    # (inputs, outputs, ref) -> None: the GUARDED result against the reference
    plan: Optional[Callable] = None     # search_stats() of the serial plain leg -> None; asserts the search plan
    plan_needs_stats: bool = False      # the plan reads a figure only option search_stats=1 records (grp_groups): the option is then
                                        # on for the PLAIN SERIAL leg of this case alone -- it makes a search wait for its stream, so
                                        # the delayed and pipelined legs never run with it (nor do users, nor does bench.py)
    dirties_fixture: bool = False


def mixtures(case):
    """Every assignment of truth / decoy to the case's input buffers."""
    t, d = case.build("truth"), case.build("decoy")
    names = sorted(t)
    for pick in itertools.product((0, 1), repeat=len(names)):
        yield {n: (t, d)[p][n] for n, p in zip(names, pick)}


def same_shapes(case):
    t, d = case.build("truth"), case.build("decoy")
    assert sorted(t) == sorted(d)
    for n in t:
        assert t[n].shape == d[n].shape and t[n].dtype == d[n].dtype, (case.name, n)
        if n in case.fixed:
            assert np.array_equal(t[n], d[n]), (case.name, n, "must agree under truth and decoy")
        else:
            assert not np.array_equal(t[n], d[n]), (case.name, n, "the decoy is the truth")


# ---- validity rules --------------------------------------------------------------------------------------------------------------
def _v_offsets(off, total, name="offsets"):
    off = np.asarray(off, dtype=np.int64)
    assert off.ndim == 1 and off[0] == 0 and off[-1] == total and (np.diff(off) >= 0).all(), name


def _v_masks(a, key="masks", n=S):
    assert a[key].shape == (n, HM, WM) and a[key].dtype == np.uint8


def _v_rle(a):
    c, o = a["counts"].astype(np.int64), a["run_offsets"]
    _v_offsets(o, len(c), "run_offsets")
    assert len(o) == S + 1 and (c >= 0).all()
    cs = np.concatenate([[0], np.cumsum(c)])
    assert np.array_equal(cs[o[1:]] - cs[o[:-1]], np.full(S, HM * WM)), "counts must sum to Hm * Wm per mask"


def _v_adj_in(a):
    assert a["cent"].shape == (S, 2) and np.isfinite(a["cent"]).all()
    _v_offsets(a["seg_offsets"], S)
    for b in range(B):
        c = a["cent"][SEG_OFF[b]:SEG_OFF[b + 1]]
        assert len(np.unique(c, axis=0)) == len(c), "duplicate centroids"


def _v_images(a):
    _v_offsets(a["seg_offsets"], S)
    assert a["tokens"].shape == (B, D, N_TOK) and np.isfinite(a["tokens"]).all()
    assert a["bits"].shape == (S, (N_TOK + 63) // 64)
    assert (a["bits"].view(np.uint64) >> np.uint64(N_TOK) == 0).all(), "incidence bits beyond N"
    sizes = np.diff(SEG_OFF).astype(np.int64)
    assert a["adj"].shape == (int((sizes * sizes).sum()),) and a["adj"].max() <= 1


def _v_describe(a):
    _v_offsets(a["seg_offsets"], S)
    _v_masks(a)
    assert all(a["masks"][s].any() for s in range(S)), "an empty mask has no centroid"
    assert a["tokens"].shape == (B, D, N_TOK) and np.isfinite(a["tokens"]).all()
    if "patch_blocks" in a:
        assert list(a["patch_images"]) == sorted(set(a["patch_images"])) and 0 <= a["patch_images"].min() and a["patch_images"].max() < B
        assert len(a["patch_blocks"]) == sum(int(SEG_OFF[b + 1] - SEG_OFF[b]) ** 2 for b in a["patch_images"]) and a["patch_blocks"].max() <= 1


def _v_rows(a, key, d):
    assert a[key].ndim == 2 and a[key].shape[1] == d and np.isfinite(a[key]).all()


# ---- steps: thin wrappers that name the outputs ------------------------------------------------------------------------------------
def _rle(a):
    import torch
    from revisit_anything_amd.rle import RleMasks

    return RleMasks(a["counts"].view(torch.uint32), a["run_offsets"], HM, WM, validate=False)


def _s_incidence(eng, a, st):
    return {"bits": eng.incidence(a["masks"], H, W, PATCH)}


def _s_incidence_centroids(eng, a, st):
    bits, cent = eng.incidence_centroids(a["masks"], H, W, PATCH)
    return {"bits": bits, "cent": cent}


def _s_mask_centroids(eng, a, st):
    return {"cent": eng.mask_centroids(a["masks"])}


def _s_incidence_rle(eng, a, st):
    bits, cent, n_bad = eng.incidence_rle(_rle(a), H, W, PATCH, want_bad=True)
    return {"bits": bits, "cent": cent, "n_bad": n_bad}


def _s_rle_decode(eng, a, st):
    m, n_bad = eng.rle_decode(_rle(a), want_bad=True)
    return {"masks": m, "n_bad": n_bad}


def _s_rle_encode(eng, a, st):
    rle, areas = eng.rle_encode(a["masks"], want_area=True)
    return {"counts": rle.counts, "run_offsets": rle.run_offsets, "areas": areas}


RLE_POISON = 0xA5A5A5A5


def _s_rle_encode_host(capacity_of_total, tag=""):
    """segvlad_rle_encode with HOST counts_out (the engine only offers device counts): `capacity_of_total(total)` slots.  An
    over-capacity call must leave the host counts alone."""
    def step(eng, a, st):
        import ctypes as C

        import torch

        m = a["masks"] if a["masks"].dtype == torch.uint8 else a["masks"].view(torch.uint8)
        m = m.contiguous()
        n_runs = int((2 * WIDTHS + 1).sum())
        cap = capacity_of_total(n_runs)
        counts = np.full(n_runs, RLE_POISON, np.uint32)
        offs = np.zeros(S + 1, np.int64)
        total = C.c_int64(-1)
        eng._stream()
        eng._check(eng.lib.segvlad_rle_encode(eng._h, m.data_ptr(), S, HM, WM, offs.ctypes.data, counts.ctypes.data, cap, None,
                                              C.byref(total)), "rle_encode")
        eng._keep = [m]
        return {tag + "counts": counts.copy(), tag + "run_offsets": offs.copy(), tag + "total": int(total.value)}
    return step


def _s_mask_regions(eng, a, st):
    return eng.mask_regions(a["masks"], MIN_AREA)


def _s_adjacency(check_empty):
    def step(eng, a, st):
        return {"adj": eng.adjacency(a["cent"], a["seg_offsets"], ORDER, check_empty=check_empty)}
    return step


def _s_adjacency_flagged(device_flags):
    def step(eng, a, st):
        adj, flags = eng.adjacency_flagged(a["cent"], a["seg_offsets"], ORDER, device_flags=device_flags)
        return {"adj": adj, "flags": flags if device_flags else np.array(flags)}
    return step


def _s_images(eng, a, st):
    return eng.seg_vlad(a["tokens"], a["bits"], a["seg_offsets"], a["adj"], want_labels=True, want_gap=True, want_block_norms=True)


def _s_images_pca(want_desc):
    def step(eng, a, st):
        return eng.seg_vlad_pca(a["tokens"], a["bits"], a["seg_offsets"], a["adj"], l2norm=True, want_desc=want_desc, want_labels=True)
    return step


def _s_describe(pca):
    def step(eng, a, st):
        return eng.describe(a["masks"], a["tokens"], a["seg_offsets"], H, W, PATCH, ORDER, pca=pca, l2norm=True, want_desc=pca)
    return step


def _s_begin(eng, a, st):
    st["h"] = eng.describe_begin(a["masks"], a["tokens"], a["seg_offsets"], H, W, PATCH, ORDER, pca=True)


def _s_flags(eng, a, st):
    flags, cent = eng.describe_flags(st["h"])
    return {"flags_host": flags.copy(), "cent_host": cent.copy()}       # read on return


def _s_end(patched):
    def step(eng, a, st):
        if not patched:
            return eng.describe_end(st["h"], l2norm=True, want_desc=True)
        blocks, pos = [], 0
        for b in a["patch_images"]:
            n = int(SEG_OFF[b + 1] - SEG_OFF[b]) ** 2
            blocks.append(a["patch_blocks"][pos:pos + n])
            pos += n
        return eng.describe_end(st["h"], a["patch_images"], blocks, l2norm=True, want_desc=True)
    return step


def _s_cancel(eng, a, st):
    eng.describe_cancel(st["h"])


def _s_kmeans(tok):
    def step(eng, a, st):
        import torch

        if "sums" not in st:
            st["sums"] = torch.zeros(K, D, dtype=torch.float64, device=eng.device)
            st["counts"] = torch.zeros(K, dtype=torch.int64, device=eng.device)
        lab = eng.kmeans_step(a[tok], st["sums"], st["counts"], want_labels=True)
        return {"labels_" + tok: lab, "sums": st["sums"], "counts": st["counts"]}
    return step


def _s_cluster_aggregate(eng, a, st):
    return {"out": eng.cluster_aggregate(K, a["res"], a["labels"], a["bits"], a["adj"])}


def _s_pca_apply(eng, a, st):
    return {"y": eng.pca_apply(a["X"], l2norm=True)}


def _s_normalize_rows(eng, a, st):
    return {"y": eng.normalize_rows(a["X"])}


# ---- builders and references: mask branch ---------------------------------------------------------------------------------------
def _b_masks(which):
    return {"masks": rect_masks(which)}


def _b_masks_specks(which):
    return {"masks": rect_masks(which, specks=True)}


def _b_rle(which):
    c, o = rle_of(which)
    return {"counts": c, "run_offsets": o}


def _b_cent(which):
    return {"cent": centroids_of(which), "seg_offsets": SEG_OFF.copy()}


def _r_incidence(a):
    return {"bits": bits_of(a["masks"])}


def _r_incidence_centroids(a):
    return {"bits": bits_of(a["masks"]), "cent": centroid_ref(a["masks"])}


def _r_mask_centroids(a):
    return {"cent": centroid_ref(a["masks"])}


def _dense_of(a):
    from revisit_anything_amd.rle import RleMasks

    return np.asarray(RleMasks(a["counts"].view(np.uint32), a["run_offsets"], HM, WM).to_dense()).astype(np.uint8)


def _r_incidence_rle(a):
    m = _dense_of(a)
    return {"bits": bits_of(m), "cent": centroid_ref(m), "n_bad": np.zeros(1, np.int32)}


def _r_rle_decode(a):
    return {"masks": _dense_of(a), "n_bad": np.zeros(1, np.int32)}


def _r_rle_encode(a):
    import rle_encode_ref
    from revisit_anything_amd.rle import RLE_ENCODE_ROWS

    counts, run_offsets, areas = rle_encode_ref.encode_model(a["masks"], RLE_ENCODE_ROWS)
    return {"counts": counts.view(np.int32), "run_offsets": run_offsets, "areas": areas}


def _r_rle_encode_host(a):
    r = _r_rle_encode(a)
    n = np.int64(len(r["counts"]))
    return {"counts": r["counts"], "run_offsets": r["run_offsets"], "total": n, "over_run_offsets": r["run_offsets"], "over_total": n,
            "over_counts": np.full(n, RLE_POISON, np.uint32).view(np.int32)}     # an over-capacity call leaves the host counts alone


def _r_mask_regions(a):
    import regions_ref

    m, changed, boxes, area = regions_ref.clean_batch(a["masks"], MIN_AREA)
    return {"masks": m, "changed": changed, "boxes": boxes, "area": area}


def _r_adjacency(a):
    return {"adj": adjacency_ref(a["cent"]), "flags": np.zeros(B, np.uint8)}


def exact(names):
    """The guarded result equals the reference, value for value, on the named outputs."""
    def check(a, out, ref):
        for n in names:
            got = out[n].view(ref[n].dtype) if out[n].dtype.itemsize == ref[n].dtype.itemsize else out[n]
            assert np.array_equal(got.reshape(ref[n].shape), ref[n]), n
    return check


# ---- builders and references: describe ------------------------------------------------------------------------------------------
def _b_images(which):
    return {"tokens": tokens_of(which), "bits": bits_of(rect_masks(which, seed=3)), "adj": random_adjacency(which),
            "seg_offsets": SEG_OFF.copy()}


def _r_desc(a):
    """fp64 descriptors of the batch given incidence bits and adjacency blocks."""
    inc = O().unpack_bits_u64(a["bits"].view(np.uint64), N_TOK)
    out, pos = [], 0
    for b in range(B):
        s0, s1 = int(SEG_OFF[b]), int(SEG_OFF[b + 1])
        n = s1 - s0
        out.append(O().seg_vlad(a["tokens"][b], inc[s0:s1], vocab(), a["adj"][pos:pos + n * n].reshape(n, n).astype(bool)))
        pos += n * n
    return np.concatenate(out)


def _project(desc, p=P):
    mean, comps, var = pca_model(p)
    y = O().pca_transform(desc, mean, comps, var, whiten=True)
    return y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)


def _r_images(a):
    return {"out": _r_desc(a)}


def _r_images_pca(a):
    desc = _r_desc(a)
    return {"desc": desc, "out": _project(desc)}


def _from_masks(a, adj=None):
    m = a["masks"]
    cent = centroid_ref(m)
    b = {"tokens": a["tokens"], "bits": bits_of(m), "adj": adjacency_ref(cent) if adj is None else adj}
    return b, cent


def _r_describe(pca):
    def ref(a):
        b, cent = _from_masks(a)
        desc = _r_desc(b)
        r = {"bits": b["bits"], "cent": cent, "adj": b["adj"], "flags": np.zeros(B, np.uint8), "cent_host": cent, "flags_host": np.zeros(B, np.uint8)}
        r.update({"desc": desc, "out": _project(desc)} if pca else {"out": desc})
        return r
    return ref


def _r_describe_patched(a):
    b, cent = _from_masks(a)
    sizes = np.diff(SEG_OFF).astype(np.int64) ** 2
    aoff = np.concatenate([[0], np.cumsum(sizes)])
    adj, pos = b["adj"].copy(), 0
    for i in a["patch_images"]:
        adj[aoff[i]:aoff[i + 1]] = a["patch_blocks"][pos:pos + sizes[i]]
        pos += sizes[i]
    b["adj"] = adj
    desc = _r_desc(b)
    return {"bits": b["bits"], "cent": cent, "adj": adj, "cent_host": cent, "flags_host": np.zeros(B, np.uint8), "desc": desc, "out": _project(desc)}


def bits_equal(names):
    """The guarded result equals the reference bit for bit on the named floating-point outputs."""
    def check(a, out, ref):
        for n in names:
            got, want = np.ascontiguousarray(out[n]), np.ascontiguousarray(ref[n], dtype=out[n].dtype)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), n
    return check


def all_of(*checks):
    def check(a, out, ref):
        for c in checks:
            c(a, out, ref)
    return check


def check_kmeans(a, out, ref):
    exact(("labels_t1", "labels_t2", "counts"))(a, out, ref)
    # tests/test_gpu_frows.py: the sums to 1e-6 per accumulated token
    assert np.abs(out["sums"] - ref["sums"]).max() < 1e-6 * max(1.0, float(ref["counts"].max()))


def check_pca_rows(a, out, ref):
    assert np.abs(out["y"] - ref["y"]).max() < PCA_REL_TOL * np.abs(ref["y"]).max()


def check_normalize_rows(a, out, ref):
    # tests/test_gpu_projection.py: per entry within 2 ulp of the float64 quotient
    ulp = np.spacing(np.abs(ref["y"]).astype(np.float32)).astype(np.float64)
    assert (np.abs(out["y"] - ref["y"]) / ulp).max() <= 2.0


def check_verify(a, out, ref):
    # tests/test_gpu_verify.py: the integer outputs exactly, the model within 1e-9 absolute
    exact(("n_inlier", "pair", "order", "inlier"))(a, out, ref)
    assert np.array_equal(np.isnan(out["model"]), np.isnan(ref["model"]))
    ok = ~np.isnan(ref["model"])
    assert np.abs(out["model"][ok] - ref["model"][ok]).max(initial=0.0) <= 1e-9


DESC_TOL = 2e-6          # tests/test_gpu_frows.py: the descriptors against the oracle's
PCA_REL_TOL = 5e-5       # tests/test_gpu_frows.py: the device's apply of a model against its fp64 evaluation, of max |y|


def check_describe(ints=(), desc="out", y=None):
    def check(a, out, ref):
        exact(ints)(a, out, ref)
        if desc:
            assert np.abs(out[desc] - ref[desc]).max() < DESC_TOL, np.abs(out[desc] - ref[desc]).max()
        if y:
            assert np.abs(out[y] - ref[y]).max() < PCA_REL_TOL * np.abs(ref[y]).max(), np.abs(out[y] - ref[y]).max()
    return check


def _b_describe(which):
    return {"masks": rect_masks(which, seed=3), "tokens": tokens_of(which), "seg_offsets": SEG_OFF.copy()}


def _b_describe_patched(which):
    d = _b_describe(which)
    r = np.random.default_rng([_seed(which), 9])
    imgs = np.array([0, 2], np.int32)
    blocks = []
    for b in imgs:
        n = int(SEG_OFF[b + 1] - SEG_OFF[b])
        blk = (r.random((n, n)) < 0.4).astype(np.uint8)
        blk[np.arange(n), np.arange(n)] = 1
        blocks.append(blk.reshape(-1))
    d.update(patch_images=imgs, patch_blocks=np.concatenate(blocks))
    return d


def _b_kmeans(which):
    return {"t1": tokens_of(which, seed=1), "t2": tokens_of(which, seed=2)}


def _r_kmeans(a):
    X = np.concatenate([O().normalize_tokens_f32(t) for tk in ("t1", "t2") for t in a[tk]])
    labels, _, sums, counts = O().kmeans_cosine_step(X, vocab())
    return {"sums": sums, "counts": counts.astype(np.int64), "labels_t1": labels[:B * N_TOK].astype(np.uint8).reshape(B, N_TOK),
            "labels_t2": labels[B * N_TOK:].astype(np.uint8).reshape(B, N_TOK)}


def _v_kmeans(a):
    for k in ("t1", "t2"):
        assert a[k].shape == (B, D, N_TOK) and np.isfinite(a[k]).all()


S_CA = 5


def _b_cluster_aggregate(which):
    r = np.random.default_rng([_seed(which), 13])
    xn = O().normalize_tokens_f32(tokens_of(which)[0])
    labels, _ = O().assign_labels(xn, vocab())
    return {"res": (xn - vocab()[labels]).astype(np.float32), "labels": labels.astype(np.uint8),
            "bits": bits_of(rect_masks(which, seed=4)[:S_CA]), "adj": random_adjacency(which, np.array([0, S_CA]))}


def _r_cluster_aggregate(a):
    inc = O().unpack_bits_u64(a["bits"].view(np.uint64), N_TOK)
    return {"out": O().vlad_matmuls_per_cluster(K, inc, a["res"], a["labels"].astype(np.int64), a["adj"].reshape(S_CA, S_CA))}


def _v_cluster_aggregate(a):
    assert a["res"].shape == (N_TOK, D) and a["labels"].shape == (N_TOK,) and a["labels"].max() < K
    assert a["bits"].shape == (S_CA, 1) and a["adj"].shape == (S_CA * S_CA,) and a["adj"].max() <= 1


def _b_pca_rows(which):
    r = np.random.default_rng([_seed(which), 17])
    return {"X": _unit32(r.standard_normal((S, K * D)))}


def _r_pca_apply(a):
    return {"y": _project(a["X"].astype(np.float64))}


def _b_rows(which):
    r = np.random.default_rng([_seed(which), 19])
    return {"X": (r.standard_normal((S, D)) * 3).astype(np.float32)}


def _r_normalize_rows(a):
    x = a["X"].astype(np.float64)
    return {"y": x / np.linalg.norm(x, axis=1, keepdims=True)}


# set_vocab / pca_set: the MODEL arrives late (device tensors) and is overwritten on return; a fixed batch then reads it back
def _decoy_vocab():
    from revisit_anything_amd import synth

    return synth.make_vocab(K, D, seed=2)


def _b_vocab(which):
    return {"C": vocab() if which == "truth" else _decoy_vocab()}


@functools.lru_cache(None)
def _probe_images():
    return _b_images("truth")


def _s_set_vocab(eng, a, st):
    eng.set_vocab(a["C"])


def _s_probe_images(eng, a, st):
    import torch

    b = _probe_images()
    dev = {k: torch.from_numpy(np.array(b[k])).to(eng.device) for k in ("tokens", "bits", "adj")}
    st["probe"] = dev                                    # (alive until the sequence's synchronisation)
    return {"out": eng.seg_vlad(dev["tokens"], dev["bits"], b["seg_offsets"], dev["adj"])["out"]}


def _r_set_vocab(a):
    b = dict(_probe_images())
    inc = O().unpack_bits_u64(b["bits"].view(np.uint64), N_TOK)
    out, pos = [], 0
    for i in range(B):
        s0, s1 = int(SEG_OFF[i]), int(SEG_OFF[i + 1])
        n = s1 - s0
        out.append(O().seg_vlad(b["tokens"][i], inc[s0:s1], a["C"], b["adj"][pos:pos + n * n].reshape(n, n).astype(bool)))
        pos += n * n
    return {"out": np.concatenate(out)}


def _v_vocab(a):
    assert a["C"].shape == (K, D) and np.isfinite(a["C"]).all() and (np.linalg.norm(a["C"], axis=1) > 0).all()


def _b_pca_model(which):
    from revisit_anything_amd import synth

    mean, comps, var = pca_model() if which == "truth" else synth.make_pca_model(K * D, P, seed=8)
    if which == "decoy":
        var = (var * np.float32(1.5)).astype(np.float32)
    return {"mean": mean, "comps": comps, "var": var}


@functools.lru_cache(None)
def _probe_rows():
    return _b_pca_rows("truth")["X"]


def _s_pca_set(eng, a, st):
    eng.pca_set(a["mean"], a["comps"], a["var"], whiten=True)


def _s_probe_pca(eng, a, st):
    import torch

    st["probe"] = torch.from_numpy(np.array(_probe_rows())).to(eng.device)     # (alive until the sequence's synchronisation)
    return {"y": eng.pca_apply(st["probe"], l2norm=True)}


def _r_pca_set(a):
    y = O().pca_transform(_probe_rows().astype(np.float64), a["mean"], a["comps"], a["var"], whiten=True)
    return {"y": y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)}


def _v_pca_model(a):
    assert a["comps"].shape == (P, K * D) and a["mean"].shape == (K * D,) and a["var"].shape == (P,)
    assert all(np.isfinite(a[k]).all() for k in a) and (a["var"] > 0).all()


# ---- builders, steps and references: index and search --------------------------------------------------------------------------
N_IMG_Q, ROWS_Q = 5, 10          # the derived searches: 5 query images of 10 rows (one single-image pass)
QOFF = (np.arange(N_IMG_Q + 1) * ROWS_Q).astype(np.int32)
NQ_SMALL = N_IMG_Q * ROWS_Q
N40, N20 = 40_000, 20_000        # just past / below plan_search's 32 768 rows
K_SEARCH = 10


def _b_queries(n, d, nq, dup=False):
    def build(which):
        return {"Q": queries(n, d, nq, which, dup)}
    return build


def _s_search(k=K_SEARCH):
    def step(eng, a, st):
        d2, idx = eng.search(a["Q"], k)
        return {"d2": d2, "idx": idx}
    return step


def _r_search(n, d, nq, k=K_SEARCH, dup=False):
    def ref(a):
        which = "truth" if np.array_equal(a["Q"], queries(n, d, nq, "truth", dup)) else "decoy"
        d2, idx = knn_ref(n, d, nq, which, k, dup)
        return {"d2": d2, "idx": idx}
    return ref


KNN_TOL = 1e-5       # tests/test_gpu_parity.py: squared L2 of unit rows; ids wherever neighbouring distances are further apart


def check_knn(a, out, ref):
    d2, idx, rd2, ridx = out["d2"], out["idx"], ref["d2"], ref["idx"]
    fin = np.isfinite(rd2)
    assert np.array_equal(np.isfinite(d2), fin) and np.abs(d2[fin] - rd2[fin]).max() < KNN_TOL, np.abs(d2[fin] - rd2[fin]).max()
    assert np.all(np.diff(d2, axis=1)[fin[:, 1:]] >= 0)
    with np.errstate(invalid="ignore"):
        sep = np.minimum(np.diff(rd2, axis=1, prepend=-1), np.diff(rd2, axis=1, append=9)) > KNN_TOL
    assert np.array_equal(idx[sep], ridx[sep])
    assert np.array_equal(idx[~fin], ridx[~fin])


def _plan(**want):
    def plan(st):
        print(f"[async order] search_stats: {st}")
        for key, v in want.items():
            got = st[key]
            assert (v(got) if callable(v) else got == v), (key, got, st)
    return plan


def _which_q(a, n, d, nq):
    return "truth" if np.array_equal(a["Q"], queries(n, d, nq, "truth")) else "decoy"


def _img_allowed(n, allowed_imgs):
    """[n_img_q][n] bool: the index rows whose image each query image may match."""
    img = index_rows(n, D)[1]
    return np.stack([np.isin(img, np.asarray(ids)[np.asarray(ids) >= 0]) for ids in allowed_imgs])


def _b_shortlist(which):
    r = np.random.default_rng([_seed(which), 23])
    sl = r.integers(0, N40 // ROWS_PER_IMAGE, (N_IMG_Q, 4)).astype(np.int32)
    sl[1, 3] = -1
    return {"Q": queries(N40, D, NQ_SMALL, which), "qseg_offsets": QOFF.copy(), "shortlist": sl}


def _s_shortlist(eng, a, st):
    d2, idx = eng.search_shortlist(a["Q"], a["qseg_offsets"], a["shortlist"], K_SEARCH)
    return {"d2": d2, "idx": idx}


def _r_shortlist(a):
    allowed = np.repeat(_img_allowed(N40, a["shortlist"]), ROWS_Q, axis=0)
    d2, idx = topk_masked(d2_matrix(N40, D, NQ_SMALL, _which_q(a, N40, D, NQ_SMALL)), allowed, K_SEARCH)
    return {"d2": d2, "idx": idx}


def _v_derived(a):
    _v_rows(a, "Q", D)
    _v_offsets(a["qseg_offsets"], len(a["Q"]), "qseg_offsets")
    n_img_ref = N40 // ROWS_PER_IMAGE
    if "shortlist" in a:
        assert a["shortlist"].shape[0] == N_IMG_Q and a["shortlist"].min() >= -1 and a["shortlist"].max() < n_img_ref
    if "cand" in a:
        assert a["cand"].shape[0] == N_IMG_Q and a["cand"].shape[1] <= 64 and a["cand"].min() >= -1 and a["cand"].max() < n_img_ref
    if "exclude" in a:
        assert a["exclude"].shape == (N_IMG_Q, 2, 2)
        width = (a["exclude"][:, :, 1].astype(np.int64) - a["exclude"][:, :, 0] + 1).clip(0).sum(1).max()
        assert K_SEARCH + width * ROWS_PER_IMAGE <= 1024, "the window must leave the inner search below depth 1024"


def _b_excluding(which):
    r = np.random.default_rng([_seed(which), 29])
    lo = r.integers(0, N40 // ROWS_PER_IMAGE - 8, (N_IMG_Q, 2)).astype(np.int32)
    ex = np.stack([lo, lo + r.integers(0, 4, (N_IMG_Q, 2)).astype(np.int32)], axis=2)
    ex[2, 1] = (0, -1)
    # (the nearest rows of every query image's first row are excluded: the window then changes the result)
    first = knn_ref(N40, D, NQ_SMALL, which, K_SEARCH)[1][::ROWS_Q, 0] // ROWS_PER_IMAGE
    ex[:, 0, 0], ex[:, 0, 1] = first, first + 1
    return {"Q": queries(N40, D, NQ_SMALL, which), "qseg_offsets": QOFF.copy(), "exclude": np.ascontiguousarray(ex, dtype=np.int32)}


def _s_excluding(eng, a, st):
    d2, idx = eng.search_excluding(a["Q"], a["qseg_offsets"], a["exclude"], K_SEARCH)
    return {"d2": d2, "idx": idx}


def _r_excluding(a):
    img = index_rows(N40, D)[1].astype(np.int64)
    allowed = np.ones((N_IMG_Q, N40), bool)
    for b in range(N_IMG_Q):
        for lo, hi in a["exclude"][b]:
            allowed[b] &= ~((img >= lo) & (img <= hi))
    d2, idx = topk_masked(d2_matrix(N40, D, NQ_SMALL, _which_q(a, N40, D, NQ_SMALL)), np.repeat(allowed, ROWS_Q, axis=0), K_SEARCH)
    return {"d2": d2, "idx": idx}


K_GROUPED = 5


def _s_grouped(eng, a, st):
    d2, idx = eng.search_grouped(a["Q"], K_GROUPED, 1)
    return {"d2": d2, "idx": idx}


def _r_grouped(a):
    from revisit_anything_amd.engine import collapse_lists

    d2, idx = knn_ref(N40, D, NQ_SMALL, _which_q(a, N40, D, NQ_SMALL), 200)
    d2, idx = collapse_lists(d2, idx, index_rows(N40, D)[1], K_GROUPED, 1)
    return {"d2": d2, "idx": idx}


def _b_range(which):
    d2 = knn_ref(N40, D, NQ_SMALL, which, K_SEARCH)[0]
    r = np.random.default_rng([_seed(which), 37])
    # between a row's 1st .. 6th neighbour's distance, away from both: the hits are decided beyond fp32 noise
    j = r.integers(0, 6, NQ_SMALL)
    rad = 0.5 * (d2[np.arange(NQ_SMALL), j] + d2[np.arange(NQ_SMALL), j + 1])
    return {"Q": queries(N40, D, NQ_SMALL, which), "radius2": rad.astype(np.float32)}


def _s_range(eng, a, st):
    lims, d2, idx = eng.range_search(a["Q"], a["radius2"])
    return {"lims": lims, "d2": d2, "idx": idx}     # (whether the first capacity sufficed follows the context's history, not the inputs)


def _r_range(a):
    dm = d2_matrix(N40, D, NQ_SMALL, _which_q(a, N40, D, NQ_SMALL))
    hit = dm < a["radius2"].astype(np.float64)[:, None]
    lims = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    d2s, ids = [], []
    for q in range(NQ_SMALL):
        j = np.nonzero(hit[q])[0]
        j = j[np.argsort(dm[q, j], kind="stable")]
        d2s.append(dm[q, j].astype(np.float32))
        ids.append(j.astype(np.int64))
    return {"lims": lims, "d2": np.concatenate(d2s), "idx": np.concatenate(ids)}


def check_range(a, out, ref):
    assert np.array_equal(out["lims"], ref["lims"]) and np.array_equal(out["idx"], ref["idx"])
    assert np.abs(out["d2"] - ref["d2"]).max() < KNN_TOL


def _b_match(which):
    nn = knn_ref(N40, D, NQ_SMALL, which, K_SEARCH)[1] // ROWS_PER_IMAGE
    r = np.random.default_rng([_seed(which), 41])
    cand = r.integers(0, N40 // ROWS_PER_IMAGE, (N_IMG_Q, 4)).astype(np.int32)
    cand[:, 0] = nn[::ROWS_Q, 0]          # the image of the first row's nearest neighbour: a slot with mutual pairs
    cand[3, 3] = -1
    return {"Q": queries(N40, D, NQ_SMALL, which), "qseg_offsets": QOFF.copy(), "cand": cand}


def _s_match(eng, a, st):
    return eng.match_pairs(a["Q"], a["qseg_offsets"], a["cand"], want_rows=True)


def _r_match(a):
    dm = d2_matrix(N40, D, NQ_SMALL, _which_q(a, N40, D, NQ_SMALL))
    img = index_rows(N40, D)[1]
    C_ = a["cand"].shape[1]
    fwd = np.full((NQ_SMALL, C_), -1, np.int64)
    mutual = np.zeros((NQ_SMALL, C_), np.uint8)
    for b in range(N_IMG_Q):
        q0, q1 = int(QOFF[b]), int(QOFF[b + 1])
        for j, c in enumerate(a["cand"][b]):
            rows = np.nonzero(img == c)[0]
            if c < 0 or not len(rows):
                continue
            blk = dm[q0:q1][:, rows]
            f, bw = blk.argmin(1), blk.argmin(0)
            fwd[q0:q1, j] = rows[f]
            mutual[q0:q1, j] = bw[f] == np.arange(q1 - q0)
    n_mutual = np.stack([mutual[QOFF[b]:QOFF[b + 1]].sum(0) for b in range(N_IMG_Q)]).astype(np.int32)
    return {"fwd_idx": fwd, "mutual": mutual, "n_mutual": n_mutual}


def _b_verify(which):
    r = np.random.default_rng([_seed(which), 43])
    n_r, C_ = 200, 4
    q_xy = r.uniform(0, 500, (NQ_SMALL, 2))
    r_xy = r.uniform(0, 500, (n_r, 2))
    fwd = r.integers(0, n_r, (NQ_SMALL, C_)).astype(np.int64)
    r_xy[fwd[:, 0]] = q_xy * 1.1 + 7.0     # slot 0: one similarity explains (most of) its pairs
    fwd[r.random((NQ_SMALL, C_)) < 0.1] = -1
    mutual = ((r.random((NQ_SMALL, C_)) < 0.7) & (fwd >= 0)).astype(np.uint8)
    return {"q_xy": q_xy, "r_xy": r_xy, "fwd_idx": fwd, "mutual": mutual, "qseg_offsets": QOFF.copy()}


def _s_verify(eng, a, st):
    return eng.verify_pairs(a["q_xy"], a["r_xy"], a["qseg_offsets"], a["fwd_idx"], a["mutual"], tol=3.0, want_rows=True)


def _r_verify(a):
    import verify_ref

    return verify_ref.verify_pairs(a["q_xy"], a["r_xy"], a["qseg_offsets"], a["fwd_idx"], a["mutual"], 3.0)


def _v_verify(a):
    n_r = len(a["r_xy"])
    assert a["q_xy"].shape == (NQ_SMALL, 2) and np.isfinite(a["q_xy"]).all() and np.isfinite(a["r_xy"]).all()
    assert a["fwd_idx"].shape == a["mutual"].shape == (NQ_SMALL, 4) and a["fwd_idx"].min() >= -1 and a["fwd_idx"].max() < n_r
    _v_offsets(a["qseg_offsets"], NQ_SMALL)


T_SEQ, C_SEQ = 20, 4


def _b_sequence(which):
    r = np.random.default_rng([_seed(which), 47])
    cand = r.integers(0, 60, (T_SEQ, C_SEQ)).astype(np.int32)
    cand[:, 0] = 10 + np.arange(T_SEQ) + (3 if which == "decoy" else 0)       # a planted traversal
    cand[r.random((T_SEQ, C_SEQ)) < 0.05] = -1
    return {"cand": cand, "score": r.uniform(0.1, 1.0, (T_SEQ, C_SEQ))}


def _s_sequence(eng, a, st):
    return eng.sequence_rerank(a["cand"], a["score"], None, back=3, fwd=3, tol=1)


def _r_sequence(a):
    import sequence_ref

    from revisit_anything_amd.engine import velocity_grid

    return sequence_ref.sequence_rerank(a["cand"], a["score"], None, back=3, fwd=3, vel=velocity_grid(), tol=1)


def _v_sequence(a):
    assert a["cand"].shape == a["score"].shape == (T_SEQ, C_SEQ) and a["cand"].min() >= -1 and np.isfinite(a["score"]).all()


PARTS, K_MERGE = 3, 8


def _b_merge(which):
    r = np.random.default_rng([_seed(which), 53])
    return {"d2_parts": np.sort(r.uniform(0, 2, (NQ_SMALL, PARTS, K_MERGE)).astype(np.float32), axis=2).reshape(NQ_SMALL, -1),
            "idx_parts": r.permutation(NQ_SMALL * PARTS * K_MERGE).reshape(NQ_SMALL, -1).astype(np.int64)}


def _s_merge(eng, a, st):
    d2, idx = eng.merge_topk(a["d2_parts"], a["idx_parts"], PARTS, K_MERGE)
    return {"d2": d2, "idx": idx}


def _r_merge(a):
    import search_tail_ref

    d2, idx = search_tail_ref.merge(a["d2_parts"], a["idx_parts"], K_MERGE)
    return {"d2": d2, "idx": idx}


def _v_merge(a):
    assert a["d2_parts"].shape == a["idx_parts"].shape == (NQ_SMALL, PARTS * K_MERGE) and a["idx_parts"].min() >= 0


N_REF_VOTE = 400


def _b_lists(which):
    r = np.random.default_rng([_seed(which), 59])
    return {"d2": np.sort(r.uniform(0, 2, (NQ_SMALL, K_SEARCH)).astype(np.float32), axis=1),
            "idx": r.integers(0, N_REF_VOTE, (NQ_SMALL, K_SEARCH)).astype(np.int64)}


def _s_sims(eng, a, st):
    s, i = eng.sims_from_d2(a["d2"], a["idx"], 5)
    return {"sims": s, "idx": i}


def _r_sims(a):
    return {"sims": (np.float32(2) - a["d2"][:, :5]).astype(np.float32), "idx": a["idx"][:, :5]}


def _v_lists(a):
    assert a["d2"].shape == a["idx"].shape == (NQ_SMALL, K_SEARCH) and a["idx"].min() >= 0 and a["idx"].max() < N_REF_VOTE


def _b_minmax(which):
    r = np.random.default_rng([_seed(which), 61])
    return {"sims": r.uniform(-1, 2, 500).astype(np.float32)}


def _s_minmax(eng, a, st):
    return {"minmax": eng.minmax(a["sims"])}


def _r_minmax(a):
    return {"minmax": np.array([a["sims"].min(), a["sims"].max()], np.float32)}


def _b_vote(which):
    r = np.random.default_rng([_seed(which), 67])
    return {"idx": r.integers(0, N_REF_VOTE, (NQ_SMALL, K_SEARCH)).astype(np.int64), "sims": r.uniform(0.5, 2, (NQ_SMALL, K_SEARCH)).astype(np.float32),
            "img_of_seg": r.integers(0, 40, N_REF_VOTE).astype(np.int32), "qseg_offsets": QOFF.copy()}


def _s_vote(eng, a, st):
    pred, sc = eng.vote(a["idx"], a["sims"], a["qseg_offsets"], n_top=5, img_of_seg=a["img_of_seg"])
    return {"pred": pred, "scores": sc}


def _r_vote(a):
    import search_tail_ref

    pred, scores = search_tail_ref.vote_wt(a["idx"], a["sims"], a["qseg_offsets"], a["img_of_seg"], 5)
    return {"pred": np.asarray(pred), "scores": np.asarray(scores)}


def _v_vote(a):
    assert a["idx"].shape == a["sims"].shape == (NQ_SMALL, K_SEARCH) and a["idx"].min() >= 0 and a["idx"].max() < len(a["img_of_seg"])
    assert a["img_of_seg"].min() >= 0 and np.isfinite(a["sims"]).all()
    _v_offsets(a["qseg_offsets"], NQ_SMALL)


# db_add in two slices, db_remove by rows and by images; a fixed probe batch reads the index back
N_A, N_B, N_IMG_LIFE = 3000, 2000, 250


@functools.lru_cache(None)
def _life_probe():
    return _unit32(np.random.default_rng(71).standard_normal((40, D)))


def _b_life(which):
    r = np.random.default_rng([_seed(which), 73])
    return {"R1": _unit32(r.standard_normal((N_A, D))), "R2": _unit32(r.standard_normal((N_B, D))),
            "im1": r.integers(0, N_IMG_LIFE, N_A).astype(np.int32), "im2": r.integers(0, N_IMG_LIFE, N_B).astype(np.int32),
            "rows": r.choice(N_A + N_B, 60, replace=False).astype(np.int64), "imgs": r.choice(N_IMG_LIFE, 6, replace=False).astype(np.int32)}


def _s_life_add(which):
    def step(eng, a, st):
        if which == 1:
            eng.db_reset()
        eng.db_add(a["R%d" % which], a["im%d" % which])
        return {"n%d" % which: eng.db_size()[0]}
    return step


def _s_life_remove_rows(eng, a, st):
    n, new_ids = eng.db_remove(row_ids=a["rows"], want_new_ids=True)
    return {"removed_rows": n, "new_ids": new_ids}


def _s_life_remove_imgs(eng, a, st):
    return {"removed_imgs": eng.db_remove(img_ids=a["imgs"]), "n_left": eng.db_size()[0]}


def _s_life_probe(eng, a, st):
    d2, idx = eng.search(_life_probe(), K_SEARCH)
    return {"d2": d2, "idx": idx}


def _life_survivors(a):
    R, im = np.concatenate([a["R1"], a["R2"]]), np.concatenate([a["im1"], a["im2"]])
    keep = np.ones(len(R), bool)
    keep[a["rows"]] = False
    new_ids = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    keep2 = keep & ~np.isin(im, a["imgs"])
    return R[keep2], new_ids, int((~keep).sum()), int((keep & ~keep2).sum())


def _r_life(a):
    R, new_ids, n_rows, n_imgs = _life_survivors(a)
    d2, idx = O().knn_l2(R, _life_probe(), K_SEARCH)
    return {"d2": d2, "idx": idx, "new_ids": new_ids, "removed_rows": np.int64(n_rows), "removed_imgs": np.int64(n_imgs),
            "n1": np.int64(N_A), "n2": np.int64(N_A + N_B), "n_left": np.int64(len(R))}


def check_life(a, out, ref):
    exact(("new_ids", "removed_rows", "removed_imgs", "n1", "n2", "n_left"))(a, out, ref)
    check_knn(a, out, ref)


def _v_life(a):
    _v_rows(a, "R1", D), _v_rows(a, "R2", D)
    assert a["im1"].min() >= 0 and a["im2"].min() >= 0 and a["rows"].min() >= 0 and a["rows"].max() < N_A + N_B
    assert len(np.unique(a["rows"])) == len(a["rows"])


# ---- fixtures: what a context holds before a case's call (always from ready inputs) -----------------------------------------------
def _fx_vocab(eng):
    eng.set_vocab(vocab())
    eng.pca_set(*pca_model(), whiten=True)


def _fx_index(n, d, dup=False):
    def fx(eng):
        eng.db_reset()
        eng.db_add(*index_rows(n, d, dup))
    return fx


FIXTURES = {"": lambda eng: None, "vocab": _fx_vocab, "db20k": _fx_index(N20, D), "db40k": _fx_index(N40, D), "db40k_d96": _fx_index(N40, 96),
            "db40k_d48": _fx_index(N40, 48), "db40k_dup": _fx_index(N40, D, True), "own": lambda eng: None}
FIXTURE_ENTRIES = {}      # (an entry counts as covered only where a CASE calls it, with late inputs overwritten on return)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _mask_case(name, entries, step, ref, ints, build=_b_masks, convert="bool", valid=_v_masks, **kw):
    return Case(name, "mask", entries, build, [(step, None)], ref, valid, convert={"masks": convert} if convert else {}, check=exact(ints), **kw)


def _search_case(name, fixture, n, d, nq, plan, options=(), k=K_SEARCH, dup=False, convert=True, plan_needs_stats=False):
    return Case(name, "search", ("search",), _b_queries(n, d, nq, dup), [(_s_search(k), None)], _r_search(n, d, nq, k, dup),
                lambda a: _v_rows(a, "Q", d), fixture=fixture, convert={"Q": "strided"} if convert else {}, options=options, check=check_knn,
                plan=plan, plan_needs_stats=plan_needs_stats)


_DERIVED = dict(valid=_v_derived, fixture="db40k", convert={"Q": "strided"})

CASES = [
    # -- mask branch
    _mask_case("incidence", ("incidence",), _s_incidence, _r_incidence, ("bits",)),
    _mask_case("incidence_centroids", ("incidence_centroids",), _s_incidence_centroids, _r_incidence_centroids, ("bits", "cent")),
    _mask_case("mask_centroids", ("mask_centroids",), _s_mask_centroids, _r_mask_centroids, ("cent",)),
    Case("incidence_rle", "mask", ("incidence_rle",), _b_rle, [(_s_incidence_rle, None)], _r_incidence_rle, _v_rle, fixed=("run_offsets",),
         check=exact(("bits", "cent", "n_bad"))),
    Case("rle_decode", "mask", ("rle_decode",), _b_rle, [(_s_rle_decode, None)], _r_rle_decode, _v_rle, fixed=("run_offsets",),
         check=exact(("masks", "n_bad"))),
    _mask_case("rle_encode", ("rle_encode",), _s_rle_encode, _r_rle_encode, ("counts", "run_offsets", "areas"), convert="strided"),
    Case("rle_encode_host_counts", "mask", ("rle_encode",), _b_masks,
         [(_s_rle_encode_host(lambda total: 3, "over_"), ()), (_s_rle_encode_host(lambda total: total), None)], _r_rle_encode_host, _v_masks,
         convert={"masks": "strided"}, check=exact(("over_counts", "over_run_offsets", "over_total", "counts", "run_offsets", "total"))),
    _mask_case("mask_regions", ("mask_regions",), _s_mask_regions, _r_mask_regions, ("masks", "changed", "boxes", "area"), build=_b_masks_specks,
               convert="strided"),
    Case("adjacency", "mask", ("adjacency",), _b_cent, [(_s_adjacency(False), None)], _r_adjacency, _v_adj_in, host=("seg_offsets",),
         fixed=("seg_offsets",), convert={"cent": "f32"}, check=exact(("adj",))),
    Case("adjacency_n_empty", "mask", ("adjacency",), _b_cent, [(_s_adjacency(True), None)], _r_adjacency, _v_adj_in, host=("seg_offsets",),
         fixed=("seg_offsets",), check=exact(("adj",))),
    Case("adjacency_flagged", "mask", ("adjacency_flagged",), _b_cent, [(_s_adjacency_flagged(False), None)], _r_adjacency, _v_adj_in,
         host=("seg_offsets",), fixed=("seg_offsets",), convert={"cent": "f32"}, check=exact(("adj", "flags"))),
    Case("adjacency_flagged_device", "mask", ("adjacency_flagged",), _b_cent, [(_s_adjacency_flagged(True), None)], _r_adjacency, _v_adj_in,
         host=("seg_offsets",), fixed=("seg_offsets",), check=exact(("adj", "flags"))),
    # -- describe
    Case("images", "describe", ("images",), _b_images, [(_s_images, None)], _r_images, _v_images, host=("seg_offsets",), fixed=("seg_offsets",),
         fixture="vocab", convert={"tokens": "strided"}, check=check_describe()),
    Case("images_pca_planes", "describe", ("images_pca",), _b_images, [(_s_images_pca(False), None)], _r_images_pca, _v_images,
         host=("seg_offsets",), fixed=("seg_offsets",), fixture="vocab", options=(("pca_path", "planes", "auto"),),
         check=check_describe(desc=None, y="out")),
    Case("images_pca_project", "describe", ("images_pca",), _b_images, [(_s_images_pca(False), None)], _r_images_pca, _v_images,
         host=("seg_offsets",), fixed=("seg_offsets",), fixture="vocab", options=(("pca_path", "project", "auto"),), convert={"tokens": "strided"},
         check=check_describe(desc=None, y="out")),
    Case("images_pca_plain_fp32", "describe", ("images_pca",), _b_images, [(_s_images_pca(True), None)], _r_images_pca, _v_images,
         host=("seg_offsets",), fixed=("seg_offsets",), fixture="vocab", options=(("pca_arith", "fp32", "auto"),),
         check=check_describe(desc="desc", y="out")),
    Case("describe", "describe", ("describe",), _b_describe, [(_s_describe(True), None)], _r_describe(True), _v_describe, host=("seg_offsets",),
         fixed=("seg_offsets",), fixture="vocab", convert={"masks": "bool", "tokens": "strided"},
         check=check_describe(("bits", "cent", "adj", "flags"), desc="desc", y="out")),
    Case("describe_raw", "describe", ("describe",), _b_describe, [(_s_describe(False), None)], _r_describe(False), _v_describe,
         host=("seg_offsets",), fixed=("seg_offsets",), fixture="vocab", check=check_describe(("bits", "cent", "adj", "flags"))),
    # begin / flags / end.  include/segvlad.h: tokens, inc_bits, seg_offsets and adj are the SAME buffers from begin to end, so the
    # caller may not touch the tokens while the call is open; the masks belong to the mask branch, which describe_flags waits for:
    # they are the caller's again once describe_flags has returned (without it: once describe_end has).
    Case("describe_begin_flags_end", "describe", ("describe_begin", "describe_flags", "describe_end"), _b_describe,
         [(_s_begin, ()), (_s_flags, ("masks",)), (_s_end(False), None)], _r_describe(True), _v_describe, host=("seg_offsets",),
         fixed=("seg_offsets",), fixture="vocab", convert={"masks": "bool", "tokens": "strided"},
         check=check_describe(("bits", "cent", "adj", "flags", "cent_host", "flags_host"), desc="desc", y="out")),
    Case("describe_begin_end_patched", "describe", ("describe_begin", "describe_flags", "describe_end"), _b_describe_patched,
         [(_s_begin, ()), (_s_flags, ("masks",)), (_s_end(True), None)], _r_describe_patched, _v_describe,
         host=("seg_offsets", "patch_images", "patch_blocks"), fixed=("seg_offsets", "patch_images"), fixture="vocab",
         check=check_describe(("bits", "cent", "adj", "cent_host", "flags_host"), desc="desc", y="out")),
    Case("describe_begin_end", "describe", ("describe_begin", "describe_end"), _b_describe, [(_s_begin, ()), (_s_end(False), None)],
         _r_describe(True), _v_describe, host=("seg_offsets",), fixed=("seg_offsets",), fixture="vocab",
         check=check_describe(("bits", "cent", "adj", "flags"), desc="desc", y="out")),
    # a cancelled begin, then a whole describe on the same context: the cancel must leave nothing of the first batch behind
    Case("describe_cancel", "describe", ("describe_begin", "describe_end", "describe"), _b_describe,
         [(_s_begin, ()), (_s_cancel, ()), (_s_describe(True), None)], _r_describe(True), _v_describe, host=("seg_offsets",),
         fixed=("seg_offsets",), fixture="vocab", check=check_describe(("bits", "cent", "adj", "flags"), desc="desc", y="out")),
    Case("set_vocab", "describe", ("set_vocab", "images"), _b_vocab, [(_s_set_vocab, None), (_s_probe_images, None)], _r_set_vocab, _v_vocab,
         fixture="own", convert={"C": "strided"}, check=check_describe(), dirties_fixture=True),
    Case("pca_set", "describe", ("pca_set", "pca_apply"), _b_pca_model, [(_s_pca_set, None), (_s_probe_pca, None)], _r_pca_set, _v_pca_model,
         fixture="own", convert={"comps": "strided"}, check=check_pca_rows, dirties_fixture=True),
    Case("kmeans_step", "describe", ("kmeans_step",), _b_kmeans, [(_s_kmeans("t1"), ("t1",)), (_s_kmeans("t2"), None)], _r_kmeans, _v_kmeans,
         fixture="vocab", convert={"t1": "strided"}, check=check_kmeans),
    Case("cluster_aggregate", "describe", ("cluster_aggregate",), _b_cluster_aggregate, [(_s_cluster_aggregate, None)], _r_cluster_aggregate,
         _v_cluster_aggregate, convert={"res": "strided"}, check=check_describe()),
    Case("pca_apply", "describe", ("pca_apply",), _b_pca_rows, [(_s_pca_apply, None)], _r_pca_apply, lambda a: _v_rows(a, "X", K * D),
         fixture="vocab", convert={"X": "strided"}, check=check_pca_rows),
    Case("normalize_rows", "describe", ("normalize_rows",), _b_rows, [(_s_normalize_rows, None)], _r_normalize_rows, lambda a: _v_rows(a, "X", D),
         convert={"X": "strided"}, check=check_normalize_rows),
    # -- index and search (plans: csrc/search.hip plan_search; 32 768 rows is the matrix path's limit, 128 query rows the small plan's)
    Case("db_add_remove", "search", ("db_reset", "db_add", "db_remove", "db_size", "search"), _b_life,
         [(_s_life_add(1), ("R1", "im1")), (_s_life_add(2), ("R2", "im2")), (_s_life_remove_rows, ("rows",)), (_s_life_remove_imgs, ("imgs",)),
          (_s_life_probe, None)], _r_life, _v_life, fixture="own", convert={"R1": "strided"}, check=check_life, dirties_fixture=True),
    _search_case("search_matrix", "db20k", N20, D, 300, _plan(levels=0, filter="none")),
    _search_case("search_f16_batch", "db40k", N40, D, 300, _plan(levels=lambda v: v >= 1, filter="f16", grp_groups=lambda v: v >= 1),
                 options=(("refine_group", 1, 1),), plan_needs_stats=True),
    _search_case("search_f16_batch_rowwise", "db40k", N40, D, 300, _plan(levels=lambda v: v >= 1, filter="f16", grp_groups=0),
                 options=(("refine_group", 0, 1),), convert=False, plan_needs_stats=True),
    # (search_stats cannot tell the next two apart -- levels, filter and the redo counts are the same with and without the device
    #  head and tail, and tests/test_gpu_small_tail.py has no such figure either: the options are what selects the path here)
    _search_case("search_small", "db40k", N40, D, NQ_SMALL, _plan(levels=1, filter="f16")),
    _search_case("search_small_readback", "db40k", N40, D, NQ_SMALL, _plan(levels=1, filter="f16"),
                 options=(("small_head", 0, 1), ("small_tail", 0, 1)), convert=False),
    _search_case("search_bf16x3", "db40k_d96", N40, 96, 300, _plan(levels=lambda v: v >= 1, filter="bf16x3")),
    _search_case("search_fp32", "db40k_d48", N40, 48, 300, _plan(levels=lambda v: v >= 1, filter="fp32")),
    _search_case("search_rigorous_redo", "db40k_dup", N40, D, 160, _plan(filter="f16", n_redo=lambda v: v >= 1), k=30, dup=True, convert=False),
    Case("search_shortlist", "search", ("search_shortlist",), _b_shortlist, [(_s_shortlist, None)], _r_shortlist, host=("qseg_offsets", "shortlist"),
         fixed=("qseg_offsets",), check=check_knn, **_DERIVED),
    Case("search_excluding", "search", ("search_excluding",), _b_excluding, [(_s_excluding, None)], _r_excluding, host=("qseg_offsets", "exclude"),
         fixed=("qseg_offsets",), check=check_knn, **_DERIVED),
    Case("search_grouped", "search", ("search_grouped",), _b_queries(N40, D, NQ_SMALL), [(_s_grouped, None)], _r_grouped,
         lambda a: _v_rows(a, "Q", D), fixture="db40k", convert={"Q": "strided"}, check=check_knn),
    Case("range_search", "search", ("range_search",), _b_range, [(_s_range, None)], _r_range, lambda a: _v_rows(a, "Q", D), fixture="db40k",
         convert={"Q": "strided"}, check=check_range),
    Case("match_pairs", "search", ("match_pairs",), _b_match, [(_s_match, None)], _r_match, host=("qseg_offsets", "cand"), fixed=("qseg_offsets",),
         check=exact(("fwd_idx", "mutual", "n_mutual")), **_DERIVED),
    Case("verify_pairs", "search", ("verify_pairs",), _b_verify, [(_s_verify, None)], _r_verify, _v_verify, host=("qseg_offsets",),
         fixed=("qseg_offsets",), convert={"q_xy": "strided"}, check=check_verify),
    Case("sequence_rerank", "search", ("sequence_rerank",), _b_sequence, [(_s_sequence, None)], _r_sequence, _v_sequence, convert={"score": "strided"},
         check=all_of(exact(("n_hit", "vel", "order")), bits_equal(("seq_score",)))),
    Case("merge_topk", "search", ("merge_topk",), _b_merge, [(_s_merge, None)], _r_merge, _v_merge, convert={"d2_parts": "strided"},
         check=all_of(exact(("idx",)), bits_equal(("d2",)))),
    Case("sims_from_d2", "search", ("sims_from_d2",), _b_lists, [(_s_sims, None)], _r_sims, _v_lists, convert={"d2": "strided"},
         check=all_of(exact(("idx",)), bits_equal(("sims",)))),
    Case("minmax", "search", ("minmax",), _b_minmax, [(_s_minmax, None)], _r_minmax, lambda a: None, check=bits_equal(("minmax",))),
    Case("vote", "search", ("vote",), _b_vote, [(_s_vote, None)], _r_vote, _v_vote, host=("qseg_offsets",), fixed=("qseg_offsets",),
         convert={"sims": "strided"}, check=all_of(exact(("pred",)), bits_equal(("scores",)))),
]
BY_NAME = {c.name: c for c in CASES}
GROUPS = ("mask", "describe", "search")
ITEMS = [(c.name, v) for c in CASES for v in (("plain", "convert") if c.convert else ("plain",))]


def group_items(group):
    """The sequence of a group: every case once, in table order, the storage alternating between plain and converting."""
    out = []
    for c in CASES:
        if c.group == group:
            out.append((c.name, "convert" if c.convert and len(out) % 2 else "plain"))
    return out


# ---- coverage of the header -------------------------------------------------------------------------------------------------------
# Entries of include/segvlad.h that no case has to call, by the groups the table may leave out.
EXCLUDED = {
    "lifetime": ("version", "create", "destroy", "last_error", "set_stream", "synchronize"),
    "option": ("set_option",),
    "stats": ("search_stats", "exclude_stats", "group_stats", "range_stats"),
    "profiling": ("set_profiling", "profile_reset", "stage_ms"),
    # multi-process entries: their tests already run unguarded, in subprocesses
    "comm": ("comm_unique_id", "comm_init", "comm_destroy", "comm_info", "allgather_rows", "search_sharded", "vote_global"),
}


def header_entries():
    with open(os.path.join(ROOT, "include", "segvlad.h")) as f:
        return sorted(set(re.findall(r"^(?:const char\*|int)\s+segvlad_(\w+)\(", f.read(), flags=re.M)))


def covered_entries():
    got = set()
    for c in CASES:
        got.update(c.entries)
        got.update(FIXTURE_ENTRIES.get(c.fixture, ()))
    return got


# ==== the device side ===============================================================================================================
LEGS = ("guarded serial", "plain serial", "plain delayed")


def make_engine(guard: bool):
    """A context with the guard on or off whatever the environment says: the variable is set around the constructor only."""
    from revisit_anything_amd.engine import SegVLADEngine

    old = os.environ.get("SEGVLAD_GUARD")
    os.environ["SEGVLAD_GUARD"] = "1" if guard else "0"
    try:
        eng = SegVLADEngine(0)
    finally:
        if old is None:
            os.environ.pop("SEGVLAD_GUARD", None)
        else:
            os.environ["SEGVLAD_GUARD"] = old
    return eng       # (every option at its default, search_stats = 0 included: the library as users run it)


class Delay:
    """A chain of large GEMMs on the current stream: a condition, not a performance figure.  It must outlast the host's issue of a
    call up to its first consumer; `prove` shows that it does, with a consumer that deliberately does not wait."""

    def __init__(self, device="cuda:0", n=4096):
        import torch

        self.a = torch.randn(n, n, device=device)
        self.b = torch.randn(n, n, device=device)
        self.c = torch.empty_like(self.a)
        for _ in range(8):                      # (the first products run slower than a warm chain)
            torch.mm(self.a, self.b, out=self.c)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(16):
            torch.mm(self.a, self.b, out=self.c)
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_gemm = max(e0.elapsed_time(e1) / 16, 1e-3)

    def enqueue(self, ms: float) -> int:
        import torch

        n = int(math.ceil(1.5 * ms / self.ms_per_gemm))     # half as much again: `ms` is a lower bound, the calibration an estimate
        for _ in range(n):
            torch.mm(self.a, self.b, out=self.c)
        return n

    def prove(self, ms: float = MIN_DELAY_MS) -> dict:
        """A torch-only consumer on the default stream that does NOT wait for S must see the decoy.  It reads valid memory."""
        import torch

        x = torch.zeros(1 << 20, dtype=torch.int32, device=self.a.device)            # the decoy
        truth = torch.ones_like(x)
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            e0.record()
            n = self.enqueue(ms)
            e1.record()
            x.copy_(truth, non_blocking=True)
        y = x.clone()                                                                # default stream, no dependency on s
        torch.cuda.synchronize()
        ones = int(y.sum())
        return {"asked_ms": ms, "gemms": n, "measured_ms": e0.elapsed_time(e1), "seen": "decoy" if ones == 0 else "truth" if ones == y.numel() else "mixed"}


def _storage(arr, kind, device):
    """(base tensor, the view handed to the engine): plain storage, or one that makes the engine convert / copy."""
    import torch

    t = torch.from_numpy(np.array(arr))      # (a copy: the builders' arrays are read-only)
    if kind == "bool":
        base = torch.zeros(t.shape, dtype=torch.bool, device=device)
        return base, base
    if kind == "f32":
        base = torch.zeros(t.shape, dtype=torch.float32, device=device)
        return base, base
    if kind == "strided":
        base = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=device)
        return base, base[..., :t.shape[-1]]
    base = torch.zeros(t.shape, dtype=t.dtype, device=device)
    return base, base


class Slot:
    """One case of a sequence on one context: its device input buffers, the staged truth and decoy, its host arrays."""

    def __init__(self, name, variant, device):
        import torch

        self.case = c = BY_NAME[name]
        self.variant = variant
        data = {w: c.build(w) for w in WHICH}
        self.truth_np = data["truth"]
        self.args, self.staged = {}, {w: {} for w in WHICH}
        for n, arr in data["truth"].items():
            if n in c.host:
                self.args[n] = np.array(arr)      # a writable host array of the case's own
                for w in WHICH:
                    self.staged[w][n] = np.array(data[w][n])
            else:
                base, view = _storage(arr, c.convert.get(n) if variant == "convert" else None, device)
                self.args[n] = view
                for w in WHICH:
                    self.staged[w][n] = torch.from_numpy(np.array(data[w][n])).to(device).to(view.dtype)

    def load(self, which, names=None):
        """Enqueues (device, current stream) or performs (host, in place) the copies of `which` into the inputs."""
        for n in (self.args if names is None else names):
            if isinstance(self.args[n], np.ndarray):
                self.args[n][...] = self.staged[which][n]
            else:
                self.args[n].copy_(self.staged[which][n], non_blocking=True)

    def fillers(self, names=None):
        """Fresh tensors of every input's size, filled with the decoy on the current stream: whatever block the allocator believes
        free -- a conversion copy the engine dropped -- is handed out and overwritten."""
        import torch

        out = []
        for n in (self.args if names is None else names):
            src = self.staged["decoy"][n]
            src = torch.from_numpy(src).to(self.case_device, non_blocking=True) if isinstance(src, np.ndarray) else src
            out.append(torch.empty_like(src).copy_(src, non_blocking=True))
        return out

    @property
    def case_device(self):
        import torch

        return next(v.device for v in self.args.values() if isinstance(v, torch.Tensor))


def _to_numpy(x):
    import torch

    if isinstance(x, torch.Tensor):
        if x.dtype == torch.uint32:
            x = x.view(torch.int32)
        return x.detach().cpu().numpy()
    return np.asarray(x)


def run_leg(items, leg, delay: Optional[Delay] = None, n_streams=1, log=None, wrong_stream=False):
    """Runs the sequence `items` = [(case name, variant)] on ONE fresh context and returns [{output name: ndarray}] per item.
    leg: one of LEGS.  The serial legs run on the default stream with ready inputs and synchronise after every call; the delayed
    leg follows the module docstring, on `n_streams` side streams used in turn (wait_stream orders the old stream's work before
    the switch), with ONE synchronisation at the end.  wrong_stream (the harness's own test): the delayed calls are bound to the
    default stream instead of S, as a library that ignored its stream would issue them -- they read the decoy, valid memory."""
    import torch

    assert leg in LEGS
    eng = make_engine(guard=leg == LEGS[0])
    try:
        return _run_leg(eng, items, leg, delay, n_streams, log, wrong_stream)
    finally:
        eng.close()


def _run_leg(eng, items, leg, delay, n_streams, log, wrong_stream):
    import torch

    dev = eng.device
    slots = [Slot(n, v, dev) for n, v in items]
    torch.cuda.synchronize()
    state = {"fixture": None}

    def ensure_fixture(case):
        if case.fixture == "own" or case.fixture != state["fixture"]:
            FIXTURES[case.fixture](eng)
            state["fixture"] = None if case.dirties_fixture else case.fixture

    def call(slot, after_step=None, sync=False):
        c, st, outs = slot.case, {}, {}
        for key, val, _ in c.options:
            eng.set_option(key, val)
        remaining = [n for n in slot.args]
        for i, (fn, release) in enumerate(c.steps):
            r = fn(eng, slot.args, st)
            outs.update(r or {})
            if sync:
                eng.synchronize()
            released = remaining if (release is None or i == len(c.steps) - 1) else [n for n in release if n in remaining]
            remaining = [n for n in remaining if n not in released]
            if after_step is not None:
                after_step(slot, released)
        for key, _, val in c.options:
            eng.set_option(key, val)
        return outs

    results = []
    if leg != LEGS[2]:
        for slot in slots:
            ensure_fixture(slot.case)
            slot.load("truth")
            torch.cuda.synchronize()
            stats = leg == LEGS[1] and slot.case.plan_needs_stats
            if stats:
                eng.set_option("search_stats", 1)
            outs = call(slot, sync=True)
            torch.cuda.synchronize()
            if leg == LEGS[1] and slot.case.plan is not None:
                slot.case.plan(eng.search_stats())
            if stats:
                eng.set_option("search_stats", 0)
            results.append({k: _to_numpy(v) for k, v in outs.items()})
        return results

    # warm-up on the decoy (ready inputs), timed with events: the delay of each call is max(20 ms, 3 x its warm-up)
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    delays = []
    with torch.cuda.stream(streams[0]):
        for slot in slots:
            ensure_fixture(slot.case)
            slot.load("decoy")
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(slot)
            e1.record()
            torch.cuda.synchronize()
            delays.append(max(MIN_DELAY_MS, 3.0 * e0.elapsed_time(e1)))
    torch.cuda.synchronize()
    state["fixture"] = None
    held, pending = [], []

    def overwrite(slot, released):
        slot.load("decoy", released)
        held.append(slot.fillers(released))
        del held[:-2]                       # (older fillers go back to the allocator: their blocks are handed out again)

    if wrong_stream:
        eng._stream = lambda: eng.lib.segvlad_set_stream(eng._h, None)
    for i, slot in enumerate(slots):
        s = streams[i % n_streams]
        if n_streams > 1 and i:
            s.wait_stream(streams[(i - 1) % n_streams])     # the old stream's work is ordered before the switch
        with torch.cuda.stream(s):
            ensure_fixture(slot.case)
            delay.enqueue(delays[i])
            slot.load("truth")
            pending.append(call(slot, after_step=overwrite))
    torch.cuda.synchronize()                # the one synchronisation of the sequence
    results = [{k: _to_numpy(v) for k, v in outs.items()} for outs in pending]
    if log is not None:
        log.append({"items": len(items), "delay_ms": [round(d, 1) for d in delays]})
    return results


def compare_legs(items, by_leg):
    """guarded serial == plain serial == plain delayed, bit for bit; the message names the leg that differs."""
    problems = []
    for i, (name, variant) in enumerate(items):
        g, p, d = (by_leg[leg][i] for leg in LEGS)
        assert sorted(g) == sorted(p) == sorted(d), (name, sorted(g), sorted(p), sorted(d))
        for k in sorted(g):
            same = [x.shape == g[k].shape and x.dtype == g[k].dtype and x.tobytes() == g[k].tobytes() for x in (p[k], d[k])]
            pd = p[k].shape == d[k].shape and p[k].tobytes() == d[k].tobytes()
            if all(same):
                continue
            if not same[0] and not same[1]:
                who = "the guarded serial leg differs from both plain legs" if pd else "all three legs differ"
            else:
                who = f"the {LEGS[1] if not same[0] else LEGS[2]} leg differs from the other two"
            problems.append(f"{name}[{variant}] output '{k}': {who}")
    assert not problems, "\n".join(problems)
