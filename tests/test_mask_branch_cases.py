"""Preconditions of tests/test_gpu_mask_branch.py, decided by references alone (no GPU): every incidence case of
tests/mask_branch_cases.py reaches the branch it is named for and its oracle row is what the reference's own operations give
(torch's nearest interpolate -> argwhere -> the pixel -> token map); every adjacency image is classified by the exact empty-circle
rule, and for the generic ones that rule agrees with Qhull before the device is asked.  The tests print the facts of every case and
the class and margin of every adjacency image, with the capture disabled: they are part of a run's output."""
import math

import numpy as np
import pytest
import torch

import mask_branch_cases as T


def _O():
    from oracle import segvlad_oracle as O

    return O


def _show(capsys, text):
    with capsys.disabled():
        print(text)


def reference_incidence_torch(masks, H, W, patch):
    """func_vpr.py:1088-1092 with the pixel -> token map of place_rec_main.py:187-194, on the CPU: nearest interpolate of the float
    masks to the image, argwhere, then mask_idx[segment, ind[pixel]] = True"""
    dh, dw = H // patch, W // patch
    idx = np.empty((H, W, 2), np.int64)
    idx[:, :, 0] = np.clip(np.arange(H) // patch, 0, dh - 1)[:, None]
    idx[:, :, 1] = np.clip(np.arange(W) // patch, 0, dw - 1)[None, :]
    ind = torch.from_numpy(np.ravel_multi_index(idx.reshape(-1, 2).T, (dh, dw)))
    m = torch.tensor(masks)
    up = torch.nn.functional.interpolate(m.float().unsqueeze(0), [H, W], mode="nearest").squeeze(0).bool().reshape(len(masks), -1)
    out = torch.zeros((len(masks), dh * dw), dtype=torch.bool)
    flat = torch.argwhere(up)
    out[flat[:, 0], ind[flat[:, 1]]] = True
    return out.numpy()


def test_the_incidence_table_reaches_every_branch(capsys):
    assert len(set(T.INC_NAMES)) == len(T.INC_NAMES)
    reached = set()
    for c in T.INCIDENCE_CASES:
        b = T.incidence_branches(c)
        _show(capsys, "%-24s %s" % (c["name"], " | ".join(sorted(b))))
        reached |= b
    assert reached == T.INCIDENCE_BRANCHES, (T.INCIDENCE_BRANCHES - reached, reached - T.INCIDENCE_BRANCHES)
    # the misaligned case is the first case's masks, moved by one byte
    assert np.array_equal(T.build_masks("unfused_misaligned")[0], T.build_masks("fused_ranges_small")[0])
    # nothing larger than the issue's largest masks, and a few megabytes per case at the most
    assert max(c["Hm"] * c["Wm"] for c in T.INCIDENCE_CASES) == 1216 * 1024
    assert max(T.build_masks(n)[0].nbytes for n in T.INC_NAMES) < 12 * 2 ** 20


@pytest.mark.parametrize("name", T.INC_NAMES)
def test_incidence_case_qualifies(name, capsys):
    c = T.INC_BY_NAME[name]
    facts = T.launch_facts(c)
    _show(capsys, "%-24s %s" % (name, " ".join("%s=%s" % (k, facts[k]) for k in (
        "fused", "why", "lds", "lds_over_64k", "ranges", "scale", "N", "nw", "grid_y", "passes", "last_pass_tokens", "S_total"))))
    for key, want in c["expect"].items():
        assert facts[key] == want, (name, key, facts[key], want)
    m, where = T.build_masks(name)
    inc, cent = T.incidence_reference(name)
    H, W, patch, Hm, Wm, S = c["H"], c["W"], c["patch"], c["Hm"], c["Wm"], c["S"]
    dh, dw, N = facts["dh"], facts["dw"], facts["N"]
    assert m.shape == (facts["S_total"], Hm, Wm) and inc.shape == (len(m), N) and cent.shape == (len(m), 2)
    if len(m) == 0:
        return
    # the oracle is the reference's operation at this shape
    assert np.array_equal(inc, reference_incidence_torch(m, H, W, patch))
    if S:
        assert set(np.unique(m[:S])) == {0, 1, 2, 128, 255} or S * Hm * Wm < 2000
        assert m[:S].reshape(S, -1).any(1).all()
    if not c["specials"]:
        return
    assert list(where) == T.special_roles(c) and sorted(where.values()) == list(range(S, len(m)))
    tok = inc.reshape(len(m), dh, dw)
    # the corner pixels: one pixel each; the first one is read by the first token (dst 0 -> src 0), whatever the scale
    for k in range(4):
        assert m[where["corner%d" % k]].sum() == 255
    assert tok[where["corner0"], 0, 0] and tok[where["corner0"]].sum() == 1
    for k, (ty, tx) in enumerate(((0, 0), (0, dw - 1), (dh - 1, 0), (dh - 1, dw - 1))):
        got = tok[where["corner%d" % k]]
        assert got.sum() <= 1 and (got.sum() == 0 or got[ty, tx]), (name, k)     # (a corner that down-sampling never reads: no token)
    # the ragged strip: tokens of the last row / column only, and at least one
    assert ("strip" in where) == (name in ("fused_ranges_small", "fused_walk_down_down", "fused_walk_up_down", "fused_walk_down_up",
                                           "fused_n1530", "unfused_wm_up", "unfused_misaligned", "patch16", "patch8"))
    if "strip" in where:
        got = tok[where["strip"]]
        assert got.any() and not got[:dh - 1, :dw - 1].any(), name
        if facts["ragged_h"] and len(T._sampling(c)[0][1]):
            assert got[dh - 1].all()
        if facts["ragged_w"] and len(T._sampling(c)[1][1]):
            assert got[:, dw - 1].all()
    # all ones / all zeros
    assert inc[where["ones"]].all() and cent[where["ones"]].tolist() == [(Wm - 1) / 2, (Hm - 1) / 2]
    assert not inc[where["zeros"]].any() and np.isnan(cent[where["zeros"]]).all()
    assert not np.isnan(np.delete(cent, where["zeros"], axis=0)).any()
    # pixels that nearest sampling never reads: there are some wherever an axis is down-sampled, and they set no token
    assert ("unsampled" in where) == ("down" in facts["scale"])
    if "unsampled" in where:
        u = m[where["unsampled"]]
        assert u.any() and not inc[where["unsampled"]].any()
        ys, xs = np.nonzero(u)
        assert cent[where["unsampled"]].tolist() == [xs.mean(), ys.mean()]


def test_the_adjacency_bound():
    """sv_adjacency_lds: the last size that fits the 160 KiB of a CU, and the first that asks for more than the default 64 KiB"""
    assert T.adjacency_lds(T.S_LIMIT) == 163600 <= 160 * 1024 < T.adjacency_lds(T.S_LIMIT + 1) == 163856
    assert T.adjacency_lds(T.S_LDS_ATTR - 1) <= 64 * 1024 < T.adjacency_lds(T.S_LDS_ATTR)
    assert all(T.adjacency_lds(s) <= 160 * 1024 for s in range(1, T.S_LIMIT + 1))


def test_the_exact_rule_in_its_two_forms():
    """The vectorised int64 form and the Python-integer form of the rule agree wherever both apply; the closure on integer matrices
    is matrix_power(A1, order) > 0."""
    for name in ("degenerate", "order6"):
        for img in T.adjacency_batches()[name]["images"]:
            a, b = T.exact_delaunay(img), T.exact_delaunay(img, force_python=True)
            assert np.array_equal(a["A1"], b["A1"]) and (a["duplicate"], a["cocircular"]) == (b["duplicate"], b["cocircular"])
            assert a["margin"] == b["margin"] or abs(a["margin"] - b["margin"]) <= 1e-9 * b["margin"]
            for order in T.ORDERS:
                want = np.linalg.matrix_power(a["A1"].astype(np.int64), order) > 0
                assert np.array_equal(T.closure(a["A1"], order), want)
    big = T.batch_classes("s385")[0][2]["A1"]          # (the BLAS form of the closure, used above 200 points)
    assert np.array_equal(T.closure(big, 3), np.linalg.matrix_power(big.astype(np.int64), 3) > 0)
    for S in range(4):
        blk = T.small_image_block(S)
        assert blk.shape == (S, S) and np.array_equal(blk, _O().adjacency_from_centroids(np.zeros((S, 2)), 5))


@pytest.mark.parametrize("name", T.ADJ_NAMES)
def test_adjacency_batch_qualifies(name, capsys):
    b = T.adjacency_batches()[name]
    facts = T.adjacency_facts(b)
    _show(capsys, "%-15s %s" % (name, " ".join("%s=%s" % kv for kv in facts.items())))
    for key, want in b["expect"].items():
        assert facts[key] == want, (name, key, facts[key], want)
    assert facts["fits"]
    classes = T.batch_classes(name)
    for i, (img, (cl, margin, ex)) in enumerate(zip(b["images"], classes)):
        _show(capsys, "    image %2d  S=%3d  %-10s margin %.3g" % (i, len(img), cl, margin))
        assert cl != "unclassified", (name, i, margin)
        assert cl == {0: "empty", 1: "small", 2: "small", 3: "small"}.get(len(img), cl)
        if cl == "generic":
            assert margin >= T.MARGIN and not ex["duplicate"] and not ex["cocircular"]
            # the exact rule and the reference's library agree before the device is asked
            assert np.array_equal(ex["A1"], _O().adjacency_from_centroids(img, 1)), (name, i)
            assert np.array_equal(ex["A1"], ex["A1"].T) and ex["A1"].diagonal().all()
    got = [cl for cl, _, _ in classes]
    if name == "ladder":
        assert [len(i) for i in b["images"]] == list(T.LADDER)
        assert all(np.all(i * 16 == np.round(i * 16)) for i in b["images"])
    elif name == "mask_centroids":
        assert [len(i) for i in b["images"]] == [30, 50] and got == ["generic", "generic"]
        assert any(Frac(float(x)).denominator > 2 ** 20 for x in b["images"][1].ravel())     # means, not lattice points
    elif name in ("b65", "b64"):
        sizes = [len(i) for i in b["images"]]
        assert min(sizes) >= 4 and max(sizes) <= 40 and set(got) == {"generic"}
        assert all(np.array_equal(x, y) for x, y in zip(T.adjacency_batches()["b65"]["images"], T.adjacency_batches()["b64"]["images"]))
    elif name == "s_limit":
        pts = b["images"][0]
        assert np.array_equal(pts, np.round(pts)) and pts.min() >= 0 and pts.max() < 4096 and len(np.unique(pts, axis=0)) == T.S_LIMIT
        assert got == ["generic"]
    elif name == "degenerate":
        want = ["degenerate" if i in T.DEGENERATE_AT else "generic" for i in range(len(got))]
        assert got == want and list(T.DEGENERATE_IMAGES) == list(T.DEGENERATE_AT.values())
        assert classes[5][2]["duplicate"] and not classes[5][2]["cocircular"]
        # exact in the kernel's fp64 too (small integers), so the device test also compares their blocks, ties kept: both diagonals
        # of the rectangles, the link between the duplicates
        assert all(np.array_equal(b["images"][i], np.round(b["images"][i])) and np.abs(b["images"][i]).max() < 128 for i in T.DEGENERATE_AT)
        assert all(classes[i][2]["A1"][0, 2] and classes[i][2]["A1"][1, 3] for i in (1, 3)) and classes[5][2]["A1"][1, 2]
        assert all(classes[i][2]["cocircular"] and not classes[i][2]["duplicate"] for i in (1, 3, 7, 9))
        # the collinear image: the middle point blocks the outer pair, every other pair of the triple is an edge
        A = classes[11][2]["A1"]
        assert not A[0, 2] and A[0, 1] and A[1, 2]
        # the turned rectangle has no side parallel to an axis
        r = T.RECT_TURNED[:4]
        assert all((r[k] != r[(k + 1) % 4]).all() for k in range(4))
    elif name == "nan":
        assert got == ["generic", "nan", "generic"]
    elif name == "order6":
        assert [len(i) for i in b["images"]] == [20, 5] and b["orders"] == (6,)
        for img, (_, _, ex) in zip(b["images"], classes):
            assert T.closure(ex["A1"], 6).all() and not ex["A1"].all()


def Frac(x):
    from fractions import Fraction

    return Fraction(x)


def test_the_adjacency_table_reaches_every_branch(capsys):
    reached = set()
    for name in T.ADJ_NAMES:
        b = T.adjacency_branches(T.adjacency_batches()[name])
        _show(capsys, "%-15s %s" % (name, " | ".join(sorted(b))))
        reached |= b
    assert reached == T.ADJACENCY_BRANCHES, (T.ADJACENCY_BRANCHES - reached, reached - T.ADJACENCY_BRANCHES)
    assert set(T.ADJ_NAMES) == set(T.adjacency_batches())
    assert all(set(b["orders"]) <= set(T.ORDERS) for b in T.adjacency_batches().values())
    assert math.isinf(T.classify(np.zeros((0, 2)))[1])


def test_a_rounded_rotation_of_the_rectangle_cannot_be_in_the_table():
    """The lattice rectangle turned by 0.7312 rad in fp64 (tests/test_gpu_parity.py flags it on the device): its rounded corners are
    not exactly co-circular, and the exact |tmax - tmin| of its diagonals is about 0.4 of the kernel's rounding bound -- neither
    'degenerate' nor 'generic' by this table's rules, which is why the table's turned rectangle has integer corners."""
    th = 0.7312
    rot = T.RECT @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T + np.array([100.0, 50.0])
    cl, margin, _ = T.classify(rot)
    assert cl == "unclassified" and 0 < margin < 1
