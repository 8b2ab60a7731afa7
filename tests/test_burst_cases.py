"""The preconditions of tests/test_gpu_burst.py, decided on the CPU with the references alone (tests/burst_ref.py), and the Python
helpers of the option vlad_burst.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import burst_ref as BR
import describe_shape_cases as T
import soft_vlad_ref as SR

MAIN = BR.PARAMS[0]      # (8, 7, 1): the fixed test-time setting


@pytest.mark.parametrize("name", BR.CASES)
def test_the_burst_matters_on_every_case(name):
    """At (8, 7, 1) the discount moves the descriptor by >= 1e-4 under every assignment, and u spreads by >= 1.2 in every image:
    a device that ignored the option, or applied a constant, could not pass the end-to-end bounds (1e-6)."""
    d = T.build(name)
    ratios = [float(u.max() / u.min()) for u in (BR.burst(t, *MAIN)[1] for t in d["toks"][:3])]
    moves = [float(np.abs(BR.reference(name, wa, assign, MAIN)["out"] - BR.reference(name, wa, assign, None)["out"]).max())
             for assign in BR.ASSIGNS for wa in (True, False)]
    print(f"{name}: max u / min u per image {np.round(ratios, 3)}, max |burst - plain| per (assign, adj) {['%.2e' % m for m in moves]}")
    assert min(ratios) >= 1.2
    assert min(moves) >= 1e-4


def test_without_the_option_the_restatement_is_soft_vlad_refs():
    for name in ("k2_d36_n65", "k33_d96_n129"):
        for assign in BR.ASSIGNS[1:]:
            ours, theirs = BR.reference(name, True, assign, None), SR.reference(name, True, assign[1], assign[0] == "soft_pooled")
            assert np.array_equal(ours["out"], theirs["out"]) and np.array_equal(ours["block_norms"], theirs["block_norms"])
        hard = T.reference(name, True)
        assert np.abs(BR.reference(name, True, BR.ASSIGNS[0], None)["out"] - hard["out"]).max() < 1e-6     # (the oracle is fp32 in parts)


@pytest.mark.parametrize("params", BR.PARAMS, ids=("8_7_1", "2_0_0.5"))
@pytest.mark.parametrize("name", BR.CASES)
def test_fp32_stays_within_the_weight_bound(name, params):
    """Sequential fp32 chains -- the plainest arithmetic of the format -- keep u within rtol = 1e-5 + 2 p a sqrt(D) 2^-24"""
    d = T.build(name)
    worst = 0.0
    for b, u32 in enumerate(BR.case_u_fp32(name, params)[:3]):
        u = BR.burst(d["toks"][b], *params)[1]
        worst = max(worst, float((np.abs(u32 - u) / u).max()))
    bound = BR.weight_rtol(d["D"], params)
    print(f"{name} {params}: fp32 u off by {worst:.3e} relative (bound {bound:.3e})")
    assert worst <= bound


@pytest.mark.parametrize("nd", BR.PROBES, ids=BR.probe_id)
def test_probe_tokens_qualify(nd):
    """Every probe token has a top-2 gap >= MIN_GAP (its fp32 label is the fp64 one), is covered by exactly one single-token
    segment, and no image holds more than 400 segments"""
    N, D = nd
    d = BR.probe(N, D)
    gap = BR.probe_gap(N, D)
    print(f"{BR.probe_id(nd)}: min gap {gap.min():.3e}, segment offsets {d['offs'].tolist()}")
    assert gap.min() >= SR.MIN_GAP
    from oracle import segvlad_oracle as O

    inc = O.unpack_bits_u64(d["bits"].view(np.uint64), N)
    assert inc.shape == (N, N) and np.array_equal(inc, np.eye(N, dtype=bool))
    assert np.diff(d["offs"]).max() <= BR.PROBE_SEGS and d["tok"].shape == (len(d["offs"]) - 1, D, N)
    for params in BR.PARAMS:
        ref = BR.probe_block_norms(N, D, params)
        assert np.all((ref > 0).sum(1) == 1)


def test_vlad_burst_value_round_trips_and_refuses():
    from revisit_anything_amd.engine import vlad_burst_value

    for abp in ((8, 7, 1), (2.0, 0.0, 0.5), (0, -8, 0), (64, 16, 2), (0.1, -0.3, 1.7), (np.float32(1 / 3), 1e-3, 2)):
        fields = vlad_burst_value(*abp).split(":")
        assert len(fields) == 3
        for f, x in zip(fields, abp):
            assert np.float32(f) == np.float32(x) and set(f) <= set("0123456789.e+-"), (f, x)
    assert vlad_burst_value(8, 7, 1) == "8.0e+00:7.0e+00:1.0e+00"
    for bad in ((None, 7, 1), (8, None, 1), (8, 7, None), ("8", 7, 1), (True, 7, 1), (float("nan"), 7, 1), (8, float("inf"), 1), (-1, 7, 1),
                (65, 7, 1), (8, -9, 1), (8, 17, 1), (8, 7, 2.5), (8, 7, -0.1), (1e50, 7, 1), ([8], 7, 1)):
        with pytest.raises(ValueError):
            vlad_burst_value(*bad)


def test_burst_reference_and_the_soft_references_burst_argument():
    from revisit_anything_amd.engine import burst_reference, soft_vlad_reference

    name = "k33_d96_n129"
    d = T.build(name)
    tok, inc, adj = d["toks"][0], d["incs"][0], d["adjs"][0]
    g, u = burst_reference(tok, *MAIN)
    g2, u2 = BR.burst(tok, *MAIN)
    assert g.dtype == np.float64 and np.allclose(g, g2, rtol=1e-13, atol=0) and np.allclose(u, u2, rtol=1e-13, atol=0)
    assert np.all(burst_reference(tok, 8, 7, 0)[1] == 1.0)
    g0 = burst_reference(tok, 0, 7, 1)[0]
    assert np.allclose(g0, tok.shape[1] / (1.0 + np.exp(-7.0)), rtol=1e-13, atol=0)      # a = 0: N sigmoid(b), whatever the tokens
    for pooled in (False, True):
        r = soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, parts=True, pooled=pooled, burst=MAIN)
        ref = BR.burst_vlad(tok, d["C"], inc, adj, ("soft_pooled" if pooled else "soft", 10.0), MAIN)
        assert np.abs(r["out"] - ref["out"]).max() < 1e-12 and np.allclose(r["block_norms"], ref["block_norms"], rtol=1e-12, atol=1e-15)


def _soft_vlad_reference_before(tokens, centres, inc, adj, temp, pooled):
    """engine.soft_vlad_reference as it stood before it took ``burst=``: the same operations in the same order"""
    X = np.asarray(tokens).astype(np.float64).T
    Cm = np.asarray(centres).astype(np.float64)
    inc = np.asarray(inc).astype(bool)
    S, (K, D) = inc.shape[0], Cm.shape
    xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
    ch = Cm / np.maximum(np.linalg.norm(Cm, axis=1, keepdims=True), 1e-12)
    z = float(temp) * (xh @ ch.T)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    U = inc if adj is None else (np.asarray(adj).astype(np.float64).reshape(S, S) @ inc.astype(np.float64)) > 0
    Uf = U.astype(np.float64)
    V = np.einsum("sn,nk,nd->skd", Uf, w, xh, optimize=True)
    V = K * V - (Uf @ w)[:, :, None] * Cm.sum(0)[None, None] if pooled else V - (Uf @ w)[:, :, None] * Cm[None]
    bn = np.linalg.norm(V, axis=2)
    V = V / np.maximum(bn, 1e-12)[:, :, None]
    out = V.reshape(S, K * D)
    return out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12), w, bn


def test_the_soft_references_default_result_is_unchanged():
    from revisit_anything_amd.engine import soft_vlad_reference

    d = T.build("k33_d96_n129")
    tok, inc = d["toks"][2], d["incs"][2]
    for adj in (None, d["adjs"][2]):
        for pooled in (False, True):
            out, w, bn = _soft_vlad_reference_before(tok, d["C"], inc, adj, 10.0, pooled)
            assert np.array_equal(soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, pooled=pooled), out)
            r = soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, parts=True, pooled=pooled, burst=None)
            assert np.array_equal(r["out"], out) and np.array_equal(r["w"], w) and np.array_equal(r["block_norms"], bn)
