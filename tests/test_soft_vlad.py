"""Soft-assignment VLAD without a GPU: the fp64 restatement (tests/soft_vlad_ref.py, engine.soft_vlad_reference) against the
fixture pinned to the reference and against the oracle's hard VLAD, the header's text, and the host side of the option."""
import os
import re
import types

import numpy as np
import pytest

import describe_shape_cases as T
import soft_vlad_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_the_restatement_reproduces_the_reference_fixture():
    """tests/golden/vlad_soft.npz is VLAD.generate (utilities.py:819-890) in soft mode, extracted by tools/make_soft_vlad_golden.py:
    an fp32 reference against fp64, at the hard path's 1e-6.

    utilities.py:883-884 reduces `w * residuals` over "(q c)": cluster k's block is sum_n w[n][k] sum_c (x^_n - c_c), the residuals
    against ALL centres.  That is the option's soft_pooled (`pooled=True` of the restatement), which aggFt selects for a VLAD object;
    the fixture pins it.  soft:<T>, whose block k is taken against c_k alone, is a different descriptor -- 2e-2 to 5e-2 per component
    away at this shape, asserted below to be far from the fixture -- and is pinned by the oracle's hard VLAD instead (the saturating
    temperature, further down).  On the full 49152-d vectors of the first token set the pooled restatement is 5.1e-9 / 6.0e-9 / 1.1e-8
    from the reference at T = 1 / 10 / 100."""
    voc, toks = SR.golden_inputs()
    z = np.load(os.path.join(G, "vlad_soft.npz"))
    Gm = SR.golden_projection(voc)
    worst = worst_proj = 0.0
    for j, tok in enumerate(toks):
        for temp in SR.GOLDEN_TEMPS:
            one = np.ones((1, tok.shape[1]), bool)
            v = SR.soft_vlad(tok, voc, one, None, temp, pooled=True)["out"][0]
            err = float(np.abs(v[::37] - z[f"vlad{j}_t{int(temp)}_sub"]).max())
            perr = float(np.abs(v @ Gm - z[f"vlad{j}_t{int(temp)}_proj"]).max())
            own = float(np.abs(SR.soft_vlad(tok, voc, one, None, temp)["out"][0][::37] - z[f"vlad{j}_t{int(temp)}_sub"]).max())
            print(f"vlad{j} T={temp:g}: pooled restatement vs fixture {err:.3e} (projection {perr:.3e}); soft:<T> vs fixture {own:.3e}")
            assert own > 1e-3                                          # the two definitions are not the same descriptor
            worst, worst_proj = max(worst, err), max(worst_proj, perr)
    assert worst < 1e-6 and worst_proj < 2e-4, (worst, worst_proj)     # (the projection: tests/test_gpu_shim.py's bound of the hard fixture)


@pytest.mark.parametrize("name", ["k1_d32_n130", "k33_d96_n129"])
def test_the_pooled_restatement_is_the_sum_over_all_residuals(name):
    """soft_pooled spelt out as the reference spells it -- the [N][K][D] residual tensor, weighted and summed over tokens and centres --
    against the closed form of the restatements, with adjacency"""
    from revisit_anything_amd.engine import soft_vlad_reference

    d = T.build(name)
    tok, C, inc, adj = d["toks"][0], d["C"].astype(np.float64), d["incs"][0], d["adjs"][0]
    K, D = C.shape
    for temp in (1.0, 10.0):
        a = SR.soft_vlad(tok, C, inc, adj, temp, pooled=True)
        b = soft_vlad_reference(tok, C, inc, adj, temp, parts=True, pooled=True)
        w, xh = SR.weights(tok, C, temp)
        res = xh[:, None, :] - C[None, :, :]                                     # [N][K][D]
        U = (adj.astype(np.int64) @ inc.astype(np.int64)) > 0
        V = np.stack([np.stack([(w[U[s], k][:, None, None] * res[U[s]]).sum((0, 1)) for k in range(K)]) for s in range(inc.shape[0])])
        bn = np.linalg.norm(V, axis=2)
        out = (V / np.maximum(bn, 1e-12)[:, :, None]).reshape(inc.shape[0], K * D)
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
        for got in (a, b):
            assert np.abs(got["out"] - out).max() < 1e-12 and np.abs(got["block_norms"] - bn).max() < 1e-9 * max(1.0, bn.max())
        assert np.all(a["out"][1] == 0)


@pytest.mark.parametrize("name", ["k2_d36_n65", "k33_d96_n129", "k128_d64_n513_s129"])
def test_the_restatement_and_the_engines_agree_and_weights_sum_to_one(name):
    from revisit_anything_amd.engine import soft_vlad_reference

    d = T.build(name)
    for temp in SR.TEMPS:
        a = SR.soft_vlad(d["toks"][0], d["C"], d["incs"][0], d["adjs"][0], temp)
        b = soft_vlad_reference(d["toks"][0], d["C"], d["incs"][0], d["adjs"][0], temp, parts=True)
        assert np.abs(a["w"].sum(1) - 1).max() < 1e-14 and (a["w"] >= 0).all()
        for key in ("out", "w", "block_norms"):
            assert np.abs(a[key] - b[key]).max() < 1e-12, (name, temp, key)
        assert np.all(a["out"][1] == 0)                            # segment 1 of image 0 covers no token, with or without adj
        nrm = np.linalg.norm(a["out"], axis=1)
        assert np.abs(nrm[nrm > 0] - 1).max() < 1e-12
    with pytest.raises(ValueError):
        soft_vlad_reference(d["toks"][0], d["C"], d["incs"][0], None, 0.0)
    with pytest.raises(ValueError):
        soft_vlad_reference(d["toks"][0], d["C"][:, :-1], d["incs"][0], None, 1.0)


@pytest.mark.parametrize("with_adj", (True, False))
@pytest.mark.parametrize("name", SR.CASES)
def test_a_saturating_temperature_is_the_oracles_hard_vlad(name, with_adj):
    """T x (the table's guaranteed gap) = 120: every weight but the arg-max's is below 7.7e-53"""
    ref = T.reference(name, with_adj)
    assert ref["gap"][np.isfinite(ref["gap"])].min(initial=1.0) >= SR.MIN_GAP
    soft = SR.reference(name, with_adj, SR.SATURATING_TEMP)
    err = float(np.abs(soft["out"] - ref["out"]).max())
    print(f"{name} adj={int(with_adj)}: max|soft(T={SR.SATURATING_TEMP:g}) - hard| {err:.3e}")
    assert err < 1e-6                                              # (the oracle normalises tokens and centres in fp32)
    assert np.array_equal(soft["zero_rows"], ref["zero_rows"]) and np.all(soft["out"][soft["zero_rows"]] == 0)


def test_the_header_documents_the_option():
    h = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    at = h.index('"vlad_assign"')
    dev = h.index("Every other key is a DEVELOPMENT switch")
    assert at < dev, "vlad_assign is documented as part of the ABI, in front of the development switches"
    text = re.sub(r"\s*\n\s*\*\s*", " ", h[at:dev])
    for needle in ("hard | soft:<T>", "soft_pooled:<T>", "sum_c (x^_n - c_c)", "utilities.py:883-884", "utilities.py:862-887", "softmax over the K real centres", "padded centres take no part",
                   "sum_{n in U(s)} w[n][k] x^_n", "SEGVLAD_ERR_LIMIT", "SEGVLAD_ERR_ARG", "segvlad_kmeans_step", "segvlad_cluster_aggregate",
                   "labels_out and gap_out stay the hard", "block_norms_out"):
        assert needle in text, needle
    from revisit_anything_amd import _lib

    names = set(re.findall(r"^(?:int|const char\*) (segvlad_\w+)\(", h, flags=re.M))
    assert len(names) == 58 and names == set(_lib.SIGNATURES)                 # no entry point was added


def test_host_side_refusals_of_set_vlad_assign():
    from revisit_anything_amd.engine import vlad_assign_value

    assert vlad_assign_value() == "hard" and vlad_assign_value("hard") == "hard"
    assert vlad_assign_value("soft_pooled", 10.0) == "soft_pooled:1.0e+01"
    for temp, want in ((1, "soft:1.0e+00"), (10.0, "soft:1.0e+01"), (np.float32(0.1), "soft:1.0e-01"), (1e30, "soft:1.0e+30")):
        v = vlad_assign_value("soft", temp)
        assert v == want and np.float32(float(v[5:])) == np.float32(temp)
    for mode, temp in (("soft", None), ("soft", 0), ("soft", -1.0), ("soft", float("nan")), ("soft", float("inf")), ("soft", 1e50), ("soft", 1e-50),
                       ("soft", "10"), ("soft", True), ("soft", [1.0, 2.0]), ("Soft", 1.0), ("soft:", 1.0), ("", 1.0), ("hard", 1.0), (None, None),
                       ("soft_pooled", None), ("soft_pooled", 0.0), ("soft_pooled:", 1.0), ("Soft_pooled", 1.0), ("pooled", 1.0)):
        with pytest.raises(ValueError):
            vlad_assign_value(mode, temp)


class _StubEngine:
    """What func_vpr.aggFt needs of an engine: records the option's values, returns zero descriptors"""

    def __init__(self):
        import torch

        self.device, self.K, self.D, self.vlad_assign, self.log, self.torch = torch.device("cpu"), 0, 0, "hard", [], torch
        self.vocab_generation = 0

    def set_vocab(self, c):
        self.K, self.D = c.shape
        self.vocab_generation += 1

    def set_option(self, key, value):
        assert key == "vlad_assign"
        self.log.append(str(value))
        self.vlad_assign = str(value)

    def set_vlad_assign(self, mode="hard", temp=None):
        from revisit_anything_amd.engine import vlad_assign_value

        before = self.vlad_assign
        self.set_option("vlad_assign", vlad_assign_value(mode, temp))
        return before

    def seg_vlad(self, tok, bits, offs, adj, **kw):
        self.log.append(("seg_vlad", self.vlad_assign))
        return {"out": self.torch.zeros((len(offs) - 1, self.K * self.D))}


def test_aggFt_sets_and_restores_the_option_and_refuses_what_it_cannot_honour(monkeypatch):
    import torch

    import revisit_anything_amd.func_vpr as fv

    stub = _StubEngine()
    monkeypatch.setattr(fv, "engine", lambda: stub)
    monkeypatch.setattr(fv, "_set_vocab", lambda c: stub.set_vocab(c))
    voc = np.random.default_rng(0).standard_normal((4, 8)).astype(np.float32)
    h5 = {"a.jpg": {"ift_dino": np.ones((1, 8, 2, 3), np.float32)}}

    def vlad(**kw):
        base = dict(c_centers=torch.from_numpy(voc), num_clusters=4, desc_dim=8, intra_norm=True, norm_descs=True, mode="cosine",
                    vlad_mode="hard", soft_temp=1.0)
        base.update(kw)
        return types.SimpleNamespace(**base)

    out = fv.aggFt(h5, None, None, {}, "vlad", vlad(vlad_mode="soft", soft_temp=10.0))
    assert len(out) == 1 and stub.log == ["soft_pooled:1.0e+01", ("seg_vlad", "soft_pooled:1.0e+01"), "hard"] and stub.vlad_assign == "hard"
    # the option the caller had set comes back, whatever the object asks for; bare centres leave it alone
    stub.vlad_assign, stub.log = "soft:2.0e+00", []
    fv.aggFt(h5, None, None, {}, "vlad", vlad())
    assert stub.log == ["hard", ("seg_vlad", "hard"), "soft:2.0e+00"]
    stub.vlad_assign, stub.log = "hard", []
    fv.aggFt(h5, None, None, {}, "vlad", torch.from_numpy(voc))
    assert stub.log == ["hard", ("seg_vlad", "hard"), "hard"]                  # a bare tensor of centres means hard
    # restored when the call fails, too
    stub.log = []
    monkeypatch.setattr(stub, "seg_vlad", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError):
        fv.aggFt(h5, None, None, {}, "vlad", vlad(vlad_mode="soft", soft_temp=3.0))
    assert stub.vlad_assign == "hard"
    for bad in (dict(intra_norm=False), dict(norm_descs=False), dict(mode="euclidean"), dict(dist_mode="euclidean"), dict(vlad_mode="fuzzy")):
        with pytest.raises(NotImplementedError):
            fv.aggFt(h5, None, None, {}, "vlad", vlad(**bad))
    with pytest.raises(ValueError):
        fv.aggFt(h5, None, None, {}, "vlad", vlad(vlad_mode="soft", soft_temp=0.0))
    assert stub.vlad_assign == "hard"
