"""The preconditions of tests/test_gpu_burst_seg.py, decided on the CPU with the references alone (tests/burst_seg_ref.py), and the
Python helpers of the option vlad_burst_scope.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import burst_ref as BR
import burst_seg_ref as BS
import describe_shape_cases as T

MAIN = BS.PARAMS[0]      # (8, 7, 1): the fixed test-time setting
TWO = BS.ASSIGNS[:2]     # hard, soft:10


def test_the_restatement_agrees_with_the_engines_reference():
    from revisit_anything_amd.engine import burst_segment_reference, soft_vlad_reference

    name = "k33_d96_n129"
    d = T.build(name)
    for b in (0, 2):
        tok, inc = d["toks"][b], d["incs"][b]
        for adj in (None, d["adjs"][b]):
            for params in BS.PARAMS:
                g, u = burst_segment_reference(tok, inc, adj, *params)
                g2, u2 = BS.burst_seg(tok, inc, adj, *params)
                U = BS.union(inc, adj)
                assert g.dtype == np.float64 and g.shape == u.shape == U.shape
                assert np.allclose(g, g2, rtol=1e-13, atol=0) and np.allclose(u, u2, rtol=1e-13, atol=0)
                assert np.all(g[~U] == 0) and np.all(u[~U] == 0) and np.all(g[U] > 0)
            assert np.all(burst_segment_reference(tok, inc, adj, 8, 7, 0)[1][BS.union(inc, adj)] == 1.0)       # p = 0: exactly 1
            for pooled in (False, True):
                r = soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, parts=True, pooled=pooled, burst=MAIN, burst_scope="segment")
                ref = BS.seg_vlad(tok, d["C"], inc, adj, ("soft_pooled" if pooled else "soft", 10.0), MAIN)
                assert np.abs(r["out"] - ref["out"]).max() < 1e-12
                assert np.allclose(r["block_norms"], ref["block_norms"], rtol=1e-12, atol=1e-15)
                img = soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, pooled=pooled, burst=MAIN)
                assert np.array_equal(img, soft_vlad_reference(tok, d["C"], inc, adj, temp=10.0, pooled=pooled, burst=MAIN, burst_scope="image"))
    with pytest.raises(ValueError):
        soft_vlad_reference(d["toks"][0], d["C"], d["incs"][0], None, temp=10.0, burst=MAIN, burst_scope="Segment")


@pytest.mark.parametrize("name", ("k2_d36_n65", "k33_d96_n129", "k31_d64_n257"))
def test_one_all_token_segment_is_the_image_scope(name):
    """One segment that holds every token, order 0: g[0][n] is burst_ref.burst's g[n], sum for sum"""
    d = T.build(name)
    tok = d["toks"][0]
    inc = np.ones((1, d["N"]), dtype=bool)
    for params in BS.PARAMS:
        g, u = BS.burst_seg(tok, inc, None, *params)
        g_img, u_img = BR.burst(tok, *params)
        assert np.array_equal(g[0], g_img) and np.array_equal(u[0], u_img)
        for assign in BS.ASSIGNS:
            seg = BS.seg_vlad(tok, d["C"], inc, None, assign, params)
            img = BR.burst_vlad(tok, d["C"], inc, None, assign, params)
            assert np.array_equal(seg["out"], img["out"]) and np.array_equal(seg["block_norms"], img["block_norms"])


@pytest.mark.parametrize("name", BS.CASES)
def test_a_zero_is_a_constant_discount(name):
    """a = 0: every term is sigmoid(b), g[s][n] = |U(s)| sigmoid(b) on U(s)"""
    d = T.build(name)
    for b in (0, 2):
        for adj in (None, d["adjs"][b]):
            U = BS.union(d["incs"][b], adj)
            g = BS.burst_seg(d["toks"][b], d["incs"][b], adj, 0.0, 7.0, 1.0)[0]
            want = U * (U.sum(1, keepdims=True) / (1.0 + np.exp(-7.0)))
            assert np.allclose(g, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("params", BS.PARAMS, ids=("8_7_1", "2_0_0.5"))
@pytest.mark.parametrize("name", BS.CASES)
def test_the_fp32_restatement_keeps_the_gpu_bound_tight(name, params):
    """4 e_u_seg <= 1e-6: the device bound 1e-6 + 4 e_u_seg of tests/test_gpu_burst_seg.py stays within a factor 2 of 1e-6.  (A table
    change that breaks this changes the case, not the cap.)"""
    for assign in TWO:
        for with_adj in (True, False):
            e = BS.e_u_seg(name, assign, params, with_adj)
            print(f"{name} {params} {assign[0]} adj={int(with_adj)}: e_u_seg {e:.3e}")
            assert 4.0 * e <= 1e-6


@pytest.mark.parametrize("name", BS.CASES)
def test_the_scope_matters_on_every_case(name):
    """Segment and image scope differ by >= 1e-4 (rows of unit norm, with the adjacency) under both parameter sets and assignments: a
    device that ignored the option could not pass the end-to-end bound of 2e-6.  The order-0 figures are printed beside them."""
    for params in BS.PARAMS:
        for assign in TWO:
            moves = [float(np.abs(BS.reference(name, wa, assign, params)["out"] - BR.reference(name, wa, assign, params)["out"]).max())
                     for wa in (True, False)]
            print(f"{name} {params} {assign[0]}: max |segment - image| with adjacency {moves[0]:.3e}, order 0 {moves[1]:.3e}")
            assert moves[0] >= 1e-4


def test_the_header_documents_the_key_in_front_of_the_development_switches():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "segvlad.h")).read()
    burst, scope, dev = text.index('"vlad_burst" '), text.index('"vlad_burst_scope"'), text.index("Every other key is a DEVELOPMENT switch")
    assert burst < scope < dev
    doc = text[scope:dev]
    assert re.search(r"image \| segment", doc) and "SEGVLAD_ERR_ARG" in doc and "SEGVLAD_ERR_LIMIT" in doc
    for phrase in ("U(s)", "g[s][n]", "u[s][n]", "sigmoid(b)", "exactly 1", "labels_out", "block_norms_out", "segvlad_kmeans_step",
                   "segvlad_cluster_aggregate", "segvlad_describe_begin", "without float atomics"):
        assert phrase in doc, phrase


class _Recorder:
    """SegVLADEngine's two option methods over a recording set_option: no library, no device"""

    def __init__(self):
        from revisit_anything_amd.engine import SegVLADEngine

        self.vlad_burst_scope, self.calls = "image", []
        self._set = SegVLADEngine.set_vlad_burst_scope

    def set_option(self, key, value):
        self.calls.append((key, value))
        if key == "vlad_burst_scope":
            self.vlad_burst_scope = str(value)

    def set_vlad_burst_scope(self, *a):
        return self._set(self, *a)


def test_the_setter_refuses_on_the_host_and_returns_the_previous_value():
    from revisit_anything_amd.engine import BURST_SCOPES

    assert BURST_SCOPES == ("image", "segment")
    e = _Recorder()
    assert e.set_vlad_burst_scope("segment") == "image" and e.vlad_burst_scope == "segment"
    for bad in ("Segment", "", "seg", "image ", None, 1, True, b"segment", ("segment",), "off"):
        with pytest.raises(ValueError):
            e.set_vlad_burst_scope(bad)
        assert e.vlad_burst_scope == "segment"
    assert e.set_vlad_burst_scope("image") == "segment" and e.set_vlad_burst_scope() == "image"
    assert e.calls == [("vlad_burst_scope", "segment"), ("vlad_burst_scope", "image"), ("vlad_burst_scope", "image")]
