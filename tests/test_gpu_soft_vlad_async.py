"""The soft kernels' stream order: the `images` and `describe` cases of tests/async_order.py (imported, not edited), replaced with
options=(("vlad_assign", "soft:10", "hard"),) and the soft reference, through that module's own three legs --

    guarded serial == plain serial == plain delayed, bit for bit

with the tokens, the incidence and the masks arriving late on a side stream and overwritten the moment the call returns: the weights
pass reads the tokens again behind the assignment pass, and must read them in the context's stream order."""
import dataclasses

import numpy as np
import pytest

import async_order as A
import soft_vlad_ref as SR
from test_gpu_async_order import _three_legs, delay  # noqa: F401  (the module's delay fixture and its three legs)

pytestmark = pytest.mark.gpu

TEMP = 10.0
SOFT = (("vlad_assign", f"soft:{TEMP:g}", "hard"),)
TAKEN = ["images", "images_pca_planes", "images_pca_plain_fp32", "describe", "describe_raw", "describe_begin_flags_end",
         "describe_begin_end_patched"]


def _soft_desc(a):
    """A._r_desc under soft assignment: fp64 descriptors of the batch given incidence bits and adjacency blocks"""
    inc = A.O().unpack_bits_u64(a["bits"].view(np.uint64), A.N_TOK)
    out, pos = [], 0
    for b in range(A.B):
        s0, s1 = int(A.SEG_OFF[b]), int(A.SEG_OFF[b + 1])
        n = s1 - s0
        out.append(SR.soft_vlad(a["tokens"][b], A.vocab(), inc[s0:s1], a["adj"][pos:pos + n * n].reshape(n, n).astype(bool), TEMP)["out"])
        pos += n * n
    return np.concatenate(out)


def _soft_case(name):
    c = A.BY_NAME[name]

    def ref(a):                      # the case's own reference with the descriptors restated (its projection, its exact outputs)
        hard, A._r_desc = A._r_desc, _soft_desc
        try:
            return c.ref(a)
        finally:
            A._r_desc = hard

    return dataclasses.replace(c, name=name + "_soft", options=tuple(c.options) + SOFT, ref=ref)


@pytest.fixture
def soft_cases():
    added = {c.name: c for c in map(_soft_case, TAKEN)}
    A.BY_NAME.update(added)
    try:
        yield added
    finally:
        for n in added:
            A.BY_NAME.pop(n, None)


@pytest.mark.parametrize("name", TAKEN)
def test_soft_case_alone(delay, soft_cases, name):  # noqa: F811
    c = soft_cases[name + "_soft"]
    variants = ["plain"] + (["convert"] if c.convert else [])
    for variant in variants:
        by_leg = _three_legs([(c.name, variant)], delay)
        truth = c.build("truth")
        c.check(truth, by_leg[A.LEGS[0]][0], c.ref(truth))         # the guarded result against the soft reference
    hard = A.run_leg([(name, "plain")], A.LEGS[1])[0]
    key = "desc" if "desc" in hard else "out"
    assert np.abs(hard[key] - by_leg[A.LEGS[1]][0][key]).max() > 1e-3      # (the option was in force)


def test_soft_cases_back_to_back_with_the_hard_ones(delay, soft_cases):  # noqa: F811
    """One sequence on one stream, soft and hard calls alternating: the option's set / restore between calls leaves no trace"""
    items = []
    for name in ("images", "describe", "describe_begin_end_patched"):
        items += [(name + "_soft", "plain"), (name, "plain")]
    _three_legs(items, delay)
