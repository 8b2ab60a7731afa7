"""segvlad_cluster_aggregate against oracle.vlad_matmuls_per_cluster (fp64) over the table of tests/cluster_aggregate_cases.py:
num_c from 1 to 256 -- set_vocab ends at 128, so labels 128 .. 255, prep_kernel's kcnt[] at K = 256 and the aggregation grid
beyond 32 workgroups run through this entry alone -- at D = 4 .. 132 that are no multiple of 32 or of 128, without a vocabulary in
the context.  tests/test_cluster_aggregate_cases.py has shown with the oracle alone that every non-empty block has norm >= 1e-2,
so no block is left out, and that folding the top label to 7 bits moves the reference by more than 1e4 times the bound.

Bound (not new: DESC_TOL of tests/test_gpu_describe_shapes.py, tests/test_gpu_shim.py): max |out - ref| < 2e-6; rows of segments
without a token in their neighbourhood exactly 0.  Each case runs with adj = None and with its adjacency, from host arrays and
from device tensors, into an output that is pre-filled with NaN (through the C entry: the wrapper allocates its own), and
once through SegVLADEngine.cluster_aggregate, whose bits must be the same.

Measured on an MI355X (max |out - ref|, held to 2e-6; host arrays and device tensors give the same figures; no entry was left NaN):
  case                 adj=None  with adjacency
  c1_d4_n65_s3         4.7e-08   4.7e-08
  c5_d36_n200_s9       4.4e-08   3.8e-08
  c129_d36_n300_s37    1.3e-08   9.8e-09
  c200_d132_n513_s70   6.0e-09   4.5e-09
  c255_d64_n257_s9     9.0e-09   9.0e-09
  c256_d32_n1030_s129  8.5e-09   7.4e-09
"""
import numpy as np
import pytest
import torch

import cluster_aggregate_cases as T

pytestmark = pytest.mark.gpu

DESC_TOL = 2e-6


def _call(eng, d, adj, device):
    """The C entry into a NaN-filled output; operands and output on the host or on the device"""
    from revisit_anything_amd.engine import _ptr

    S, K, D, N = d["S"], d["num_c"], d["D"], d["N"]
    ops = [d["res"], d["labels"], d["bits"], adj]
    out = np.full((S, K * D), np.nan, np.float32)
    if device:
        ops = [None if a is None else torch.from_numpy(a).to(eng.device) for a in ops]
        out = torch.from_numpy(out).to(eng.device)
    res, lab, bits, a = ops
    eng._stream()
    eng._check(eng.lib.segvlad_cluster_aggregate(eng._h, K, _ptr(res), _ptr(lab), N, D, _ptr(bits), S, _ptr(a), _ptr(out)), "cluster_aggregate")
    return out.cpu().numpy() if device else out


@pytest.mark.parametrize("name", T.NAMES)
def test_cluster_aggregate_against_the_oracle(name):
    from revisit_anything_amd.engine import SegVLADEngine

    d = T.build(name)
    facts = T.launch_facts(d["case"])
    assert all(facts[key] == want for key, want in d["case"]["expect"].items()), name
    assert d["labels"].max() == d["num_c"] - 1
    eng = SegVLADEngine(0)         # no vocabulary: the entry does not use the context's
    try:
        for with_adj in (False, True):
            ref, _, zero = T.reference(name, with_adj)
            adj = d["adj"] if with_adj else None
            outs = {}
            for device in (False, True):
                out = outs[device] = _call(eng, d, adj, device)
                tag = f"{name} adj={int(with_adj)} {'device' if device else 'host'}"
                n_nan = int(np.isnan(out).sum())
                err = float(np.abs(out - ref).max()) if not n_nan else float("nan")
                print(f"{tag}: unwritten (NaN) entries {n_nan}, max|out-ref| {err:.3e} (bound {DESC_TOL:.0e}), rows exactly 0: {int(zero.sum())}")
                assert n_nan == 0, tag
                assert out.shape == ref.shape and err < DESC_TOL, tag
                assert zero[1] and np.all(out[zero] == 0), tag
            wrapped = eng.cluster_aggregate(d["num_c"], d["res"], d["labels"], d["bits"], adj).cpu().numpy()
            for device in (False, True):
                assert np.array_equal(outs[device].view(np.uint32), wrapped.view(np.uint32)), (name, with_adj, device)
    finally:
        eng.close()
