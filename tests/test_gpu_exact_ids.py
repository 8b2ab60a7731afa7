"""kNN ids WITHOUT a near-tie allowance: at 1 M x 1024 the device's (distance, id) lists must equal, bit for bit
and ties included, the lists a host emulation of the device's documented fp32 arithmetic produces (tests/fp32_emu.py: the
sequential fma chain, the row_sumsq lane order, sv_d2 with faiss's clamp) -- on 64 queries of the three kinds (planted, random,
near-copies), for the batch search, the single-image pass and the fp32 filter.

The emulation runs on the CONTESTED rows only (tests/fp32_emu.py: check_contested): per query every row whose distance by a
plain fp32 GEMM lies near the k-th smallest, typically 200-400 rows; the fp64 oracle stays beside it."""
import pytest
import torch

import fp32_emu as E

pytestmark = pytest.mark.gpu


def _data():
    dev = torch.device("cuda:0")
    n_img, S, d, group = 20000, 50, 1024, 4
    g = torch.Generator(device=dev)
    g.manual_seed(3000)
    R = torch.empty(n_img * S, d, device=dev)
    for g0 in range(0, n_img // group, 500):
        ng = min(500, n_img // group - g0)
        base = torch.nn.functional.normalize(torch.randn(ng, 1, S, d, device=dev, generator=g), dim=3)
        blk = base + (0.05 / d ** 0.5) * torch.randn(ng, group, S, d, device=dev, generator=g)
        R[g0 * group * S:(g0 + ng) * group * S] = torch.nn.functional.normalize(blk, dim=3).reshape(-1, d)
    gq = torch.Generator(device=dev)
    gq.manual_seed(4100)
    tau = torch.randint(0, n_img * S, (40,), device=dev, generator=gq)
    q_pl = torch.nn.functional.normalize(R[tau] + (4.0 / d ** 0.5) * torch.randn(40, d, device=dev, generator=gq), dim=1)
    q_rand = torch.nn.functional.normalize(torch.randn(12, d, device=dev, generator=gq), dim=1)
    src = torch.randint(0, n_img * S, (12,), device=dev, generator=gq)
    q_dup = torch.nn.functional.normalize(R[src] + (0.02 / d ** 0.5) * torch.randn(12, d, device=dev, generator=gq), dim=1)
    Q = torch.cat([q_pl, q_rand, q_dup]).contiguous()
    R[777_777] = R[123_456]                     # an exact duplicate pair: a genuine tie that only the id can break
    Q[0] = torch.nn.functional.normalize(R[123_456] + (1.0 / d ** 0.5) * torch.randn(d, device=dev, generator=gq), dim=0)
    return R, Q


def test_device_ids_equal_the_emulated_fp32_arithmetic_bit_for_bit():
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    R, Q = _data()
    k, nq = 200, Q.shape[0]
    eng.db_add(R)
    d2_b, id_b = eng.search(Q, k)                                    # batch plan (> 128 rows would be; 64 rows take the single-image plan) ...
    d2_big, id_big = eng.search(torch.cat([Q, Q, Q]).contiguous(), k)   # ... so also as part of a 192-row batch
    eng.set_option("knn_filter", "fp32")
    d2_f, id_f = eng.search(Q, k)
    eng.set_option("knn_filter", "auto")
    assert torch.equal(id_big[:nq], id_b) and torch.equal(d2_big[:nq], d2_b) and torch.equal(id_f, id_b) and torch.equal(d2_f, d2_b)
    n_contested, n_tie_pairs, worst64 = E.check_contested(Q, R, d2_b, id_b, k)   # (contested rows, emulated fp32, fp64 within 4e-6)
    dd, ii = d2_b.cpu().numpy(), id_b.cpu().numpy()
    assert ii[0, 0] == 123_456 and ii[0, 1] == 777_777 and dd[0, 0] == dd[0, 1]      # the planted exact tie: lower id first
    print(f"[exact ids] {nq} queries x {k}: {n_contested} contested pairs emulated, {n_tie_pairs} exact-tie neighbours among the results, "
          f"max |fp32 - fp64| {worst64:.2e}")
    eng.close()
