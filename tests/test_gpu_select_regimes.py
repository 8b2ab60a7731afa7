"""Every instantiation of the candidate-list selects at its boundary (csrc/select_dev.h, csrc/knn_select_kernels.hip): the wave
select's 4 / 16 / 32 / 64 keys per lane (lists of <= 256 / 1024 / 2048 / 4096 entries), the workgroup forms beyond it
(select_approx_kernel for batches, select_wg_kernel's 16 / 32 keys per thread for a single image) and the overflow of the lists'
capacity (8192).  One clump of near-copies of a vector, with a dozen queries next to it, sets the longest list: every case asserts
the interval its search_stats()["cand_max"] lands in -- none can pass on another body -- and compares (d2, ids) bit for bit with
the all-fp32 filter; batches also with the plain levels (level_carry = 0) and with the rigorous thresholds (knn_heuristic = 0:
`check` off).  Which rule a case runs is asserted too: k = 10 keeps the rigorous thresholds, k = 20 guesses them (two filter levels
for a batch, the checks), and a batch of more than 1024 query rows -- enough tiles for the complement form of the last level's
filter at this index size -- carries the stride-16 level's survivors (select mode Carry).  Run with `-m gpu` on an MI355X."""
import pytest
from conftest import engine_scope

pytestmark = pytest.mark.gpu

N, D, NEAR = 65536 + 7, 64, 12
STEP = 7   # the clump of size c lives in rows 0, 7, 14, ..., 7 (c - 1): every strided sample of the levels sees its share of them
# clump size -> the interval of the longest last-level list.  The lists hold the clump and nothing else: every query row lies in
# its neighbourhood (a dozen next to its centre: the whole clump is inside their band; the others a little off), the other index
# rows are far away.  The sample of the level before the last (stride 16) must hold k rows of the clump for that: 16 k <= c.
REGIMES = [(200, 0, 256), (600, 256, 1024), (1500, 1024, 2048), (3000, 2048, 4096), (6000, 4096, 8192), (9000, 8192, None)]
# k = 10: the plan keeps the rigorous thresholds (one filter level; `check` off, nothing carried).  k = 20 is the smallest k whose
# thresholds are guessed: a batch then has two filter levels and the checks; its lists cannot stay within 256 entries (the
# stride-16 sample would have to hold 19 rows of a clump of <= 256), so that interval is k = 10's alone.
# Forms: a batch (192 query rows), a single image (40), and -- guessed thresholds only -- a batch of 1040 rows, which carries.
FORMS = {"batch": 192, "single_image": 40, "batch_carry": 1040}
CASES = [(10, r, f) for r in REGIMES for f in ("batch", "single_image")] + [(20, r, f) for r in REGIMES[1:] for f in FORMS]


@pytest.fixture(scope=engine_scope)
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device (no CPU fallback exists)"
    from revisit_anything_amd.engine import SegVLADEngine

    e = SegVLADEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def base():
    """The un-planted index, the clump's rows at full length and the queries: drawn once, never written to."""
    import torch

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4242)
    R = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
    v0 = torch.nn.functional.normalize(torch.randn(1, D, device=dev, generator=g), dim=1)
    clump = torch.nn.functional.normalize(v0 + (1e-3 / D ** 0.5) * torch.randn(9000, D, device=dev, generator=g), dim=1)
    Q = v0 + (0.3 / D ** 0.5) * torch.randn(max(FORMS.values()), D, device=dev, generator=g)
    Q[:NEAR] = v0 + (1e-3 / D ** 0.5) * torch.randn(NEAR, D, device=dev, generator=g)
    return R, clump, torch.nn.functional.normalize(Q, dim=1).contiguous()


def _plant(base, c, nq):
    R0, clump, Q = base
    R = R0.clone()
    R[0:STEP * c:STEP] = clump[:c]
    return R, Q[:nq].contiguous()


def _search(eng, R, Q, k, **opts):
    """A search on a fresh index (rows redone by an earlier search must not switch the guessed thresholds off)."""
    eng.db_reset()
    eng.db_add(R)
    defaults = {"knn_filter": "auto", "level_carry": 1, "knn_heuristic": 1}
    try:
        eng.set_option("search_stats", 1)
        for name, v in opts.items():
            eng.set_option(name, v)
        d2, idx = eng.search(Q, k)
        st = eng.search_stats()
    finally:
        for name in opts:
            eng.set_option(name, defaults[name])
        eng.set_option("search_stats", 0)
    return d2, idx, st


@pytest.mark.parametrize("k,regime,form", CASES, ids=[f"k{k}-clump{r[0]}-{f}" for k, r, f in CASES])
def test_select_regime_equals_the_fp32_filter(eng, base, k, regime, form):
    import torch

    c, lo, hi = regime
    nq = FORMS[form]
    R, Q = _plant(base, c, nq)
    d2, idx, st = _search(eng, R, Q, k)
    print(f"k {k} clump {c} nq {nq}:", st)
    assert st["filter"] == "f16", st
    assert st["cand_max"] > lo and (hi is None or st["cand_max"] <= hi), st
    if k == 10:
        assert st["levels"] == 1 and st["carry_rows"] == 0, st
    elif nq > 128:
        assert st["levels"] == 2 and st["carry_rows"] == ((N + 15) // 16 if form == "batch_carry" else 0), st
    if hi is not None:
        assert st["n_fallback"] == 0, st
    else:
        # the planted queries' lists overflow their capacity.  Rigorous thresholds: the rows go to the exact matrix path (n_fallback).
        # Guessed ones: a batch redoes them with the rigorous thresholds first (n_redo; those lists overflow again), a single image
        # finishes them on the device by exact brute force (n_redo)
        assert max(st["n_fallback"], st["n_redo"]) >= NEAR, st
    d2f, idf, _ = _search(eng, R, Q, k, knn_filter="fp32")
    assert torch.equal(idx, idf) and torch.equal(d2, d2f)
    assert bool(((idx % STEP == 0) & (idx < STEP * c)).all())       # the clump is every query's neighbourhood
    if nq > 128:
        d2p, idp, stp = _search(eng, R, Q, k, level_carry=0)
        assert stp["carry_rows"] == 0 and stp["levels"] == st["levels"], stp
        assert torch.equal(idx, idp) and torch.equal(d2, d2p)
        d2r, idr, _ = _search(eng, R, Q, k, knn_heuristic=0)
        assert torch.equal(idx, idr) and torch.equal(d2, d2r)
