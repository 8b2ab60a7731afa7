"""Every kernel and every selectable schedule of the fp16 candidate filter returns the SAME bits (kernel family, deep-row geometry,
operand DMA, tile walk are options of the context -- `csrc/segvlad_dev.h` -- and only ever change the schedule): the result of
each is compared with the all-fp32 filter's, bit for bit, on shapes that reach the persistent batch kernel (>= 1024 tiles), its
serpentine walk with a short k-loop, coherent databases that overflow a wave's hit list (the in-place flush), the deep-row
(blocked accumulation) kernels, and -- queries far shorter than the database rows -- the three kernels without the bias.
Every listed variant must run; the values of variants that left the library are refused."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine():
    from revisit_anything_amd.engine import SegVLADEngine

    return SegVLADEngine(0)


def _unit(x):
    return torch.nn.functional.normalize(x, dim=1)


def _check_variants(R, Q, k, variants, defaults):
    eng = _engine()
    eng.db_add(R)
    eng.set_option("knn_filter", "fp32")
    ref = eng.search(Q, k)
    assert eng.search_stats()["filter"] == "fp32"
    eng.set_option("knn_filter", "auto")
    ran = 0
    for v in variants:
        for key, val in {**defaults, **v}.items():
            eng.set_option(key, val)
        d2, idx = eng.search(Q, k)
        st = eng.search_stats()
        assert st["filter"] == "f16" and st["levels"] >= 1, (v, st)
        assert torch.equal(idx, ref[1]) and torch.equal(d2, ref[0]), f"variant {v} differs from the fp32 filter"
        ran += 1
    eng.close()
    assert ran == len(variants)


BATCH_DEFAULTS = {"f16_cfg": -1, "f16_walk": -1, "f16_gm": -1, "f16_buf": -1, "f16_deep_cfg": -1, "level_carry": 1}
BATCH_VARIANTS = [{}, {"f16_walk": 0}, {"f16_walk": 1}, {"f16_walk": 2}, {"f16_walk": 3, "f16_gm": 4}, {"f16_walk": 7}, {"f16_walk": 4}, {"f16_walk": 5},
                  {"f16_walk": 6}, {"f16_buf": 0}, {"f16_cfg": 250}, {"f16_cfg": 300}, {"f16_cfg": 62}, {"f16_cfg": 63},
                  # the deep-row kernels at a depth of 256: flushed blocks over every row (no carry), the register-blocked complement forms
                  {"f16_cfg": 300, "level_carry": 0}, {"f16_cfg": 300, "f16_deep_cfg": 4}, {"f16_cfg": 300, "f16_deep_cfg": 4, "f16_buf": 0}]


def test_batch_filter_variants_are_bit_identical_to_the_fp32_filter():
    g = torch.Generator(device="cuda:0")
    g.manual_seed(11)
    n, d, nq = 300_000, 256, 3000          # 12 x 1172 tiles of 256 x 256: the persistent kernel; 4 k-tiles: a short serpentine
    R = _unit(torch.randn(n, d, device="cuda:0", generator=g))
    Q = _unit(R[(torch.arange(nq, device="cuda:0") * 97) % n] + 0.05 * torch.randn(nq, d, device="cuda:0", generator=g))
    _check_variants(R, Q, 100, BATCH_VARIANTS, BATCH_DEFAULTS)


def test_batch_filter_variants_on_a_coherent_database():
    """Every query's neighbourhood sits in ONE 256-row tile (300 near-copies of each of 40 anchors, contiguous): thousands of
    hits in single 64 x 128 wave blocks -- the wave-private epilogue flushes its list in place, the older one walks its
    accumulators -- and refine bands beyond the first-tier list."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(12)
    d, anchors, copies = 128, 40, 300
    A = _unit(torch.randn(anchors, d, device="cuda:0", generator=g))
    clump = _unit(A.repeat_interleave(copies, dim=0) + 0.02 * torch.randn(anchors * copies, d, device="cuda:0", generator=g))
    fill = _unit(torch.randn(290_000, d, device="cuda:0", generator=g))
    R = torch.cat([fill[:100_000], clump, fill[100_000:]])
    Q = _unit(A.repeat_interleave(50, dim=0) + 0.02 * torch.randn(anchors * 50, d, device="cuda:0", generator=g))   # 2000 queries
    _check_variants(R, Q, 200, [{}, {"f16_walk": 0}, {"f16_cfg": 250}, {"f16_cfg": 300}], BATCH_DEFAULTS)


def test_deep_row_filter_variants_are_bit_identical_to_the_fp32_filter():
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    n, d, nq = 40_000, 4096, 1500           # d >= 4096: blocked accumulation (4 k-blocks of 1024)
    R = _unit(torch.randn(n, d, device="cuda:0", generator=g))
    Q = _unit(R[(torch.arange(nq, device="cuda:0") * 13) % n] + 0.05 * torch.randn(nq, d, device="cuda:0", generator=g))
    _check_variants(R, Q, 50, [{"f16_deep_cfg": c} for c in (-1, 4, 5)] + [{"f16_buf": 0}, {"f16_deep_cfg": 4, "f16_buf": 0}, {"f16_cfg": 300}],
                    {"f16_cfg": -1, "f16_deep_cfg": -1, "f16_buf": -1})


def _unbiased(n, d, nq, k, seed):
    """Unit database rows, query rows of norm 0.05: bias_mult = 1 + max||r|| / (2 min||q||) = 11 > 5, so the search keeps the
    accumulators unbiased (csrc/ctx.h: sv_f16_c_eps) and the three kernels without the bias run."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    R = _unit(torch.randn(n, d, device="cuda:0", generator=g))
    Q = 0.05 * _unit(R[(torch.arange(nq, device="cuda:0") * 61) % n] + 0.05 * torch.randn(nq, d, device="cuda:0", generator=g))
    _check_variants(R, Q, k, [{}], {"f16_cfg": -1, "f16_deep_cfg": -1})


def test_unbiased_batch_kernels_are_bit_identical_to_the_fp32_filter():
    # 4 x 258 tiles of 256 x 256 >= 1024: the full level takes the persistent kernel, the stride-16 level (4 x 17 tiles) the plain one
    # (k = 50: guessed thresholds, hence the three-level plan; at k < 17 the search runs the full level alone)
    _unbiased(66_000, 64, 1024, 50, 14)


def test_unbiased_deep_row_kernel_is_bit_identical_to_the_fp32_filter():
    # d >= 4096 without the bias: 4 waves of 64 x 64 on 128 x 128 tiles, blocked accumulation (databases of <= 32 768 rows never
    # reach a filter, hence 34 000)
    _unbiased(34_000, 4096, 256, 50, 15)


def test_removed_variants_are_refused():
    from revisit_anything_amd._lib import SEGVLAD_ERR_ARG, SegVLADError

    eng = _engine()
    for key, val in (("f16_deep_cfg", 2), ("f16_cfg", 55), ("f16_buf", 1)):
        with pytest.raises(SegVLADError) as e:
            eng.set_option(key, val)
        assert e.value.code == SEGVLAD_ERR_ARG and "development" in str(e.value), (key, val, e.value)
    for key in ("f16_epi", "f16_mf", "f16_pp", "f16_small_mf", "f16_dsplit"):   # keys that left with their variants: unknown
        with pytest.raises(SegVLADError) as e:
            eng.set_option(key, -1)
        assert e.value.code == SEGVLAD_ERR_ARG, (key, e.value)
    eng.close()
