"""Hand-chosen shapes of segvlad_search, one per decision of its plan (csrc/search.hip: plan_search, chunk_path), with the branch
each one exists for, the data it runs on, and the two references it is held against (host code: no GPU, no library).

    plan()              a restatement of the plan's decisions from the comments and arithmetic of search.hip -- a model, kept
                        to what the table needs: the two stride loops, `matrix`, the filter kind, `guessed`, the single-image
                        plan's stride, the deeper guessed levels, the chunks, the carry, level 0's form and launch count
    CASES               the table; every case DECLARES its branch, tests/test_search_plan_cases.py holds the declarations against
                        plan(), tests/test_gpu_search_plan.py against search_stats() and the stage launch counts of the device
    make_data()         the case's index rows and query rows (NumPy, seeded: the CPU self-test and the GPU test see the same)
    check_all_queries() every query row against float64 distances (torch: the CPU or the device)

Branch fields of a case:
    filter   none (the matrix path) | f16 | bf16x3 | fp32                                search_stats()["filter"]
    levels   filter levels behind level 0 (0 on the matrix path)                         search_stats()["levels"]
    carry    the last level runs over the complement of the stride-16 sample              search_stats()["carry_rows"] > 0
    form     matrix | single (every chunk <= 128 rows) | batch                           launches: see plan()["launches"]
    flags    zero     n_fallback == 0 and n_redo == 0 (matrix path, rigorous thresholds)
             rare     guessed thresholds on benign data: n_fallback == 0; a redo is a matter of chance BY DESIGN (heur_rank: 4 sigma,
                      heur_rank_small: 2e-5 per row and level), so n_redo <= 1 + nq / 4096 -- three orders above its expectation
             nonzero  n_fallback + n_redo > 0: the margin's band cannot fit the lists (margin_overflows())
The form has no field of its own in search_stats(): it follows from nq alone (chunk_path: m > 128), and what the device can
witness of it is the number of chunks and level-0 launches, which plan()["launches"] counts (stages knn_gemm + knn_level0).

Level 0 has a fourth form, FilterLists (guessed batches over rows of d >= 4096); the smallest index that reaches it is
32769 x 4096 floats (0.5 GB), which no case of a suite that has to stay quick builds: the table reaches the other three."""
import math
from collections import namedtuple

import numpy as np

SV_RATIO, SV_CAP, SV_CHUNK = 16, 8192, 16384


# ---- the restatement ----------------------------------------------------------------------------------------------------
def heur_rank(target):
    """Smallest r >= 16 whose 1/16-sample threshold still admits `target` rows 4 sigma below its expectation 16 r."""
    r = 16
    while 16.0 * r - 64.0 * math.sqrt(r) < target:
        r += 1
    return r


def heur_rank_small(target, ratio, pfail=2e-5):
    """Smallest r >= 2 with P[Gamma(r, 1) < target / ratio] < pfail (the single-image plan's low ranks)."""
    x = target / ratio
    ex, term, acc = math.exp(-x), 1.0, 0.0
    for r in range(1, target):
        acc += term
        term *= x / r
        if r >= 2 and 1.0 - ex * acc < pfail:
            return r
    return target


def plan(n, d, nq, k, knn_filter="auto", knn_heuristic=1, level_carry=1, q_offset=0, bias_ok=True):
    """What segvlad_search decides for an index of n rows of d, nq query rows, k neighbours, a query pointer q_offset floats past
    a 16-byte boundary and the default options but the three named.  bias_ok: the batch's norms allow the biased kernel
    (1 + max||r|| / (2 min||q||) <= 5: unit rows give 1.5)."""
    p = {"matrix": True, "filter": "none", "levels": 0, "guessed": False, "small": False, "stride0": 1, "carry_rows": 0,
         "form": "matrix", "l0": [], "fuse_qn": False, "wide_prep": False}
    # rigorous plan: strides 16^L .. 16, 1; level 0's sample keeps >= 4.8 k rows (and >= 512), and never exceeds 32768 rows
    stride, levels = 1, 0
    if n > 32768:
        want = max((24 * k + 4) // 5, 512)
        while n // (stride * SV_RATIO) >= want:
            stride, levels = stride * SV_RATIO, levels + 1
        while n // stride > 32768:
            stride, levels = stride * SV_RATIO, levels + 1
    p["rig_levels"], p["rig_stride0"] = levels, stride
    if levels == 0 or n // stride < 4 * k:
        # one exact distance block of at most 2 GiB per launch
        ld = (n + 3) & ~3
        rows = min(max((2 << 30) // (ld * 4), 128), nq)
        p["launches"] = -(-nq // rows)
        return p
    p["matrix"] = False
    f16 = knn_filter in ("auto", "f16") and d % 64 == 0
    bf16 = not f16 and knn_filter != "fp32" and d % 32 == 0
    p["filter"] = "f16" if f16 else "bf16x3" if bf16 else "fp32"
    guessed = p["filter"] != "fp32" and bool(knn_heuristic) and heur_rank(k) < k
    p["guessed"] = guessed
    ratio_last = SV_RATIO
    small_stride = 16
    while -(-n // small_stride) > 4096 and small_stride <= 512:
        small_stride *= 2
    small = guessed and nq <= 128 and small_stride <= 512
    p["small"] = small
    if small:                      # one query image: ONE filter level behind a sample of 2048 .. 4096 rows
        levels, stride, ratio_last = 1, small_stride, small_stride
    elif guessed:                  # guessed thresholds need a few dozen sample rows per rank: level 0 shrinks to >= 192 rows
        while levels < 6 and n // (stride * SV_RATIO) >= 192:
            stride, levels = stride * SV_RATIO, levels + 1
    p["levels"], p["stride0"] = levels, stride
    p["form"] = "batch" if nq > 128 else "single"
    n0 = -(-n // stride)
    # query preparation: one image of <= 2^18 floats is prepared by ONE workgroup, which writes the norms too when the view is aligned
    one_wg = f16 and nq <= 128 and (nq * d) % 4 == 0 and nq * d <= (1 << 18)
    p["fuse_qn"] = one_wg and q_offset % 4 == 0
    p["wide_prep"] = f16 and nq <= 128 and not one_wg
    n_comp = n - -(-n // SV_RATIO)
    launches = 0
    for q0 in range(0, nq, SV_CHUNK):
        m = min(nq - q0, SV_CHUNK)
        batch = m > 128
        short = n0 <= 4096 and p["filter"] != "fp32"
        if not batch and short:
            l0 = "SplitReduce"
        elif guessed and f16 and batch and n0 <= 4096:
            l0 = "FilterLists" if d >= 4096 else "SampleF16"
        else:
            l0 = "ExactGemm"
        p["l0"].append(l0)
        # the sample's exact GEMM splits K over workgroups when it has <= 32 tiles of rows >= 512 long: reduction and rank are then
        # a second launch of the stage.  (The one-launch head of an aligned single image of d < 512 counts one, like level 0 itself.)
        tiles = -(-m // 128) * -(-n0 // 128)
        launches += (2 if l0 == "SplitReduce" and tiles <= 32 and d >= 512 and not one_wg else 1) + levels
        fills = -(-m // 256) * -(-n_comp // 256) >= 1024          # the persistent 256 x 256 kernel has the complement form
        if guessed and f16 and levels >= 2 and ratio_last == SV_RATIO and batch and level_carry and bias_ok and fills and d < 4096:
            p["carry_rows"] = n - n_comp
    p["launches"] = launches
    return p


def f16_c_eps(d, bias_mult=1.0):
    """|d2~ - d2| <= c_eps ||q|| ||r|| of the one-product fp16 filter with one running accumulator (d < 4096), 25 % slack included."""
    return 2.5 * (2.0 ** -10 + 2.0 ** -22 + bias_mult * 2.0 * d * 2.0 ** -24)


def margin_overflows(Q, R, k):
    """Per query row: does the fp16 filter's last list certainly outgrow SV_CAP?  The list holds every row with d2~ <= T + eps,
    eps = c_eps ||q|| max||r||, under a threshold T that is never below the k-th smallest distance (or the row is flagged for
    that); the error of a pair's d2~ is within c_eps ||q|| ||r|| / 1.25 for ITS row's norm (the bound without its slack), so
    every row with d2 <= kth + eps - c_eps ||q|| ||r|| / 1.25 is in the list."""
    Q64, R64 = Q.astype(np.float64), R.astype(np.float64)
    q2, r2 = (Q64 * Q64).sum(1), (R64 * R64).sum(1)
    D = q2[:, None] + r2[None, :] - 2.0 * (Q64 @ R64.T)
    kth = np.partition(D, k - 1, axis=1)[:, k - 1]
    c = f16_c_eps(Q.shape[1])
    eps = c * np.sqrt(q2 * r2.max())
    own = c * np.sqrt(q2[:, None] * r2[None, :]) / 1.25
    return (D <= (kth + eps)[:, None] - own).sum(1) > SV_CAP


# ---- the table ----------------------------------------------------------------------------------------------------------
# data: gauss (N(0, 1) entries, rows of every norm), unit (unit rows, queries next to index rows), unit_far (unit rows, unit
#       queries drawn on their own), shell, clump, mixed (make_data)
# q_offset: floats between a 16-byte boundary and the query view (0 or 1);  opts: the options the case sets
# fp64: the all-queries float64 check applies (the shell and mixed-norm cases rely on the emulation alone: their neighbours are
#       closer together than any float64 tolerance that allows for fp32 arithmetic);  emulate_all: every query row is emulated
# tol64: the bound of the EMULATED arithmetic against float64 (fp32_emu.check_contested), relative to max(1, (q2 + max r2) / 2)
Case = namedtuple("Case", "name n d nq k data q_offset opts filter levels carry form flags fp64 emulate_all tol64")


def _c(name, n, d, nq, k, data, filter, levels, form, flags="zero", carry=False, q_offset=0, opts=None, fp64=True, emulate_all=False,
       tol64=4e-6):
    return Case(name, n, d, nq, k, data, q_offset, dict(opts or {}), filter, levels, carry, form, flags, fp64, emulate_all, tol64)


def _m(d, n, nq, k, **kw):
    return _c(f"matrix-d{d}-n{n}-nq{nq}-k{k}" + ("-off1" if kw.get("q_offset") else ""), n, d, nq, k, "gauss", "none", 0, "matrix", **kw)


def _f(filter, d, n, nq, k, levels, flags, tag="", data="unit", **kw):
    form = "batch" if nq > 128 else "single"
    return _c(f"{filter}-d{d}-n{n}-nq{nq}-k{k}{tag}", n, d, nq, k, data, filter, levels, form, flags, **kw)


# The widest case's tol64: the emulation's own worst deviation from float64 over its eight emulated query rows, measured on the
# case's data on the CPU (tests/test_search_plan_cases.py: test_wide_case_tol64 repeats the measurement): 4.63e-7, times 2 for
# the draw of the other rows.  Its queries are drawn on their own (unit_far): next to an index row the dot product's partial sums
# run up to 1 over 2112 steps and the fp32 chain ITSELF leaves float64 by 2.6e-6 on the emulated rows and by more than the
# all-queries check's 4e-6 on others (the device equals the emulation bit for bit there) -- that tolerance is meant for the
# device's error, so the case keeps to data on which fp32's own error is well inside it.
TOL64_D2112 = 9.3e-7

MATRIX = [
    # scalar loads (d % 4 != 0); d < 32 is one partial k-tile; 33 and 65 leave a k-tail of one element
    _m(1, 128, 1, 1), _m(1, 257, 257, 257), _m(3, 127, 129, 126), _m(3, 1, 128, 1), _m(5, 257, 128, 260), _m(30, 128, 128, 128),
    _m(30, 127, 257, 130), _m(33, 129, 257, 1), _m(33, 128, 129, 128), _m(50, 1, 127, 4), _m(50, 129, 128, 128), _m(63, 128, 1, 127),
    _m(63, 127, 257, 130), _m(65, 127, 128, 127), _m(65, 128, 1, 127), _m(100, 128, 129, 131), _m(100, 257, 127, 1),
    # vector loads, guarded loop (d % 32 != 0)
    _m(4, 129, 127, 129), _m(4, 128, 128, 1), _m(36, 257, 129, 256), _m(36, 127, 1, 130),
    # fast loop on interior tiles (d % 32 == 0), guarded on the edge tiles
    _m(32, 128, 128, 128), _m(32, 257, 257, 260), _m(32, 1, 1, 1), _m(64, 128, 257, 127), _m(64, 129, 128, 1), _m(64, 127, 127, 127),
    _m(64, 257, 129, 260),
    # the query view one float past a 16-byte boundary: no vector load in the whole GEMM, the query norms on the scalar path
    _m(64, 257, 129, 20, q_offset=1), _m(36, 129, 128, 132, q_offset=1),
    # the last matrix-path size, and an index beyond it whose level-0 sample (n / 16 = 2500 rows) is shorter than 4 k
    _m(64, 32768, 16, 10), _m(64, 40000, 16, 700),
]

FILTER = [
    # f16 (d % 64 == 0): the three index sizes (32784 is a multiple of 16), nq = 1 | 128 | 129
    _f("f16", 64, 32769, 1, 10, 1, "zero"), _f("f16", 64, 32784, 128, 10, 1, "zero"), _f("f16", 64, 32785, 129, 10, 1, "zero"),
    # k = 1 | 19 rigorous, k = 20 guessed (heur_rank(20) = 19 < 20), one query image and a batch
    _f("f16", 64, 32769, 40, 1, 1, "zero"), _f("f16", 64, 32769, 40, 19, 1, "zero"), _f("f16", 64, 32769, 40, 20, 1, "rare"),
    _f("f16", 64, 32769, 192, 1, 1, "zero"), _f("f16", 64, 32769, 192, 19, 1, "zero"), _f("f16", 64, 32769, 192, 20, 1, "rare"),
    # one query image through a view one float past a 16-byte boundary: the preparation kernel leaves the norms to row_sumsq
    _f("f16", 64, 32785, 40, 20, 1, "rare", "-off1", q_offset=1),
    # one query image of more than 2^18 floats: the many-workgroup preparation (and level 0's K split: two launches)
    _f("f16", 2112, 32769, 128, 20, 1, "rare", data="unit_far", tol64=TOL64_D2112),
    # two chunks: 16384 rows and one
    _f("f16", 64, 32769, 16385, 20, 1, "rare"),
    # a batch that carries the stride-16 level's survivors (two levels need n / 256 >= 192; the complement form needs
    # ceil(nq / 256) x ceil(n_comp / 256) >= 1024 tiles), and the same case with plain levels
    _f("f16", 64, 65537, 1040, 20, 2, "rare", carry=True), _f("f16", 64, 65537, 1040, 20, 2, "rare", "-nocarry", opts={"level_carry": 0}),
    # the other side of the matrix fallback: 2500 sample rows >= 4 x 600
    _f("f16", 64, 40000, 16, 600, 1, "rare"),
    # bf16x3 (d % 32 == 0, d % 64 != 0)
    _f("bf16x3", 96, 32769, 1, 10, 1, "zero"), _f("bf16x3", 96, 32784, 128, 20, 1, "rare"), _f("bf16x3", 96, 32785, 129, 10, 1, "zero"),
    _f("bf16x3", 32, 32785, 129, 20, 1, "rare"), _f("bf16x3", 32, 32769, 1, 10, 1, "zero"),
    # fp32 (every other width): d = 50 runs the strided-sample GEMM and the filter GEMM on scalar loads
    _f("fp32", 48, 32769, 1, 10, 1, "zero"), _f("fp32", 48, 32784, 128, 10, 1, "zero"), _f("fp32", 48, 32785, 129, 10, 1, "zero"),
    _f("fp32", 50, 32785, 129, 10, 1, "zero"), _f("fp32", 50, 32769, 1, 20, 1, "zero"), _f("fp32", 50, 32784, 128, 20, 1, "zero"),
]

STRESS = [
    # 3 k rows on a shell around every query (equal distances to 1e-6 relative: below the fp16 product's error), two of them duplicates
    _f("f16", 64, 33001, 16, 20, 1, "rare", "-shell", data="shell", fp64=False, emulate_all=True),
    # a clump of 3 k near-copies of the query whose fp16 products are all off in ONE direction, by 0.78 of the margin (rigorous thresholds:
    # level 0's exact k-th distance is ~0, so a margin a quarter of its size loses the whole neighbourhood)
    _f("f16", 64, 33001, 16, 10, 1, "zero", "-clump", data="clump", fp64=False, emulate_all=True),
    # unit rows, six rows of norm 1e3 (they set the index's fp16 scale and the margin), queries of norm 1 and 1e-2: every list overflows
    _f("f16", 64, 33001, 16, 20, 1, "nonzero", "-mixed", data="mixed", fp64=False, emulate_all=True),
    _f("f16", 64, 33001, 16, 10, 1, "nonzero", "-mixed", data="mixed", fp64=False, emulate_all=True),
]

CASES = MATRIX + FILTER + STRESS
assert len({c.name for c in CASES}) == len(CASES)


def case_plan(c):
    return plan(c.n, c.d, c.nq, c.k, q_offset=c.q_offset, **{k: v for k, v in c.opts.items() if k in ("level_carry", "knn_heuristic", "knn_filter")})


def declared(c):
    return {"filter": c.filter, "levels": c.levels, "carry": c.carry, "form": c.form}


def planned(p):
    return {"filter": p["filter"], "levels": p["levels"], "carry": p["carry_rows"] > 0, "form": p["form"]}


# ---- data ---------------------------------------------------------------------------------------------------------------
SHELL_STEP = 7   # the shell of query j lives in rows 5 + 7 (3 k j + i), i < 3 k: every strided sample sees its share


def clump_ids(k):
    """Rows of the clump (3 k of them): half in the stride-16 sample (more than k: level 0's exact k-th distance is the clump's), half not."""
    m = 3 * k
    return np.concatenate([16 * (3 + 5 * np.arange(m // 2)), 7 + 16 * (2 + 5 * np.arange(m - m // 2))])


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def make_data(c):
    """(R [n, d], Q [nq, d]) fp32, C-contiguous, from a generator seeded by the case's position in the table."""
    rng = np.random.Generator(np.random.PCG64(9000 + [x.name for x in CASES].index(c.name)))
    n, d, nq, k = c.n, c.d, c.nq, c.k
    R = rng.standard_normal((n, d), dtype=np.float32)
    if c.data == "gauss":
        return R, rng.standard_normal((nq, d), dtype=np.float32)
    R = _unit(R)
    if c.data == "shell":
        Q = _unit(rng.standard_normal((nq, d)))
        m = 3 * k
        for j in range(nq):
            q = Q[j].astype(np.float64)
            u = rng.standard_normal((m, d))
            u -= (u @ q)[:, None] * q / (q @ q)
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            ids = 5 + SHELL_STEP * (m * j + np.arange(m))
            R[ids] = (0.8 * q / np.linalg.norm(q) + 0.6 * u).astype(np.float32)
            R[ids[m // 2]] = R[ids[3]]                       # two exact duplicates: only the id orders them
        return R, Q
    if c.data == "clump":
        # every entry +-v with v a hair below the midpoint of two fp16 values (at any power-of-two scale): both operands round DOWN by
        # 0.97 x 2^-11 relative, in every term of the product, so d2~ exceeds d2 by ~1.9e-3 ||q|| ||r|| -- 0.78 of the margin
        w = rng.choice([-1.0, 1.0], d) * (0.125 * (1.0 + 0.97 * 2.0 ** -11))
        m = 3 * k
        R[clump_ids(k)] = (w[None, :] * (1.0 + 1.4e-5 * rng.uniform(-1.0, 1.0, (m, d)))).astype(np.float32)
        return R, (w[None, :] * (1.0 + 1.4e-5 * rng.uniform(-1.0, 1.0, (nq, d)))).astype(np.float32)
    if c.data == "unit_far":
        return R, _unit(rng.standard_normal((nq, d), dtype=np.float32))
    Q = _unit(R[rng.integers(0, n, nq)] + (0.3 / math.sqrt(d)) * rng.standard_normal((nq, d), dtype=np.float32))
    if c.data == "mixed":
        R[11:n:n // 6][:6] *= np.float32(1e3)
        Q[nq // 2:] *= np.float32(1e-2)
    return R, Q


def emulated_rows(c):
    """The query rows held against the emulation: first, last, both sides of the 128-row and 16384-row chunk boundaries, and
    evenly spaced others up to min(nq, 8); every row of a stress case."""
    if c.emulate_all:
        return list(range(c.nq))
    rows = {r for r in (0, c.nq - 1, 127, 128, 16383, 16384) if r < c.nq}
    want = min(c.nq, 8)
    for j in range(want):
        if len(rows) >= want:
            break
        rows.add((j * c.nq) // want)
    return sorted(rows)


# ---- every query row against float64 --------------------------------------------------------------------------------------
def check_all_queries(Q, R, d2, idx, k, tol=4e-6, block_bytes=64 << 20):
    """Q [nq, d], R [n, d] fp32 torch tensors, (d2 [nq, k] fp32, idx [nq, k] int64) a search result on the same device.
    With d64 the float64 distances, kth their min(k, n)-th smallest per query and t = tol x max(1, (||q||^2 + max ||r||^2) / 2):
    every row with d64 < kth - t is listed, every listed row has d64 <= kth + t, |d2 - d64| <= t, the list ascends with equal
    distances in id order, slots beyond n hold (+inf, -1).  Rows within t of kth are undecided when more of them exist than
    slots are left for them.  Returns (undecided pairs, nq x min(k, n))."""
    import torch

    nq, n = Q.shape[0], R.shape[0]
    kk = min(k, n)
    R64 = R.double()
    r2 = (R64 * R64).sum(1)
    undecided = 0
    step = max(1, block_bytes // (8 * n))
    for q0 in range(0, nq, step):
        Q64 = Q[q0:q0 + step].double()
        dd, ii = d2[q0:q0 + step], idx[q0:q0 + step]
        q2 = (Q64 * Q64).sum(1)
        D = q2[:, None] + r2[None, :] - 2.0 * (Q64 @ R64.T)
        t = tol * torch.clamp((q2 + r2.max()) / 2.0, min=1.0)
        kth = torch.kthvalue(D, kk, dim=1).values
        assert bool((ii[:, kk:] == -1).all()) and bool(torch.isposinf(dd[:, kk:]).all()), "slots beyond the index"
        ii, dd = ii[:, :kk], dd[:, :kk]
        assert bool(((ii >= 0) & (ii < n)).all())
        listed = torch.zeros(D.shape, dtype=torch.bool, device=D.device)
        listed.scatter_(1, ii, True)
        assert bool((listed.sum(1) == kk).all()), "a row is listed twice"
        below = D < (kth - t)[:, None]
        missing = below & ~listed
        assert not bool(missing.any()), ("a neighbour is missing", q0 + int(torch.nonzero(missing.any(1))[0]))
        dl = torch.gather(D, 1, ii)
        assert bool((dl <= (kth + t)[:, None]).all()), "a listed row is too far"
        assert bool(((dd.double() - dl).abs() <= t[:, None]).all()), float(((dd.double() - dl).abs() / t[:, None]).max())
        step_ok = (dd[:, 1:] > dd[:, :-1]) | ((dd[:, 1:] == dd[:, :-1]) & (ii[:, 1:] > ii[:, :-1]))
        assert bool(step_ok.all()), "order"
        band = ((D - kth[:, None]).abs() <= t[:, None]).sum(1)
        undecided += int(torch.where(band > kk - below.sum(1), band, torch.zeros_like(band)).sum())
    return undecided, nq * kk


def fp64_topk(Q, R, k):
    """The float64 distances' own top-k in (distance, id) order, as a search result (d2 fp32, idx int64; padded beyond n)."""
    import torch

    n = R.shape[0]
    kk = min(k, n)
    Q64, R64 = Q.double(), R.double()
    D = (Q64 * Q64).sum(1)[:, None] + (R64 * R64).sum(1)[None, :] - 2.0 * (Q64 @ R64.T)
    dd, ii = torch.sort(D, dim=1, stable=True)
    d2 = torch.full((Q.shape[0], k), float("inf"), dtype=torch.float32)
    idx = torch.full((Q.shape[0], k), -1, dtype=torch.int64)
    d2[:, :kk], idx[:, :kk] = dd[:, :kk].float(), ii[:, :kk]
    # float64 neighbours that round to the same fp32 value: a result lists them in id order
    d2n, idn = d2.numpy(), idx.numpy()
    for r in np.nonzero((np.diff(d2n[:, :kk], axis=1) == 0).any(1))[0]:
        o = np.lexsort((idn[r, :kk], d2n[r, :kk]))
        idn[r, :kk] = idn[r, :kk][o]
    return d2, idx
