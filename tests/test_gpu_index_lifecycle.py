"""A LIVE index through its lifetime: one context serving many db_add / db_reset / search calls, as a place-recognition map that
grows image by image.  Between calls the context keeps derived state (csrc/ctx.h): the fp16 image of the rows and its scale, the
max row norm of the filter's margin, the bf16 hi/lo planes, db_heur_off, the shortlist's image -> row map and the single-image
pass's device words (tickets, totals, the head's barrier counter).  The central check of every step: the result does not depend on
history -- the live context gives the same (d2, idx) bits and the same plan statistics as a FRESH context holding the same rows in
one db_add -- and on a subset of query rows it equals the emulated fp32 reference bit for bit, ties included, with the fp64 oracle
beside it (tests/fp32_emu.py: check_contested).  The data is benign (noise-perturbed copies of rows): no pass redoes a row.

Every test owns its contexts (no module fixture: the history IS the subject)."""
import numpy as np
import pytest
import torch

import fp32_emu as E

pytestmark = pytest.mark.gpu

K = 50
SINGLE = (1, 50, 128)     # one query image per pass (<= 128 rows: the single-image plan)
BATCH = 320               # a batch (the multi-level plan)


def _engine(**opts):
    from revisit_anything_amd.engine import SegVLADEngine

    eng = SegVLADEngine(0)
    for key, v in opts.items():
        eng.set_option(key, v)
    return eng


def _unit_rows(n, d, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=g), dim=1)


def _queries(R, m, seed, noise=0.05, lo=0):
    """m noise-perturbed copies of rows lo .. len(R) - 1 (as _problem of test_gpu_small_tail.py), scaled to their source's norm."""
    g = torch.Generator(device=R.device)
    g.manual_seed(seed)
    src = torch.randint(lo, R.shape[0], (m,), device=R.device, generator=g)
    base = R[src]
    nrm = base.norm(dim=1, keepdim=True)
    return (nrm * torch.nn.functional.normalize(base / nrm + noise * torch.randn(m, R.shape[1], device=R.device, generator=g), dim=1)).contiguous()


def _step_queries(R, seed, fresh_rows=0):
    """The searches of one step: single-image batches of every size in SINGLE and one BATCH; half of the rows near the rows the
    last db_add brought (fresh_rows of them at the end of R), so the new rows are neighbours."""
    out = []
    for j, m in enumerate(SINGLE + (BATCH,)):
        lo = R.shape[0] - fresh_rows if fresh_rows and j % 2 else 0
        out.append(_queries(R, m, seed + j, lo=lo))
    return out


def _run(eng, Qs, k=K):
    res = []
    for Q in Qs:
        d2, idx = eng.search(Q, k)
        res.append((d2, idx, eng.search_stats()))
    return res


def _emulated_subset(m):
    return sorted({0, m // 2, m - 1})


def _check_against_fresh(R, Qs, got, k=K, opts=None, emulate=True, single_levels=True):
    """got: the live context's [(d2, idx, stats)] for Qs over the rows R.  A fresh context holding R (one db_add) must give the
    same bits and plan; a subset of rows is held to the emulated fp32 reference."""
    fresh = _engine(**(opts or {}))
    fresh.db_add(R)
    ref = _run(fresh, Qs, k)
    fresh.close()
    for Q, (d2, idx, st), (rd2, ridx, rst) in zip(Qs, got, ref):
        m = Q.shape[0]
        assert torch.equal(idx, ridx), (R.shape, m, int((idx != ridx).sum()))
        assert torch.equal(d2.view(torch.int32), rd2.view(torch.int32)), (R.shape, m)
        assert (st["levels"], st["filter"]) == (rst["levels"], rst["filter"]), (R.shape, m, st, rst)
        assert st["n_redo"] == 0 and st["n_fallback"] == 0, (R.shape, m, st)
        assert rst["n_redo"] == 0 and rst["n_fallback"] == 0, (R.shape, m, rst)
        if single_levels and R.shape[0] > 32768 and st["filter"] != "fp32":
            assert (st["levels"] == 1) == (m <= 128), (R.shape, m, st)
        if emulate:
            E.check_contested(Q, R, d2, idx, k, queries=_emulated_subset(m))


# Growth across the single-image plan's stride and grid changes.  small_stride = the smallest power of two >= 16 that leaves
# n0 = ceil(n / stride) <= 4096 sample rows, and small_head_kernel's grid NW = ceil(n0 / 32) (csrc/search.hip, small_pass_kernels.hip):
#        80 000 rows: stride  32, n0 2500, NW  79
#       100 000 rows: stride  32, n0 3125, NW  98
#       140 000 rows: stride  64, n0 2188, NW  69
#     1 000 000 rows: stride 256, n0 3907, NW 123
#        70 000 rows: stride  32, n0 2188, NW  69      (after db_reset)
# The head's grid barrier once derived its generation from a 64-bit arrival counter, (ticket / NW + 1) * NW: after 79 arrivals of the
# first step, the 98 workgroups of the second drew tickets 79 .. 176 and most of them waited for 196 arrivals that never came (their
# rows: threshold -inf -> the tail's brute force; n_redo > 0, later the rigorous plan).  d = 96 (d % 64 != 0) is the older path
# without the fused head (query_f16_small_kernel + the exact sample level), taken through the same growth.
@pytest.mark.parametrize("d", [1024, 96])
def test_growth_across_grid_and_stride_changes(d):
    dev = torch.device("cuda:0")
    sizes = (80_000, 100_000, 140_000, 1_000_000)
    Rall = _unit_rows(sizes[-1], d, 7000 + d, dev)
    live = _engine()
    prev = 0
    for s, n in enumerate(sizes):
        live.db_add(Rall[prev:n])
        R = Rall[:n]
        Qs = _step_queries(R, 100 * s + d, fresh_rows=n - prev)
        _check_against_fresh(R, Qs, _run(live, Qs))
        prev = n
    del Rall
    live.db_reset()
    R = _unit_rows(70_000, d, 7100 + d, dev)
    live.db_add(R)
    Qs = _step_queries(R, 900 + d)
    _check_against_fresh(R, Qs, _run(live, Qs))
    live.close()


def test_small_index_grows_into_the_filter_plan():
    """<= 32 768 rows take the plain matrix path, with no fp16 image of the rows: the image is built lazily by the first filter
    search AFTER the index outgrew it, on a context that has searched before."""
    dev = torch.device("cuda:0")
    d = 256
    Rall = _unit_rows(140_000, d, 31, dev)
    live = _engine()
    prev = 0
    for s, n in enumerate((20_000, 30_000, 60_000, 140_000)):
        live.db_add(Rall[prev:n])
        R = Rall[:n]
        Qs = _step_queries(R, 300 + s, fresh_rows=n - prev)
        got = _run(live, Qs)
        if n <= 32768:
            assert all(st["filter"] == "none" for _, _, st in got), [st for _, _, st in got]
        _check_against_fresh(R, Qs, got)
        prev = n
    live.close()


def _history_rows(case, n, d, dev):
    """Rows added to a unit-norm index after a search.  larger: max |x| x 4 (the fp16 image is rescaled); smaller: x 1e-3 (no
    rescale: the new rows are quantised under the old scale -- few of them: every one sits at d2 ~ 1 from a unit query, closer
    than any unit row but its source, and they must not flood the candidate lists); wider_norm: norm 3 but max |x| = 3 / sqrt(d),
    below the unit rows' max (no rescale, but a larger max row norm for the filter's margin)."""
    g = torch.Generator(device=dev)
    g.manual_seed({"larger": 44, "smaller": 45, "wider_norm": 46}[case])
    if case == "larger":
        return 4.0 * _unit_rows(n, d, 41, dev)
    if case == "smaller":
        return 1e-3 * _unit_rows(n // 20, d, 42, dev)
    signs = torch.randint(0, 2, (n, d), device=dev, generator=g).float() * 2.0 - 1.0
    return (3.0 / d ** 0.5) * signs


@pytest.mark.parametrize("case", ["larger", "smaller", "wider_norm"])
def test_magnitude_history_of_the_fp16_image(case):
    dev = torch.device("cuda:0")
    d = 256
    R0 = _unit_rows(60_000, d, 40, dev)
    live = _engine()
    live.db_add(R0)
    Qs = _step_queries(R0, 500)
    _check_against_fresh(R0, Qs, _run(live, Qs))
    Rh = _history_rows(case, 20_000, d, dev)
    if case == "wider_norm":
        assert float(Rh.abs().max()) < float(R0.abs().max()) and float(Rh.norm(dim=1).min()) > 2.9
    live.db_add(Rh)
    R1 = torch.cat([R0, Rh])
    # the new rows are the true neighbours of half the queries (queries at their own scale: norm 4, 1e-3, 3)
    Qs = _step_queries(R1, 510, fresh_rows=Rh.shape[0])
    got = _run(live, Qs)
    _check_against_fresh(R1, Qs, got)
    near_new = got[1][1].cpu().numpy()[:, 0]                 # (m = 50: its rows are copies of new rows)
    assert (near_new >= R0.shape[0]).mean() > 0.9, near_new
    R2 = _unit_rows(40_000, d, 43, dev)
    live.db_add(R2)
    R3 = torch.cat([R1, R2])
    Qs = _step_queries(R3, 520, fresh_rows=R2.shape[0])
    _check_against_fresh(R3, Qs, _run(live, Qs))
    live.close()


@pytest.mark.parametrize("filt", ["fp32", "bf16x3"])
def test_filter_arithmetic_across_adds(filt):
    """The non-fp16 filters across the same kind of history: the bf16 hi/lo planes are extended incrementally."""
    dev = torch.device("cuda:0")
    d = 256
    live = _engine(knn_filter=filt)
    parts = [_unit_rows(60_000, d, 60, dev), _history_rows("larger", 20_000, d, dev), _unit_rows(40_000, d, 61, dev)]
    for s in range(len(parts)):
        live.db_add(parts[s])
        R = torch.cat(parts[:s + 1])
        Qs = _step_queries(R, 600 + 10 * s, fresh_rows=parts[s].shape[0])
        got = _run(live, Qs)
        assert all(st["filter"] == filt for _, _, st in got), [st for _, _, st in got]
        _check_against_fresh(R, Qs, got, opts={"knn_filter": filt})
    live.close()


def test_heuristic_switch_off_ends_with_the_index():
    """db_heur_off: forced by a database whose passes keep being redone (debug_small_tail = 1), cleared by db_add -- the next pass
    is back on the single-level plan with nothing redone."""
    dev = torch.device("cuda:0")
    d = 256
    R0 = _unit_rows(80_000, d, 70, dev)
    live = _engine()
    live.db_add(R0)
    Q = _queries(R0, 40, 71)
    live.set_option("debug_small_tail", 1)
    seen = []
    for _ in range(6):
        live.search(Q, K)
        seen.append(live.search_stats()["n_redo"])
    assert seen[0] == 40 and seen[-1] == 0, seen            # switched to the rigorous plan
    live.set_option("debug_small_tail", 0)
    R1 = _unit_rows(20_000, d, 72, dev)
    live.db_add(R1)
    R = torch.cat([R0, R1])
    Qs = _step_queries(R, 700, fresh_rows=R1.shape[0])
    got = _run(live, Qs)
    assert got[1][2]["levels"] == 1 and got[1][2]["n_redo"] == 0, got[1][2]
    _check_against_fresh(R, Qs, got)
    live.close()


@pytest.mark.parametrize("on_side_stream", [False, True])
def test_interleaved_searches_across_an_add(on_side_stream):
    """Single-image and batch searches alternating across a db_add that changes the head's grid (80 000 -> 100 000 rows: NW 79 -> 98),
    enqueued back to back with no synchronisation and no statistics fetch between the searches on either side of the add (db_add
    itself waits for its stream before it returns: the rows may be freed after it), so the host's arrival count crosses the grid
    change with passes still in flight in front of the add; once on the default stream, once on a side stream (synchronised at the
    switch)."""
    dev = torch.device("cuda:0")
    d = 1024
    Rall = _unit_rows(100_000, d, 80, dev)
    R0, R1 = Rall[:80_000], Rall[80_000:]
    Qa = [_queries(R0, m, 81 + j) for j, m in enumerate((50, BATCH, 1, 50))]
    Qb = [_queries(Rall, m, 91 + j, lo=80_000 * (j % 2)) for j, m in enumerate((50, BATCH, 50, 1))]
    live = _engine()
    stream = torch.cuda.Stream(dev) if on_side_stream else torch.cuda.current_stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        live.db_add(R0)
        out_a = [live.search(Q, K) for Q in Qa]
        live.db_add(R1)
        out_b = [live.search(Q, K) for Q in Qb]
        out_c = [live.search(Q, K) for Q in Qb]     # and again: the pass after the first one on the new grid
    stream.synchronize()
    torch.cuda.synchronize()
    st_last = live.search_stats()
    assert st_last["n_redo"] == 0 and st_last["n_fallback"] == 0 and st_last["levels"] == 1, st_last
    live.close()
    for rows, Qs, outs in ((R0, Qa, [out_a]), (Rall, Qb, [out_b, out_c])):
        fresh = _engine()
        fresh.db_add(rows)
        for Q, o in zip(Qs, zip(*outs)):
            rd2, ridx = fresh.search(Q, K)
            for d2, idx in o:
                assert torch.equal(idx, ridx) and torch.equal(d2.view(torch.int32), rd2.view(torch.int32)), (rows.shape, Q.shape)
        fresh.close()
    E.check_contested(Qb[0], Rall, out_b[0][0], out_b[0][1], K, queries=_emulated_subset(50))


def test_shortlist_of_every_image_equals_search_after_each_add():
    """search_shortlist with every image on every shortlist equals search bit for bit (its documented contract) -- after each
    db_add, which invalidates the image -> row map the shortlist search rebuilds lazily."""
    dev = torch.device("cuda:0")
    d, per = 256, 50
    Rall = _unit_rows(100_000, d, 90, dev)
    img_all = (torch.arange(100_000, device=dev, dtype=torch.int32) // per)
    live = _engine()
    prev = 0
    for s, n in enumerate((20_000, 60_000, 100_000)):
        live.db_add(Rall[prev:n], img_all[prev:n])
        R = Rall[:n]
        n_img = n // per
        assert live.n_img_ref == n_img
        for m_img, seed in ((1, 800 + s), (7, 810 + s)):
            Q = _queries(R, m_img * per, seed, lo=prev if s else 0)
            qoff = np.arange(0, m_img * per + 1, per, dtype=np.int32)
            shortlist = np.tile(np.arange(n_img, dtype=np.int32), (m_img, 1))
            sd2, sidx = live.search_shortlist(Q, qoff, shortlist, K)
            d2, idx = live.search(Q, K)
            assert torch.equal(sidx, idx) and torch.equal(sd2.view(torch.int32), d2.view(torch.int32)), (n, m_img)
            if m_img == 1:
                _check_against_fresh(R, [Q], [(d2, idx, live.search_stats())])
        prev = n
    live.close()

