"""The shortlist search's shape table (tests/shortlist_cases.py) against itself, on the CPU: the model's constants are the ones
csrc/shortlist_kernels.hip holds, every branch the table was written for is reached by the case NAMED here (its MT, S, final sort,
map branch, scan stride, number of cuts, tie at a cut -- the target, not just "somewhere"), the brute force equals a float64
ranking on a toy case, the replay of the kernel's candidate bookkeeping ends in the brute force's lists for every row of every
case, and every case stays under the cost cap.  One line per case is printed.  The device's side is
tests/test_gpu_shortlist_cases.py."""
import os
import re

import numpy as np
import pytest

import fp32_emu as E
import shortlist_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "revisit-anything_amd", "csrc", "shortlist_kernels.hip")).read()
C = T.BY_NAME


def _one(pattern):
    m = re.findall(pattern, SRC)
    assert len(m) == 1, (pattern, m)
    return m[0]


def test_constants_are_the_sources():
    assert int(_one(r"constexpr int SL_GMAX = (\d+);")) == T.SL_GMAX
    assert int(_one(r"constexpr int SL_SORT_CAP = (\d+);")) == T.SL_SORT_CAP
    assert int(_one(r"constexpr int SL_SLICES_MAX = (\d+);")) == T.SL_SLICES_MAX
    assert int(_one(r"constexpr int SL_SCAN_T = (\d+);")) == T.SL_SCAN_T
    assert tuple(int(x) for x in _one(r"const int cap = k <= (\d+) \? (\d+) : (\d+);")) == (T.SL_CAP_K, T.SL_CAP_SMALL, T.SL_CAP_LARGE)
    # S = max(1, min(SL_SLICES_MAX, ceil(1536 / ng))), lowered while S k > 8192 or the buffers exceed 512 MB
    assert int(_one(r"int S = std::max\(1, std::min\(SL_SLICES_MAX, \((\d+) \+ ng - 1\) / std::max\(ng, 1\)\)\);")) == T.SL_WORKGROUPS
    keys, mb, sh = _one(r"while \(S > 1 && \(S \* k > (\d+) \|\| \(size_t\)n_lists \* S \* cap \* 8 > \(\(size_t\)(\d+) << (\d+)\)\)\) --S;")
    assert int(keys) == T.SL_FINAL_KEYS and int(mb) << int(sh) == T.SL_CAND_BYTES
    # the tile is 128 union rows, a buffer is cut when it could not take another one, MT follows the longest group
    assert int(_one(r"if \(\(int\)s_cnt\[r\] > cap - (\d+)\) compact\(r, k\);")) == T.TILE
    assert int(_one(r"const int ntile = \(U \+ (\d+)\) >> 7;")) == T.TILE - 1
    assert _one(r"const int mt = gmax > (\d+) \? (\d) : (\d);") == ("32", "2", "1")
    assert int(_one(r"int np2m = (\d+);")) == 64
    assert _one(r"if \(S > 1 \|\| total > 1\) sv_bitonic") is not None
    assert _one(r"if \(c <= 1\) return;") and _one(r"if \(c <= SL_SORT_CAP\) \{")
    assert int(_one(r"if \(flds > (\d+) \* 1024\)")) == 48


# ---- what every case reaches ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    """Per case: the replay of every query row (simulate) next to the brute force's lists."""
    out = {}
    for c in T.CASES:
        x = T.make_data(c.data)
        rows = []
        for b, (u, D) in enumerate(T.unions(c.data)):
            rows += [T.simulate(c, D[r], u) for r in range(D.shape[0])]
        out[c.name] = rows
        assert len(rows) == x["Q"].shape[0]
    return out


def _cuts(rows):
    return np.array([r["cuts"] for r in rows])


def test_one_line_per_case(replays):
    for c in T.CASES:
        p, rows = T.plan(c), replays[c.name]
        cuts = _cuts(rows)
        branches = {str(b): int((p["sort"] == b).sum()) for b in ("none", "lds", "scan")}
        print(f"{c.name}: MT {p['MT']} S {p['S']} cap {p['cap']} np2 {p['np2']} np2m {p['np2m']} map {branches} per {p['per']} "
              f"U {min(p['U'])}..{max(p['U'])} mid-loop cuts {cuts.min()}..{cuts.max()} end cuts {sum(any(r['end_cut']) for r in rows)} "
              f"rows tie at a cut {sum(r['tie_cut'] for r in rows)} rows cost {p['cost']:.3g}")
        assert p["cost"] <= T.COST_CAP, (c.name, p["cost"])
        assert len(T.make_data(c.data)["R"]) <= 32768
        assert 1 <= c.k <= 1024 and 1 <= T.make_data(c.data)["sl"].shape[1] <= 4096


def test_named_targets_of_the_gemm(replays):
    # MT = 1: every group of the call <= 32 rows, groups of 1, 31 and 32 rows; unions that end at 128, 129 and 257
    p = T.plan(C["mt1-rows-1-31-32"])
    assert p["MT"] == 1 and {g[1] for g in p["groups"]} >= {1, 31, 32} and set(p["U"]) == {128, 129, 257}
    assert p["tiles"][0][:3] == [1, 1, 1] and p["S"] == 8
    # MT = 2 with a one-row group beside it, and the near-equal split 65 -> 32 + 33
    p = T.plan(C["mt2-rows-33-64-65-1"])
    assert p["MT"] == 2 and sorted(g[1] for g in p["groups"]) == [1, 32, 33, 33, 64]
    # widths: one k-tile everywhere else, three and five here; the view off its boundary
    assert T.make_data("d96")["d"] == 96 and T.make_data("d160")["d"] == 160 and C["d160-view-off-16-bytes"].q_offset == 1
    assert all(T.make_data(c.data)["d"] == 32 for c in T.CASES if c.data not in ("d96", "d160"))
    assert [c.name for c in T.CASES if c.q_offset] == ["d160-view-off-16-bytes"]


def test_named_targets_of_the_slice_rule(replays):
    # S = 1: 1536 groups; a mid-loop cut (nine tiles into 1024 keys); a list of one key and an empty one: the no-sort path
    c = C["s1-1536-one-row-images"]
    p, rows = T.plan(c), replays[c.name]
    assert p["S"] == 1 and p["ng"] == 1536 and p["np2"] >= c.k
    assert p["U"][5] == 1 and p["U"][9] == 0 and rows[5]["lens"] == [1] and rows[9]["lens"] == [0]
    assert all(r["cuts"] == [1] for j, r in enumerate(rows) if j not in (5, 9))
    # S = 6, the final sort padded: np2 = 64 > 60
    c = C["s6-300-groups"]
    p = T.plan(c)
    assert p["S"] == 6 == p["S_wanted"] and p["np2"] == 64 > p["S"] * c.k and p["np2"] & (p["np2"] - 1) == 0
    # the memory rule: 200 groups ask for 8 slices, 512 MB allow 5; the one tile goes to slice 0
    c = C["s5-by-memory-12800-rows"]
    p = T.plan(c)
    assert p["S_wanted"] == 8 and p["S"] == 5 and p["S"] * c.k <= T.SL_FINAL_KEYS
    assert 12800 * 5 * 1024 * 8 <= T.SL_CAND_BYTES < 12800 * 6 * 1024 * 8
    assert all(t == [1, 0, 0, 0, 0] for t in p["tiles"])
    # every other case: S = 8; slices without a tile occur there too
    assert {T.plan(c)["S"] for c in T.CASES} == {1, 5, 6, 8}


def test_named_targets_of_the_running_threshold(replays):
    # k = 256 | 257 on the same data: cap 1024 | 2048
    a, b = C["cuts-k256"], C["cuts-k257"]
    assert a.data == b.data and (a.k, b.k) == (256, 257) and (T.plan(a)["cap"], T.plan(b)["cap"]) == (1024, 2048)
    assert min(T.plan(a)["U"]) >= 3 * 8 * (1024 - 128)
    # >= 3 mid-loop cuts of EVERY (row, slice) at cap 1024.  At cap 2048 a third cut needs 16 + 13 + 13 tiles per slice, a union of
    # 43008 rows: more than an index of 32768 rows holds -- one cut of every (row, slice) there
    assert _cuts(replays[a.name]).min() >= 3, _cuts(replays[a.name]).min()
    assert _cuts(replays[b.name]).min() >= 1
    assert all(all(r["end_cut"]) for r in replays[a.name] + replays[b.name])
    # the planted copies: >= k + 200 of them over many reference images; every row of image 0 cuts inside the run, in the loop
    # and at the end; the k best of every row are copies, so every slice contributes and the ids alone order the list
    c = C["ties-k256"]
    x, rows = T.make_data(c.data), replays[c.name]
    same = np.nonzero((x["R"] == x["R"][T.brute(c)[1][0, 0]]).all(1))[0]
    assert len(same) >= c.k + 200 and len(np.unique(x["img"][same])) >= 100
    assert all(r["tie_cut"] for r in rows[:40]) and _cuts(rows).min() >= 3
    d2, ids = T.brute(c)
    assert (d2[:, :c.k] == d2[:, :1]).all() and np.isin(ids, same).all() and (np.diff(ids, axis=1) > 0).all()
    u0 = T.unions(c.data)[0][0]
    slice_of = {int(r): (p // T.TILE) % 8 for p, r in enumerate(u0)}
    assert len({slice_of[int(r)] for r in ids[0]}) == 8
    # k = 1024: padding behind a short union and the final sort's 64 KiB; cap = 2048 cut in the loop, S k = 8192 exactly
    c = C["k1024-union-of-700"]
    p = T.plan(c)
    assert max(p["U"]) < c.k and p["final_lds_over_48k"] and p["np2"] == 8192 and (T.brute(c)[1][:, max(p["U"]):] == -1).all()
    c = C["k1024-union-of-17500"]
    p = T.plan(c)
    assert min(p["U"]) >= 8 * 1920 and p["cap"] == 2048 and p["S"] * c.k == T.SL_FINAL_KEYS and p["S"] == 8
    assert _cuts(replays[c.name]).min() >= 1 and p["final_lds_over_48k"]
    assert [c.name for c in T.CASES if T.plan(c)["final_lds_over_48k"]] == ["k1024-union-of-700", "k1024-union-of-17500"]


def test_named_targets_of_the_map_and_the_union():
    # the ordered scan: 4097 = SL_SORT_CAP + 1 and 9000 rows, in all three adds, in every wave of the scan's blocks; last block partial
    c = C["large-images-4097-9000"]
    p, x = T.plan(c), T.make_data(c.data)
    assert p["counts"][T.LARGE_A] == T.SL_SORT_CAP + 1 and p["counts"][T.LARGE_B] == 9000
    assert [i for i, b in enumerate(p["sort"]) if b == "scan"] == [T.LARGE_A, T.LARGE_B] and len(x["img"]) % 256 != 0
    assert sorted(p["counts"][p["sort"] == "lds"].tolist()) == [20] * 30 and (p["sort"] == "none").sum() == 8
    assert len(x["splits"]) == 3 and x["splits"][0][0] == 0 and x["splits"][-1][1] == len(x["img"])
    for g in (T.LARGE_A, T.LARGE_B):
        own = np.nonzero(x["img"] == g)[0]
        assert all(((own >= a) & (own < b)).any() for a, b in x["splits"])
        assert {int(w) for w in (own % 256) // 64} == {0, 1, 2, 3} and (own >= len(x["img"]) // 256 * 256).any()
        # the planted duplicates lie inside the image, and two of them are neighbours in the map
        dup = [r for r in own if ((x["R"][own] == x["R"][r]).all(1)).sum() == 2]
        assert len(dup) == 2 * T.LARGE_PAIRS
    assert x["sl"].tolist() == [[T.LARGE_A, -1, -1], [T.LARGE_B, -1, -1], [T.LARGE_A, 3, 11], [T.LARGE_B, 5, 30]]
    assert [c.name for c in T.CASES if (T.plan(c)["sort"] == "scan").any()] == [c.name]
    # the scan's stride and the small branches
    c = C["many-images-0-to-3-rows"]
    p = T.plan(c)
    assert p["nimg"] == 2500 and p["nimg"] % T.SL_SCAN_T != 0 and p["per"] == 3 and set(p["counts"]) == {0, 1, 2, 3}
    assert p["sort_np2"] == [2, 4] and (p["sort"] == "none").sum() > 1000 and len(T.make_data(c.data)["splits"]) == 3
    assert all(T.plan(c)["per"] == 1 for c in T.CASES if c.data != "many")
    # the union kernel: M = 1 | 65 | 4096
    for name, M, np2m in (("m1", 1, 64), ("m65", 65, 128), ("m4096", 4096, 4096)):
        x, p = T.make_data(C[name].data), T.plan(C[name])
        assert x["sl"].shape[1] == M and p["np2m"] == np2m
        rowless = np.nonzero(p["counts"] == 0)[0]
        assert (x["sl"] == -1).any() and np.isin(x["sl"], rowless).any()
    sl = T.make_data("m4096")["sl"]
    assert len(np.unique(sl[0])) <= 13 and T.plan(C["m4096"])["U"][3] == 10
    assert T.plan(C["m1"])["U"] == [0, 0, 10, 10]


# ---- the references ---------------------------------------------------------------------------------------------------------
def test_brute_force_on_a_toy_case_equals_a_float64_ranking():
    rng = np.random.default_rng(11)
    R = T._unit(rng.standard_normal((120, 32)).astype(np.float32))
    img = rng.integers(0, 6, 120).astype(np.int32)
    qoff = np.array([0, 7, 12], np.int32)
    Q = T._unit(R[rng.integers(0, 120, 12)] + 0.1 * rng.standard_normal((12, 32)).astype(np.float32))
    sl = np.array([[4, 1, 1, -1], [0, 5, 9, 2]], np.int32)               # a duplicate, -1, an id beyond the index
    k = 30
    d2, ids = T._brute(Q, R, img, qoff, sl, k)
    decided = 0
    for b in range(2):
        allowed = np.nonzero(np.isin(img, sl[b][sl[b] >= 0]))[0]
        assert len(allowed) >= k
        for q in range(qoff[b], qoff[b + 1]):
            d64 = ((Q[q].astype(np.float64)[None, :] - R[allowed].astype(np.float64)) ** 2).sum(1)
            o = np.argsort(d64, kind="stable")
            assert set(ids[q].tolist()) <= set(allowed.tolist()) and np.abs(d2[q] - d64[np.searchsorted(allowed, ids[q])]).max() < 1e-5
            gap = np.diff(d64[o])[:k]                                    # gap[j]: between the float64 ranks j and j + 1
            for j in range(k):
                if (j == 0 or gap[j - 1] > 1e-4) and gap[j] > 1e-4:
                    assert ids[q, j] == allowed[o[j]], (q, j)
                    decided += 1
    assert decided > 200, decided
    # the row-at-a-time form the table's vectorised one replaced
    qn, rn = E.row_sumsq(Q), E.row_sumsq(R)
    for q in (0, 11):
        allowed = np.nonzero(np.isin(img, sl[int(q >= 7)]))[0]
        dd = E.d2(qn[q], rn[allowed], E.dot_chain(Q[q], R[allowed]))
        o = np.lexsort((allowed, dd))[:k]
        assert np.array_equal(ids[q], allowed[o]) and np.array_equal(d2[q].view(np.uint32), dd[o].view(np.uint32))


def test_replay_ends_in_the_brute_forces_lists(replays):
    for c in T.CASES:
        d2, ids = T.brute(c)
        rows = replays[c.name]
        assert np.array_equal(np.stack([r["ids"] for r in rows]), ids), c.name
        assert np.array_equal(np.stack([r["d2"] for r in rows]).view(np.uint32), d2.view(np.uint32)), c.name
        p = T.plan(c)
        for b, U in enumerate(p["U"]):
            q0, q1 = T.make_data(c.data)["qoff"][b:b + 2]
            assert (ids[q0:q1, :min(U, c.k)] >= 0).all() and (ids[q0:q1, min(U, c.k):] == -1).all()
