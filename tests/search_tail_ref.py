"""Plain references of the search tail -- segvlad_vote (both modes), segvlad_merge_topk, segvlad_sims_from_d2, segvlad_minmax -- and
the generators of the inputs that tests/test_gpu_search_tail.py runs them on.  NumPy and python only; written to be read.

tests/test_search_tail_ref.py pins the references to the oracle and asserts, per generated case, the conditions that make the case
worth running (its regime, planted weights, ties, ...): a generator change cannot silently empty a case."""
import functools

import numpy as np

INF = np.float32(np.inf)
TWO_M17 = 2.0 ** -17


# =====================================================================================================================
# references
# =====================================================================================================================
def weights(sims, smin=None, smax=None):
    """The vote's weights, fp32 as NumPy forms them: (sims - smin) / (smax - smin) on float32 arrays; the extrema default to those
    of ALL of sims."""
    sims = np.asarray(sims, np.float32)
    smin = np.float32(np.min(sims) if smin is None else smin)
    smax = np.float32(np.max(sims) if smax is None else smax)
    return (sims - smin) / (smax - smin)


def visiting_order(a, off, b):
    """Query image b's entries of a [nq][k] array in the vote's visiting order: rank-major, then segment."""
    return np.asarray(a)[off[b]:off[b + 1]].T.reshape(-1)


def _kept(matches, off, b, n_ref):
    ids = visiting_order(matches, off, b)
    keep = (ids >= 0) & (ids < n_ref)                     # an id outside [0, n_ref) is skipped
    return ids, keep


def padded(rows, n_top):
    ids = np.full((len(rows), n_top), -1, np.int32)
    sc = np.zeros((len(rows), n_top), np.float64)
    for b, row in enumerate(rows):
        for j, (g, s) in enumerate(row[:n_top]):
            ids[b, j], sc[b, j] = g, s
    return ids, sc


def vote_wt_ranking(matches, sims, off, img_of_seg, smin=None, smax=None):
    """Per query image the WHOLE ranking [(image id, fp64 score), ...]: python floats added in visiting order into a dict keyed by
    image id, ordered by (score descending, first appearance)."""
    img_of_seg = np.asarray(img_of_seg)
    w = weights(sims, smin, smax)
    out = []
    for b in range(len(off) - 1):
        ids, keep = _kept(matches, off, b, len(img_of_seg))
        scores = {}
        for g, x in zip(img_of_seg[ids[keep]].tolist(), visiting_order(w, off, b)[keep].tolist()):
            if g in scores:
                scores[g] += x
            else:
                scores[g] = x
        ranked = sorted(scores, key=lambda g: scores[g], reverse=True)      # stable: ties keep the dict's (first-appearance) order
        out.append([(g, scores[g]) for g in ranked])
    return out


def vote_count_ranking(matches, off, img_of_seg):
    """The same walk, counting; ordered by (count descending, image id ascending)."""
    img_of_seg = np.asarray(img_of_seg)
    out = []
    for b in range(len(off) - 1):
        ids, keep = _kept(matches, off, b, len(img_of_seg))
        counts = {}
        for g in img_of_seg[ids[keep]].tolist():
            counts[g] = counts.get(g, 0) + 1
        out.append([(g, float(counts[g])) for g in sorted(counts, key=lambda g: (-counts[g], g))])
    return out


def vote_wt(matches, sims, off, img_of_seg, n_top, smin=None, smax=None):
    """(ids [n_img][n_top] int32 padded with -1, scores [n_img][n_top] float64 padded with 0.0)."""
    return padded(vote_wt_ranking(matches, sims, off, img_of_seg, smin, smax), n_top)


def vote_count(matches, off, img_of_seg, n_top):
    return padded(vote_count_ranking(matches, off, img_of_seg), n_top)


def merge(d2_parts, idx_parts, k):
    """Top-k of every row over all parts by (distance, id); an entry with id < 0 is padding whatever its distance: it comes last
    and is emitted as (inf, -1).  The parts: a list of [nq][k_part] arrays, or one [nq][parts * k_part] array."""
    d2 = np.concatenate(d2_parts, axis=1) if isinstance(d2_parts, (list, tuple)) else np.asarray(d2_parts)
    idx = np.concatenate(idx_parts, axis=1) if isinstance(idx_parts, (list, tuple)) else np.asarray(idx_parts)
    d2 = d2.astype(np.float32)
    idx = idx.astype(np.int64)
    pad = idx < 0
    order = np.lexsort((idx, np.where(pad, INF, d2), pad), axis=1)[:, :k]   # last key first: padding, then distance, then id
    od = np.take_along_axis(np.where(pad, INF, d2), order, 1)
    oi = np.take_along_axis(np.where(pad, -1, idx), order, 1)
    if od.shape[1] < k:                                  # (fewer candidates than k)
        od = np.concatenate([od, np.full((len(od), k - od.shape[1]), INF, np.float32)], 1)
        oi = np.concatenate([oi, np.full((len(oi), k - oi.shape[1]), -1, np.int64)], 1)
    return od, oi


def sims_from_d2(d2, idx, k_keep):
    return np.float32(2.0) - np.asarray(d2, np.float32)[:, :k_keep], np.asarray(idx, np.int64)[:, :k_keep].copy()


def minmax(x):
    x = np.asarray(x, np.float32).reshape(-1)
    if x.size == 0:
        return np.float32(np.nan), np.float32(np.nan)
    return np.min(x), np.max(x)


# =====================================================================================================================
# the vote's launch rule
# =====================================================================================================================
def launch_regime(seg_counts, k):
    """Mirror of sv_launch_vote (csrc/vote_kernels.hip): (regime of the in-LDS launch, its pow2 padding, images left to GLOBAL)."""
    small = [s * k for s in seg_counts if s * k <= 16384]
    epad = 2
    while epad < max(small, default=0):
        epad *= 2
    regime = "fast" if epad <= 4096 else "weights_in_lds" if epad * 12 <= 128 * 1024 else "no_weight_array"
    return regime, epad, [i for i, s in enumerate(seg_counts) if s * k > 16384]


# name -> (segments, k, entries, regime, pow2 padding of the image)
VOTE_CASES = {
    "fast_last_64x64": (64, 64, 4096, "fast", 4096),
    "wl_first_241x17": (241, 17, 4097, "weights_in_lds", 8192),
    "wl_last_64x128": (64, 128, 8192, "weights_in_lds", 8192),
    "nowl_first_2731x3": (2731, 3, 8193, "no_weight_array", 16384),
    "nowl_last_128x128": (128, 128, 16384, "no_weight_array", 16384),
    "global_first_145x113": (145, 113, 16385, "global", 32768),
    "bench_depth_50x200": (50, 200, 10000, "no_weight_array", 16384),
}
# one shape per regime, for the order-sensitive sums and the ties
REGIME_SHAPES = ["fast_last_64x64", "wl_first_241x17", "nowl_first_2731x3", "global_first_145x113"]


def case_regime(seg_counts, k):
    """The regime that the batch's LARGEST image runs in: "global" when it is left to the second launch."""
    regime, epad, big = launch_regime(seg_counts, k)
    largest = int(np.argmax(seg_counts))
    if largest in big:
        e, epad = seg_counts[largest] * k, 2
        while epad < e:
            epad *= 2
        return "global", epad
    return regime, epad


# =====================================================================================================================
# vote inputs
# =====================================================================================================================
N_REF_IMG, SEGS_PER_REF = 200, 10
LARGEST = 1                                              # position of the case's largest image in its batch


@functools.lru_cache(maxsize=None)
def ref_map():
    """img_of_seg [2000] int32: 200 reference images of 10 segments each, scattered."""
    rng = np.random.default_rng(2000)
    return rng.permutation(np.repeat(np.arange(N_REF_IMG, dtype=np.int32), SEGS_PER_REF))


def batch_shape(name):
    """The batch of a vote case: a 3-segment image, the case's largest image, an image without segments, a mid-size image."""
    segs, k = VOTE_CASES[name][:2]
    counts = [3, segs, 0, max(4, segs // 3)]
    return counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), k


def _concentrated(rng, off, k, img_of_seg, share=0.5, n_hot=4):
    """Random segment ids, with `share` of every query image's entries redirected to n_hot reference images of its own: runs of
    hundreds of entries."""
    n_img_ref = int(img_of_seg.max()) + 1
    segs_of = np.argsort(img_of_seg, kind="stable").reshape(n_img_ref, -1)
    m = rng.integers(0, len(img_of_seg), size=(int(off[-1]), k))
    hot = []
    for b in range(len(off) - 1):
        pool = rng.choice(n_img_ref, size=n_hot, replace=False)
        hot.append(pool)
        rows = slice(off[b], off[b + 1])
        shape = m[rows].shape
        sel = rng.random(shape) < share
        repl = segs_of[pool[rng.integers(0, n_hot, size=shape)], rng.integers(0, segs_of.shape[1], size=shape)]
        m[rows] = np.where(sel, repl, m[rows])
    return m.astype(np.int64), hot


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


@functools.lru_cache(maxsize=None)
def vote_case(name):
    """matches, sims (descending per row, as a search emits them), off, img_of_seg, k of a regime / boundary case."""
    counts, off, k = batch_shape(name)
    rng = np.random.default_rng(_seed(name))
    im = ref_map()
    matches, _ = _concentrated(rng, off, k, im)
    sims = np.sort(rng.uniform(0.2, 1.9, size=matches.shape).astype(np.float32), axis=1)[:, ::-1].copy()
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)


def with_invalid_ids(case, seed=5):
    """About 5 % of the ids replaced by -1, n_ref and n_ref + 7: the empty slots of a derived search and ids past the map."""
    rng = np.random.default_rng(seed)
    n_ref = len(case["img_of_seg"])
    m = case["matches"].copy()
    sel = rng.random(m.shape) < 0.05
    m[sel] = rng.choice(np.array([-1, n_ref, n_ref + 7], np.int64), size=int(sel.sum()))
    return dict(case, matches=m)


def inner_extrema(sims):
    """Explicit extrema strictly inside the data's range: 5 % of the weights fall below 0 and 5 % above 1."""
    lo, hi = np.quantile(np.asarray(sims, np.float64), [0.05, 0.95])
    return float(np.float32(lo)), float(np.float32(hi))


def n_top_set(case):
    """1, 5, and one more than the number of distinct images of the 3-segment image (so that its row ends in padding)."""
    ids = visiting_order(case["matches"], case["off"], 0)
    ids = ids[(ids >= 0) & (ids < len(case["img_of_seg"]))]
    return [1, 5, len(np.unique(case["img_of_seg"][ids])) + 1]


def run_edges_beside_skipped(case, b):
    """Of query image b: (run starts, run ends) that have a skipped entry as a neighbour in the visiting order.  A run is the
    sequence of an image's entries; its start / end are the first / last appearance of the image."""
    im = case["img_of_seg"]
    ids, keep = _kept(case["matches"], case["off"], b, len(im))
    g = np.where(keep, im[np.where(keep, ids, 0)], -1)
    beside = np.zeros(len(g), bool)
    beside[1:] |= ~keep[:-1]
    beside[:-1] |= ~keep[1:]
    pos = np.nonzero(keep)[0]
    _, first = np.unique(g[pos], return_index=True)
    _, last = np.unique(g[pos][::-1], return_index=True)
    return int(beside[pos[first]].sum()), int(beside[pos[::-1][last]].sum())


# ---- order-sensitive sums -------------------------------------------------------------------------------------------
def _plant_tiny(rng, case, b, hot, per_run, scale, step):
    """Replace, in query image b, `per_run` similarities of every hot image's run by values of order `scale` (the minimum of sims
    is 0.0, so these ARE the small weights, with full 24-bit mantissas).  A small weight added to a running sum S is rounded to
    ulp(S), so WHERE in the run it is added decides the result: the places are the entries `step` before and behind those at which
    the run's sum, in visiting order, passes a power of two -- an entry that an unordered sum adds one binade early or late rounds
    differently.  Returns the number planted."""
    im, off = case["img_of_seg"], case["off"]
    sims = case["sims"]
    S = int(off[b + 1] - off[b])
    ids = visiting_order(case["matches"], off, b)
    n = 0
    for g in hot:
        o = np.nonzero(im[ids] == g)[0]                   # the run, in visiting order
        cum = np.cumsum(visiting_order(sims, off, b)[o].astype(np.float64))
        where = []
        c = 2.0 ** np.floor(np.log2(cum[-1]))
        while len(where) < per_run and c > cum[0]:
            j = int(np.searchsorted(cum, c))              # the entry at which the running sum reaches c
            where += [x for x in (j - step, j + step) if 0 <= x < len(o) and x not in where]
            c /= 2
        for j in where[:per_run]:
            rank, seg = divmod(int(o[j]), S)
            sims[off[b] + seg, rank] = np.float32(scale * (1.0 + rng.random()))
            n += 1
    return n


@functools.lru_cache(maxsize=None)
def order_case(name):
    """The batch shape of vote_case(name) with similarities in [0, 1], an exact 0.0 as their minimum, and about 30 similarities of
    order 1e-9 (and twice as many of order 1e-13: they lose bits from a running sum of 2^-10 on) planted into the hot runs of the largest
    image.  Not sorted per row: the vote does not ask for it."""
    counts, off, k = batch_shape(name)
    rng = np.random.default_rng(_seed(name) + 1)
    im = ref_map()
    matches, hot = _concentrated(rng, off, k, im)
    sims = rng.uniform(0.01, 1.0, size=matches.shape).astype(np.float32)
    case = dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)
    n9 = _plant_tiny(rng, case, LARGEST, hot[LARGEST], 8, 1e-9, 1)
    n13 = _plant_tiny(rng, case, LARGEST, hot[LARGEST], 16, 1e-13, 3)
    sims[off[0], k - 1] = 0.0                             # the global minimum, in the 3-segment image
    case["planted"] = n9 + n13
    case["hot"] = hot[LARGEST]
    return case


def planted_weights(case):
    """(number of weights strictly between 0 and 2^-17, runs of the largest image that hold one and sum to more than 2)."""
    w = weights(case["sims"])
    small = (w > 0) & (w < TWO_M17)
    b = LARGEST
    ids = visiting_order(case["matches"], case["off"], b)
    sm = visiting_order(small, case["off"], b)
    imgs = set(case["img_of_seg"][ids[sm]].tolist())
    score = dict(vote_wt_ranking(case["matches"], case["sims"], case["off"], case["img_of_seg"])[b])
    return int(small.sum()), sum(1 for g in imgs if score[g] > 2.0)


@functools.lru_cache(maxsize=None)
def single_run_case():
    """64 x 64: all 4096 entries of the image on ONE reference image, ordinary weights -- the longest run that the exactness argument
    of the fast path covers.  Beside it a 3-segment image."""
    rng = np.random.default_rng(4096)
    im = ref_map()
    off = np.array([0, 64, 67], np.int32)
    k = 64
    matches = rng.integers(0, len(im), size=(67, k)).astype(np.int64)
    matches[:64] = rng.choice(np.nonzero(im == 17)[0], size=(64, k))
    sims = rng.uniform(0.2, 1.9, size=matches.shape).astype(np.float32)
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=[64, 3])


# ---- batch composition ----------------------------------------------------------------------------------------------
COMPANIONS = [0, 82, 164, 328]                           # segments at k = 50: alone, 4100, 8200 and 16400 entries
COMPOSITION_EXTREMA = (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def composition_case(companion, poison):
    """A fixed 40 x 50 image, alone or beside a companion image that moves the launch into another regime.  Similarities in
    [0, 1) and explicit extrema (0, 1): the fixed image's weights are its similarities whatever stands beside it.  poison: tiny
    similarities in the fixed image's hot runs.  Returns the case and the fixed image's position in the batch."""
    k = 50
    rng = np.random.default_rng(4050)
    im = ref_map()
    off1 = np.array([0, 40], np.int32)
    m1, hot = _concentrated(rng, off1, k, im)
    s1 = rng.uniform(0.01, 1.0, size=m1.shape).astype(np.float32)
    fixed = dict(matches=m1, sims=s1, off=off1, img_of_seg=im, k=k, counts=[40])
    if poison:
        fixed["planted"] = _plant_tiny(rng, fixed, 0, hot[0], 6, 1e-9, 1) + _plant_tiny(rng, fixed, 0, hot[0], 12, 1e-13, 3)
    if companion == 0:
        return fixed, 0
    rng = np.random.default_rng(companion)
    off2 = np.array([0, companion], np.int32)
    m2, _ = _concentrated(rng, off2, k, im)
    s2 = rng.uniform(0.0, 1.0, size=m2.shape).astype(np.float32)
    first = companion == 164                             # the fixed image comes second in one of the batches
    parts = [(m2, s2), (m1, s1)] if first else [(m1, s1), (m2, s2)]
    counts = [companion, 40] if first else [40, companion]
    case = dict(matches=np.concatenate([p[0] for p in parts]), sims=np.concatenate([p[1] for p in parts]),
                off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), img_of_seg=im, k=k, counts=counts)
    return case, 1 if first else 0


# ---- ties -----------------------------------------------------------------------------------------------------------
TIE_N_TOP = 20


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """The batch shape of vote_case(name); similarities from {0, 0.25, 0.5, 1}: the weights are the similarities and every sum is
    exact, so many images reach equal scores.  A reference map of its own, one segment per image and about 8 entries per image
    of the largest query image, scattered ids: first appearance and lower id disagree."""
    counts, off, k = batch_shape(name)
    rng = np.random.default_rng(_seed(name) + 2)
    n_ref = max(50, counts[LARGEST] * k // 8)
    im = rng.permutation(n_ref).astype(np.int32)
    matches = rng.integers(0, n_ref, size=(int(off[-1]), k)).astype(np.int64)
    sims = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), size=matches.shape)
    sims[0, 0], sims[0, 1] = 0.0, 1.0
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)


def tie_groups(ranking, n_top):
    """Groups of >= 2 images with equal scores that begin inside the first n_top places: [[image ids in ranked order], ...]."""
    groups, i = [], 0
    while i < min(n_top, len(ranking)):
        j = i
        while j + 1 < len(ranking) and ranking[j + 1][1] == ranking[i][1]:
            j += 1
        if j > i and i + 1 < n_top:                      # at least two of the group's places are compared
            groups.append([g for g, _ in ranking[i:j + 1]][:n_top - i])
        i = j + 1
    return groups


# =====================================================================================================================
# merge inputs
# =====================================================================================================================
MERGE_SHAPES = [(1, 50), (3, 50), (8, 200), (8, 1024), (5, 13), (2, 1), (3, 1000)]
MERGE_KINDS = ["distinct", "ties", "padded", "unsorted", "midpad", "duplicates"]
TIE_POOL = np.array([0.0, 0.125, 0.3, 0.5, 0.75, 1.0, 1.5, 1.9], np.float32)


def merge_rows(parts, k):
    return 48 if parts * k >= 3000 else 150


def sorted_parts(d, i, parts, k):
    """Order every part of every row by (distance, id), padding (id < 0) last."""
    nq = len(d)
    d3, i3 = d.reshape(nq, parts, k), i.reshape(nq, parts, k)
    order = np.lexsort((i3, d3, i3 < 0), axis=2)
    return (np.take_along_axis(d3, order, 2).reshape(nq, parts * k).copy(),
            np.take_along_axis(i3, order, 2).reshape(nq, parts * k).copy())


@functools.lru_cache(maxsize=None)
def merge_case(parts, k, kind):
    """(d2 [nq][parts * k] float32, idx [nq][parts * k] int64): non-negative finite distances (no -0.0, no NaN) or +inf with id -1;
    distinct ids (but for the kind "duplicates"), scattered over the parts so that the id order says nothing about the part."""
    nq, cand = merge_rows(parts, k), parts * k
    rng = np.random.default_rng(1000 * parts + k + 7 * MERGE_KINDS.index(kind))
    idx = np.stack([rng.permutation(3 * cand)[:cand] for _ in range(nq)]).astype(np.int64) + 5_000_000_000 * (np.arange(nq)[:, None] % 2)
    if kind in ("ties", "duplicates"):
        d = np.empty((nq, cand), np.float32)
        for q in range(nq):                              # (a row of few candidates draws from few values: equal pairs everywhere)
            pool = rng.choice(TIE_POOL, size=min(8, max(1, cand // 2)), replace=False)
            d[q] = rng.choice(pool, size=cand)
    else:
        d = np.stack([rng.permutation(4 * cand)[:cand] for _ in range(nq)]).astype(np.float32) * np.float32(0.001)
    if kind == "padded":
        length = rng.integers(0, k + 1, size=(nq, parts))
        length[0] = 0                                    # a row where every part is padding
        if nq > 1:
            length[1] = 0
            length[1, 1 % parts] = k                     # a row where a single part holds all the entries
        pad = (np.arange(k)[None, None, :] >= length[:, :, None]).reshape(nq, cand)
        d[pad], idx[pad] = INF, -1
    d, idx = sorted_parts(d, idx, parts, k)
    if kind == "duplicates":
        # The SAME (distance, id) in two parts, as shards that overlap would list it: the only entries that compare equal under
        # (distance, id), so the only ones the rank merge's rule for equal entries is there for.  The first entry of every even
        # part goes into the next part as well, and a few deeper ones into a random other part.
        for q in range(nq):
            for r in range(0, parts - 1, 2):
                d[q, (r + 1) * k], idx[q, (r + 1) * k] = d[q, r * k], idx[q, r * k]
            for _ in range(min(4, k - 1) if parts > 1 else 0):
                r, r2 = rng.choice(parts, size=2, replace=False)
                a, b = int(rng.integers(1, k)), int(rng.integers(1, k))
                if idx[q, r * k + a] not in idx[q, r2 * k:(r2 + 1) * k]:
                    d[q, r2 * k + b], idx[q, r2 * k + b] = d[q, r * k + a], idx[q, r * k + a]
        d, idx = sorted_parts(d, idx, parts, k)
    if kind == "unsorted" and k >= 2:                    # (a part of one entry cannot be out of order)
        for q in range(0, nq, 3):
            r = int(rng.integers(parts))
            a, b = sorted(rng.choice(k, size=2, replace=False).tolist())
            for arr in (d, idx):
                arr[q, r * k + a], arr[q, r * k + b] = arr[q, r * k + b], arr[q, r * k + a]
    if kind == "midpad":
        for q in range(nq):
            j = int(rng.integers(parts)) * k + k // 2
            idx[q, j] = -1
            if q % 2:
                d[q, j] = INF                            # (the even rows keep a finite distance in the slot: it must not count)
    return d, idx


def cross_part_tie_rows(d, idx, parts, k):
    """Rows in which an equal-distance pair from two different parts sits inside, or straddles the end of, the first k places."""
    n = 0
    for q in range(len(d)):
        valid = idx[q] >= 0
        order = np.lexsort((idx[q], d[q], ~valid))
        dq, part = d[q][order], (order // k)
        hit = False
        for p in range(min(k, int(valid.sum()) - 1)):    # entry p is inside the first k; p + 1 inside or just behind
            if dq[p] == dq[p + 1] and part[p] != part[p + 1]:
                hit = True
                break
        n += hit
    return n


def cross_part_duplicate_rows(d, idx, parts, k):
    """Rows in which the same (distance, id) is listed by two different parts and the pair sits inside, or straddles the end of,
    the first k places."""
    n = 0
    for q in range(len(d)):
        order = np.lexsort((idx[q], d[q], idx[q] < 0))
        dq, iq, part = d[q][order], idx[q][order], order // k
        same = (dq[:-1] == dq[1:]) & (iq[:-1] == iq[1:]) & (iq[:-1] >= 0) & (part[:-1] != part[1:])
        n += bool(same[:k].any())
    return n


# =====================================================================================================================
# sims_from_d2 and minmax inputs
# =====================================================================================================================
SIMS_SHAPES = [(200, 50), (50, 50), (7, 1), (1024, 1023)]


@functools.lru_cache(maxsize=None)
def sims_case(nq, k_in):
    """Ascending distance rows in [0, 4) with ids; every third row ends in a (+inf, -1) tail of its own length (one row is all
    tail)."""
    rng = np.random.default_rng(nq * 10000 + k_in)
    d = np.sort(rng.uniform(0.0, 4.0, size=(nq, k_in)).astype(np.float32), axis=1)
    idx = rng.integers(0, 1 << 40, size=(nq, k_in)).astype(np.int64)
    for q in range(0, nq, 3):
        n_tail = k_in if q == 0 else int(rng.integers(1, k_in + 1))
        d[q, k_in - n_tail:], idx[q, k_in - n_tail:] = INF, -1
    return d, idx


MINMAX_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1024 * 256, 1024 * 256 + 1, 3 * (1 << 18) + 5]
MINMAX_KINDS = ["min_first_max_last", "max_first_min_last", "inf_inside"]


@functools.lru_cache(maxsize=None)
def minmax_case(count, kind):
    """Values of both signs, no NaN and no zero; the extrema at the two ends, or -inf / +inf somewhere inside."""
    rng = np.random.default_rng(count + 31 * MINMAX_KINDS.index(kind))
    x = rng.standard_normal(count).astype(np.float32)
    x[x == 0] = 1.0
    if count == 0:
        return x
    lo, hi = np.float32(-7.5), np.float32(9.25)
    if kind == "inf_inside":
        lo, hi = -INF, INF
        a, b = (0, 0) if count == 1 else rng.choice(count, size=2, replace=False)
    elif kind == "min_first_max_last":
        a, b = 0, count - 1
    else:
        a, b = count - 1, 0
    x[a] = lo
    if count > 1 or kind == "max_first_min_last":
        x[b] = hi
    return x
