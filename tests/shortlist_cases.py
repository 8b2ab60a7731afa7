"""Hand-chosen shapes of segvlad_search_shortlist and of the image -> row map it builds (csrc/shortlist_kernels.hip), one per branch
of its host arithmetic and of its kernels' bookkeeping, with the data each one runs on and the host references it is held against
(host code: no GPU, no library).

    plan()       a restatement of the host arithmetic of search_shortlist, sl_launch_gemm and sl_build_map: the groups and MT, the
                 slice count S and the buffer size cap, the final sort's size, the union kernel's size, the map's sort branch per
                 reference image and the scan's stride, and per query image the union size U and the tiles every slice gets
    simulate()   a replay of sl_gemm_kernel's candidate bookkeeping for ONE query row -- per slice the tiles s, s + S, ..., every
                 key below the running threshold appended, a buffer of more than cap - 128 keys cut to its k best (the k-th key
                 the new threshold), the end cut to <= k -- and of sl_final_kernel's merge, on emulated distances
    _brute()     the contract: per query row the rows of its image's shortlisted reference images, the device's exact fp32
                 distance (tests/fp32_emu.py), (distance, id) order, (+inf, -1) padding
    CASES        the table; tests/test_shortlist_cases.py holds every case against plan() and simulate() on the CPU,
                 tests/test_gpu_shortlist_cases.py holds the device against _brute(), bit for bit

A case is named data (DATA: an index (R, img, the db_add splits), queries (Q, qoff), a shortlist [n_img][M]), a k and the number of
floats between a 16-byte boundary and the device query view.  Rows are unit-norm, the generator is seeded by the data's name.
Every case keeps sum over query rows of U(row) d <= COST_CAP (the brute force stays at a few seconds of NumPy) and its index at
<= 32768 rows (segvlad_search, which the neighbouring tests compare with, plans no filter there)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import fp32_emu as E

# the constants of csrc/shortlist_kernels.hip (tests/test_shortlist_cases.py reads them out of the source and compares)
SL_GMAX, SL_SORT_CAP, SL_SLICES_MAX, SL_SCAN_T = 64, 4096, 8, 1024
SL_WORKGROUPS, SL_FINAL_KEYS, SL_CAND_BYTES = 1536, 8192, 512 << 20
SL_CAP_SMALL, SL_CAP_LARGE, SL_CAP_K = 1024, 2048, 256
TILE = 128
COST_CAP = 6.4e7
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def cap_of(k):
    return SL_CAP_SMALL if k <= SL_CAP_K else SL_CAP_LARGE


# ---- the contract ---------------------------------------------------------------------------------------------------------
def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def image_rows(img, n_img_ref=None):
    """The image -> row map: (off [n_img_ref + 1], rows [rows with an id >= 0]) -- image g's rows, ascending, are rows[off[g]:off[g + 1]]."""
    img = np.asarray(img, np.int64)
    n_img_ref = int(img.max()) + 1 if n_img_ref is None else n_img_ref
    held = np.nonzero(img >= 0)[0]
    rows = held[np.argsort(img[held], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(img[held], minlength=n_img_ref))])
    return off, rows


def union_rows(img, shortlist_b, m=None):
    """One query image's union in the device's order: its shortlist's ids that carry rows, ascending and once each, every image's
    rows ascending.  m: image_rows(img), when the caller has it."""
    off, rows = image_rows(img) if m is None else m
    ids = np.unique(np.asarray(shortlist_b, np.int64))
    ids = ids[(ids >= 0) & (ids < len(off) - 1)]
    return np.concatenate([rows[off[g]:off[g + 1]] for g in ids] + [np.zeros(0, np.int64)])


def pair_d2(Q, R, qn, rn, qi, ri):
    """The emulated fp32 distance of the pairs (Q[qi[j]], R[ri[j]]), in blocks of at most 2^23 / d pairs."""
    out = np.empty(len(qi), np.float32)
    step = max(1, (1 << 23) // Q.shape[1])
    for a in range(0, len(qi), step):
        q, r = qi[a:a + step], ri[a:a + step]
        out[a:a + step] = E.d2(qn[q], rn[r], E.dot_chain(Q[q], R[r]))
    return out


def union_d2(Q, R, img, qoff, shortlist):
    """Per query image b: (ids [U_b] in union order, D [rows_b][U_b] emulated fp32 distances).  The pairs of all images run through
    the emulation together: a thousand one-row images cost what one image of a thousand rows costs."""
    Q, R = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(R, np.float32)
    qn, rn = E.row_sumsq(Q), E.row_sumsq(R)        # (the entry sums the norms of an ALIGNED copy of the queries: sv_aligned_queries)
    m = image_rows(img)
    ids = [union_rows(img, shortlist[b], m) for b in range(len(qoff) - 1)]
    rws = [np.arange(qoff[b], qoff[b + 1]) for b in range(len(qoff) - 1)]
    qi = np.concatenate([np.repeat(a, len(u)) for a, u in zip(rws, ids)] + [np.zeros(0, np.int64)]).astype(np.int64)
    ri = np.concatenate([np.tile(u, len(a)) for a, u in zip(rws, ids)] + [np.zeros(0, np.int64)]).astype(np.int64)
    flat = pair_d2(Q, R, qn, rn, qi, ri)
    out, at = [], 0
    for a, u in zip(rws, ids):
        out.append((u, flat[at:at + len(a) * len(u)].reshape(len(a), len(u))))
        at += len(a) * len(u)
    return out


def rank(unions, nq, qoff, k):
    """(d2 [nq][k], ids [nq][k]) from union_d2()'s output: (distance, id) order, (+inf, -1) padding."""
    d2 = np.full((nq, k), np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    for b, (u, D) in enumerate(unions):
        if not D.size:
            continue
        by_id = np.argsort(u, kind="stable")
        o = by_id[np.argsort(D[:, by_id], axis=1, kind="stable")[:, :k]]          # stable over ascending ids: (distance, id)
        d2[qoff[b]:qoff[b + 1], :o.shape[1]] = np.take_along_axis(D, o, 1)
        ids[qoff[b]:qoff[b + 1], :o.shape[1]] = u[o]
    return d2, ids


def _brute(Q, R, img, qoff, shortlist, k):
    """Host reference: per query row, the rows whose image is in its image's shortlist, emulated fp32 distances,
    (distance, id) order, (+inf, -1) padding."""
    return rank(union_d2(Q, R, img, qoff, shortlist), Q.shape[0], qoff, k)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def groups_of(qoff):
    """search_shortlist's groups: an image's rows in ceil(rows / 64) near-equal runs -- [(q0, nrows, image)]."""
    out = []
    for b in range(len(qoff) - 1):
        rws = int(qoff[b + 1]) - int(qoff[b])
        if rws <= 0:
            continue
        ng = -(-rws // SL_GMAX)
        for j in range(ng):
            a0, a1 = int(qoff[b]) + rws * j // ng, int(qoff[b]) + rws * (j + 1) // ng
            out.append((a0, a1 - a0, b))
    return out


def slices_of(ng, n_lists, k):
    """sl_launch_gemm's slice count: ~1536 workgroups, at most 8 slices, at most 8192 keys in a row's final sort, at most 512 MB of
    candidate buffers."""
    cap = cap_of(k)
    S = max(1, min(SL_SLICES_MAX, -(-SL_WORKGROUPS // max(ng, 1))))
    while S > 1 and (S * k > SL_FINAL_KEYS or n_lists * S * cap * 8 > SL_CAND_BYTES):
        S -= 1
    return S


def plan_of(img, qoff, shortlist, k, d):
    img, qoff, shortlist = np.asarray(img), np.asarray(qoff), np.asarray(shortlist)
    nq, n_img, M = int(qoff[-1]), len(qoff) - 1, shortlist.shape[1]
    grp = groups_of(qoff)
    gmax = max([g[1] for g in grp] + [0])
    p = {"groups": grp, "ng": len(grp), "gmax": gmax, "MT": 2 if gmax > 32 else 1, "cap": cap_of(k)}
    p["S_wanted"] = max(1, min(SL_SLICES_MAX, -(-SL_WORKGROUPS // max(len(grp), 1))))
    S = p["S"] = slices_of(len(grp), nq, k)
    np2 = 2
    while np2 < S * k:
        np2 <<= 1
    p["np2"], p["final_lds_over_48k"] = np2, np2 * 8 > 48 * 1024
    np2m = 64
    while np2m < M:
        np2m <<= 1
    p["np2m"] = np2m
    # the map: rows per reference image, the scan's images per thread, the sort branch per image
    nimg = int(img.max()) + 1
    cnt = np.bincount(img[img >= 0], minlength=nimg)
    p["nimg"], p["per"], p["counts"] = nimg, -(-nimg // SL_SCAN_T), cnt
    p["sort"] = np.where(cnt <= 1, "none", np.where(cnt <= SL_SORT_CAP, "lds", "scan"))
    p["sort_np2"] = sorted({1 << int(c - 1).bit_length() for c in cnt if 1 < c <= SL_SORT_CAP})      # (the LDS sort's padded size)
    # per query image: the union and the tiles of every slice
    off = np.concatenate([[0], np.cumsum(cnt)])
    p["U"], p["tiles"] = [], []
    for b in range(n_img):
        ids = np.unique(shortlist[b])
        ids = ids[(ids >= 0) & (ids < nimg)]
        U = int((off[ids + 1] - off[ids]).sum())
        p["U"].append(U)
        p["tiles"].append([len(range(s, -(-U // TILE), S)) for s in range(S)])
    p["cost"] = float(sum(U * (int(qoff[b + 1]) - int(qoff[b])) for b, U in enumerate(p["U"]))) * d
    return p


# ---- the replay -----------------------------------------------------------------------------------------------------------
def keys_of(d2, ids):
    """(f2key_(distance) << 32) | row id, the device's 64-bit sort key."""
    u = np.ascontiguousarray(d2, np.float32).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return (u.astype(np.uint64) << np.uint64(32)) | np.asarray(ids).astype(np.uint64)


def replay(S, cap, k, d2, ids):
    """sl_gemm_kernel's bookkeeping for one query row over the union (d2, ids) in union order, then sl_final_kernel's merge."""
    keys = keys_of(d2, ids)
    ntile = -(-len(keys) // TILE)
    cuts, end_cut, lens, tie, lists = [], [], [], False, []

    def cut(buf):
        s = np.sort(buf)
        inside = len(s) > k and (s[k - 1] >> np.uint64(32)) == (s[k] >> np.uint64(32))
        return s[:k], (s[k - 1] if len(s) >= k else None), inside

    for s in range(S):
        buf, thr, n_cuts = np.zeros(0, np.uint64), KEY_NONE, 0
        for t in range(s, ntile, S):
            kt = keys[t * TILE:(t + 1) * TILE]
            buf = np.concatenate([buf, kt[kt < thr]])
            assert len(buf) <= cap, "a candidate buffer overflows"
            if len(buf) > cap - TILE:
                buf, th, inside = cut(buf)
                thr = thr if th is None else th
                tie |= inside
                n_cuts += 1
        e = len(buf) > k
        if e:
            buf, _, inside = cut(buf)
            tie |= inside
        cuts.append(n_cuts)
        end_cut.append(e)
        lens.append(len(buf))
        lists.append(buf)
    a = np.concatenate(lists)
    if S > 1 or len(a) > 1:
        a = np.sort(a)
    a = a[:k]
    u = (a >> np.uint64(32)).astype(np.uint32)
    dd = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
    out_d = np.full(k, np.inf, np.float32)
    out_i = np.full(k, -1, np.int64)
    out_d[:len(a)] = dd
    out_i[:len(a)] = np.where(dd < np.inf, (a & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    return {"d2": out_d, "ids": out_i, "cuts": cuts, "end_cut": end_cut, "tie_cut": bool(tie), "lens": lens}


# ---- the data -------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def _shuffled(rng, counts):
    """img [n]: image g on counts[g] rows, in random order (no image's rows are contiguous)."""
    return rng.permutation(np.repeat(np.arange(len(counts), dtype=np.int32), counts)).astype(np.int32)


def _near(rng, R, nq, noise=0.2):
    d = R.shape[1]
    return _unit(R[rng.integers(0, len(R), nq)] + (noise / np.sqrt(d)) * rng.standard_normal((nq, d)).astype(np.float32))


def _pad(lists, M=None):
    M = max(len(x) for x in lists) if M is None else M
    out = np.full((len(lists), M), -1, np.int32)
    for b, x in enumerate(lists):
        out[b, :len(x)] = x
    return out


def _data(d, R, img, Q, qoff, sl, splits=None):
    qoff = np.asarray(qoff, np.int32)
    assert Q.shape == (qoff[-1], d) and R.shape == (len(img), d) and sl.shape[0] == len(qoff) - 1 and len(R) <= 32768
    return {"d": d, "R": R, "img": np.asarray(img, np.int32), "Q": Q, "qoff": qoff, "sl": np.ascontiguousarray(sl, np.int32),
            "splits": splits or [(0, len(R))]}


def _plain(name, d, counts, q_rows, lists, splits=None, M=None):
    rng = _rng(name)
    img = _shuffled(rng, counts)
    R = _unit(rng.standard_normal((len(img), d)).astype(np.float32))
    qoff = np.concatenate([[0], np.cumsum(q_rows)])
    return _data(d, R, img, _near(rng, R, int(qoff[-1])), qoff, _pad(lists, M), splits)


def _mt1(name):
    # rows 1 | 31 | 32 | 17: every group <= 32 rows.  Unions of 257 rows (tiles of 128, 128, 1), 257, 129 and 128
    return _plain(name, 32, [128, 1, 128, 100, 29, 60], [1, 31, 32, 17], [[0, 2, 1], [3, 4, 0], [0, 1], [2]])


def _mt2(name):
    # rows 33 | 64 | 65 (groups of 32 and 33) | 1
    return _plain(name, 32, [50] * 6, [33, 64, 65, 1], [[0, 1, 2], [5, 3], [0, 1, 2, 3, 4, 5], [4, 1, 0]])


def _width(name, d):
    return _plain(name, d, [40] * 8, [40, 20], [[1, 3, 4, 6], [0, 7, 3]])


def _s1(name):
    # 1536 one-row query images: one group each, S = 1.  Unions of 10 x 103 = 1030 rows (nine tiles: the buffer is cut after the
    # eighth), but image 5's (one row: the final kernel sorts nothing) and image 9's (empty)
    rng = _rng(name)
    counts = [103] * 40 + [1, 0, 30]
    img = _shuffled(rng, counts)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    sl = np.stack([rng.permutation(40)[:10] for _ in range(1536)]).astype(np.int32)
    sl[5] = -1
    sl[5, 3] = 40
    sl[9] = -1
    return _data(32, R, img, _near(rng, R, 1536), np.arange(1537), sl)


def _s6(name):
    # 300 groups: S = ceil(1536 / 300) = 6; unions of 800 rows are seven tiles, slice 0 takes two
    rng = _rng(name)
    img = _shuffled(rng, [80] * 20)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    sl = np.stack([rng.permutation(20)[:10] for _ in range(300)]).astype(np.int32)
    return _data(32, R, img, _near(rng, R, 600), np.arange(0, 601, 2), sl)


def _mem(name):
    # 12800 query rows: eight slices of 1024-key buffers would be 800 MB -- S = 5.  Unions of 100 rows: slices 1 .. 4 get no tile
    rng = _rng(name)
    img = _shuffled(rng, [25] * 10)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    sl = np.stack([rng.permutation(10)[:4] for _ in range(200)]).astype(np.int32)
    return _data(32, R, img, _near(rng, R, 12800), np.arange(0, 12801, 64), sl)


CUTS_LISTED, CUTS_PER = 249, 100


def _cuts(name, ties):
    """Two query images of 40 rows around one centre c.  The 249 listed reference images (even ids, 100 rows each) hold rows
    c + s g with s falling from 1 to 0.02 along the image ids: union positions ascend from far to near, every later tile passes
    the threshold the last cut has set, and a slice's buffer fills again and again.  40 unlisted images (odd ids) hold rows nearer
    than any listed one.  Image 1's shortlist leaves ten listed images out.
    ties: 512 exact copies of one row nearer to every query than all others: 13 in each of slice 0's tiles of image 0's union
    (more than k in ONE slice's buffer: its cuts fall inside the run), 200 anywhere else."""
    rng = _rng(name)
    d, nl = 32, CUTS_LISTED * CUTS_PER
    c = _unit(rng.standard_normal((1, d)).astype(np.float32))
    img = np.concatenate([np.repeat(2 * np.arange(CUTS_LISTED), CUTS_PER), np.repeat(2 * np.arange(40) + 1, 50)]).astype(np.int32)
    s = np.concatenate([0.02 ** (np.arange(nl) / nl), np.full(2000, 0.001)]).astype(np.float32)
    R = _unit(c + s[:, None] * rng.standard_normal((len(img), d)).astype(np.float32) / np.float32(np.sqrt(d)))
    order = rng.permutation(len(img))
    R, img = R[order], img[order]
    Q = _unit(c + np.float32(0.002 / np.sqrt(d)) * rng.standard_normal((80, d)).astype(np.float32))
    listed = 2 * np.arange(CUTS_LISTED, dtype=np.int32)
    sl = _pad([listed, np.delete(listed, [3, 50, 51, 120, 121, 122, 200, 230, 240, 248])])
    if ties:
        u = union_rows(img, sl[0])
        copy = _unit(c + np.float32(0.0005 / np.sqrt(d)) * rng.standard_normal((1, d)).astype(np.float32))
        tiles = np.arange(0, -(-len(u) // TILE), SL_SLICES_MAX)               # slice 0's tiles at S = 8
        at = np.concatenate([t * TILE + rng.permutation(min(TILE, len(u) - t * TILE))[:13] for t in tiles])
        rest = np.setdiff1d(np.arange(len(u)), at)
        at = np.concatenate([at, rng.permutation(rest)[:200]])
        R[u[at]] = copy
    return _data(d, R, img, Q, [0, 40, 80], sl)


def _k1024(name, U_images):
    rng = _rng(name)
    img = _shuffled(rng, [100] * U_images + [50] * 10)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    q_rows = [10, 3] if U_images < 11 else [20, 20]
    qoff = np.concatenate([[0], np.cumsum(q_rows)])
    sl = _pad([np.arange(U_images), np.arange(U_images)[::-1][:max(U_images - 1, 1)]])
    return _data(32, R, img, _near(rng, R, int(qoff[-1])), qoff, sl)


LARGE_A, LARGE_B = 7, 20            # the reference images of 4097 and 9000 rows
LARGE_PAIRS = 6                     # exact duplicate pairs planted inside each of them


def _large(name):
    """Images 7 (4097 rows) and 20 (9000 rows) among 30 images of 20 rows (ids 0 .. 39, eight of them without rows), all rows
    shuffled together, in three db_add calls.  Inside each large image six rows are exact copies of six others, and the first
    query rows of the images 0 and 1 are copies of them too: their nearest row is a tie that the id -- in segvlad_match_pairs the
    POSITION in the map -- decides."""
    rng = _rng(name)
    counts = np.zeros(40, np.int64)
    small = np.setdiff1d(np.arange(40), [LARGE_A, LARGE_B, 0, 9, 15, 16, 28, 33, 35, 36])
    assert len(small) == 30
    counts[small], counts[LARGE_A], counts[LARGE_B] = 20, SL_SORT_CAP + 1, 9000
    img = _shuffled(rng, counts)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    Q = _near(rng, R, 80)
    for j, g in enumerate((LARGE_A, LARGE_B)):
        own = np.nonzero(img == g)[0]
        pick = rng.permutation(len(own))[:2 * LARGE_PAIRS]
        first, second = own[pick[:LARGE_PAIRS]], own[pick[LARGE_PAIRS:]]
        second[0] = own[own > first[0]][0]                                    # (one pair of neighbours in the map)
        R[second] = R[first]
        Q[20 * j:20 * j + LARGE_PAIRS] = R[first]
        Q[20 * (1 - j) + 10:20 * (1 - j) + 10 + LARGE_PAIRS] = R[first]
    assert len(img) % 256 != 0
    sl = _pad([[LARGE_A], [LARGE_B], [LARGE_A, 3, 11], [LARGE_B, 5, 30]])
    return _data(32, R, img, Q, [0, 20, 40, 60, 80], sl, [(0, 5000), (5000, 9001), (9001, len(img))])


def _many(name):
    # 2500 reference images of 0 .. 3 rows: the scan gives every thread three images; ids without rows everywhere
    rng = _rng(name)
    counts = rng.integers(0, 4, 2500)
    counts[2499], counts[0] = 2, 0
    img = _shuffled(rng, counts)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    sl = rng.integers(0, 2500, (2, 200)).astype(np.int32)
    sl[0, :3] = (2499, 0, 2499)
    n = len(img)
    return _data(32, R, img, _near(rng, R, 20), [0, 10, 20], sl, [(0, 1000), (1000, 1001), (1001, n)])


def _union_edge(name, M):
    # 30 reference image ids, ten of them without rows, 10 rows each
    rng = _rng(name)
    counts = np.full(30, 10)
    counts[[0, 3, 4, 11, 12, 13, 20, 27, 28, 29]] = 0
    counts[29] = 10
    img = _shuffled(rng, counts)
    R = _unit(rng.standard_normal((len(img), 32)).astype(np.float32))
    if M == 1:
        sl = np.array([[4], [-1], [29], [5]], np.int32)                      # an id without rows; nothing; the last id; (no query rows)
    elif M == 65:
        sl = rng.integers(-1, 30, (4, 65)).astype(np.int32)
    else:
        few = np.array([2, 5, 6, 7, 9, 14, 21, 22, 25, 29, 3, 12, -1, -1], np.int32)     # ten with rows, two without, -1
        sl = few[rng.integers(0, len(few), (4, 4096))]
        sl[3] = -1
        sl[3, 4095] = 6
    return _data(32, R, img, _near(rng, R, 46), [0, 5, 6, 46, 46], sl)


DATA = {
    "mt1": _mt1, "mt2": _mt2, "d96": lambda n: _width(n, 96), "d160": lambda n: _width(n, 160), "s1": _s1, "s6": _s6, "mem": _mem,
    "cuts": lambda n: _cuts(n, False), "ties": lambda n: _cuts(n, True), "k1024-short": lambda n: _k1024(n, 7),
    "k1024-cuts": lambda n: _k1024(n, 175), "large": _large, "many": _many, "m1": lambda n: _union_edge(n, 1),
    "m65": lambda n: _union_edge(n, 65), "m4096": lambda n: _union_edge(n, 4096),
}


@functools.lru_cache(maxsize=None)
def make_data(name):
    """The named data (a dict: d, R, img, splits, Q, qoff, sl), built once per process; nobody writes to it."""
    x = DATA[name](name)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def unions(name):
    """union_d2() of the named data: shared by the cases on the same data, the replay and the brute force."""
    x = make_data(name)
    return union_d2(x["Q"], x["R"], x["img"], x["qoff"], x["sl"])


# ---- the table ------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name data k q_offset reaches")

CASES = [
    Case("mt1-rows-1-31-32", "mt1", 10, 0, "MT = 1: sl_gemm_kernel<1, false>, its key block and ballot append at 32 rows; tile edges 128 | 129 | 257"),
    Case("mt2-rows-33-64-65-1", "mt2", 20, 0, "MT = 2 with a one-row group and a 32 + 33 split beside it"),
    Case("d96", "d96", 20, 0, "three k-tiles: an odd count"),
    Case("d160-view-off-16-bytes", "d160", 20, 1, "five k-tiles; sv_aligned_queries copies the view, the norms are the aligned form's"),
    Case("s1-1536-one-row-images", "s1", 10, 0, "S = 1: a mid-loop cut, the final kernel's no-sort path (one key; none)"),
    Case("s6-300-groups", "s6", 10, 0, "S = 6: np2 = 64 > S k = 60"),
    Case("s5-by-memory-12800-rows", "mem", 10, 0, "S lowered 8 -> 5 by the 512 MB rule; slices without a tile"),
    Case("cuts-k256", "cuts", 256, 0, ">= 3 mid-loop cuts of every (row, slice) at cap = 1024"),
    Case("cuts-k257", "cuts", 257, 0, "cap = 2048 on the same data: one mid-loop cut of every (row, slice)"),
    Case("ties-k256", "ties", 256, 0, "cuts inside a run of equal distances; ties across slices; ids decide"),
    Case("k1024-union-of-700", "k1024-short", 1024, 0, "padding behind U < k; the final sort's 64 KiB of LDS"),
    Case("k1024-union-of-17500", "k1024-cuts", 1024, 0, "cap = 2048 mid-loop cuts at k = 1024; S k = 8192 exactly"),
    Case("large-images-4097-9000", "large", 50, 0, "the map's ordered scan: 4097 and 9000 rows, three adds, n % 256 != 0"),
    Case("many-images-0-to-3-rows", "many", 20, 0, "scan per = 3; images of <= 1 row return early; the two-element sort"),
    Case("m1", "m1", 5, 0, "M = 1: np2m = 64, 192 threads own nothing"),
    Case("m65", "m65", 5, 0, "M = 65: np2m = 128, 128 threads own nothing"),
    Case("m4096", "m4096", 5, 0, "M = 4096: sixteen ids per thread, duplicates, -1, ids without rows"),
]
assert len({c.name for c in CASES}) == len(CASES) and all(c.data in DATA for c in CASES)
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def plan(case):
    x = make_data(case.data)
    return plan_of(x["img"], x["qoff"], x["sl"], case.k, x["d"])


def simulate(case, d2, ids):
    """The replay of one query row of `case` over its union (d2, ids in union order): see replay()."""
    p = plan(case)
    return replay(p["S"], p["cap"], case.k, d2, ids)


def brute(case):
    x = make_data(case.data)
    return rank(unions(case.data), x["Q"].shape[0], x["qoff"], case.k)
