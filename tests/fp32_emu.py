"""Host emulation of the DEVICE's documented fp32 arithmetic for one exact squared distance (test infrastructure; VERDICT r05
next #7): with it a kNN id comparison needs no "near-tie" allowance -- the device's (distance, id) lists must equal the emulated
ones bit for bit, ties included.

What the device computes for a (query q, database row r) pair on EVERY exact path (distance-matrix GEMM gemm_nt_kernel<1>,
refine_exact_*, refine_group_gemm_kernel, small_tail_kernel):

    dot   = the sequential chain  acc = fmaf(q[j], r[j], acc),  j = 0 .. d-1,  acc = 0                 (one rounding per step)
            (gemm_nt_kernel's guarded loop pads a partial k-tile, and rows beyond the operand, with zeros: fmaf(0, 0, acc) = acc,
            so the chain is the same for every d, every tile position and every nq, whichever of the two main loops runs)
    ||x||^2 = row_sumsq (csrc/gemm_kernels.hip): lane L of a 64-lane wave sums the float4s L, L + 64, ... of the row with fmaf
              (x, y, z, w in turn), then the xor butterfly v += shfl_xor(v, o), o = 32, 16, 8, 4, 2, 1 -- when d % 4 == 0 AND
              the row starts on a 16-byte boundary; otherwise lane L sums the single elements L, L + 64, ... with fmaf, then
              the same butterfly.  Index rows are the library's own copy (16-byte aligned base): their form follows from d
              alone; a query view keeps its caller's alignment.
    d2    = fmaf(-2, dot, ||q||^2 + ||r||^2), negative values set to zero                                (csrc/ctx.h: sv_d2)

fp32 fma is emulated exactly in float64: the product of two fp32 numbers is exact in float64 (48 significant bits), the sum with
the fp32 addend is formed with an error-free TwoSum, and the ONE rounding to fp32 is decided from the pair (sum, error) -- the
double rounding of "round to float64, then to float32" differs from the true fma exactly when the float64 sum sits on an fp32
rounding boundary and the discarded error is not zero, which the pair resolves.  Everything is vectorised over pairs."""
import numpy as np


def fma32(a, b, c):
    """round_to_fp32(a * b + c) for fp32 arrays a, b, c (broadcasting), exactly."""
    a64, b64, c64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    p = a64 * b64                          # exact (24 + 24 bits)
    s = p + c64                            # rounded to 53 bits ...
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)      # ... with the rounding error recovered (TwoSum: s + err == p + c exactly)
    r = s.astype(np.float32)               # float64 -> float32, ties to even
    d = s - r.astype(np.float64)           # exact
    # s exactly on the midpoint of two adjacent fp32 values: |d| is half an ulp of the fp32 grid there.  Then the TRUE value
    # s + err is off the midpoint by err, and the nearest fp32 neighbour lies on err's side.
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(r, np.float32(np.inf))
        dn = np.nextafter(r, np.float32(-np.inf))
        half_up = (up.astype(np.float64) - r.astype(np.float64)) * 0.5
        half_dn = (r.astype(np.float64) - dn.astype(np.float64)) * 0.5
    tie_hi = (d > 0) & (d == half_up)      # s is the midpoint between r and up; ties-to-even chose r
    tie_lo = (d < 0) & (-d == half_dn)     # s is the midpoint between dn and r
    r = np.where(tie_hi & (err > 0), up, r)
    r = np.where(tie_lo & (err < 0), dn, r)
    return r.astype(np.float32)


def row_sumsq(X, aligned=True):
    """||row||^2 of every row of X [n, d] fp32 as csrc/gemm_kernels.hip: row_sumsq computes it.  aligned: the rows start on
    16-byte boundaries (then d % 4 == 0 takes the float4 form); False, or d % 4 != 0: the single-element form."""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    if d % 4 != 0 or not aligned:
        s = np.zeros((n, 64), np.float32)
        for j0 in range(0, d, 64):                   # lane L takes element j0 + L
            w = min(64, d - j0)
            v = X[:, j0:j0 + w]
            s[:, :w] = fma32(v, v, s[:, :w])
        for o in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, np.arange(64) ^ o]).astype(np.float32)
        return s[:, 0].copy()
    d4 = d // 4
    X4 = X.reshape(n, d4, 4)
    s = np.zeros((n, 64), np.float32)
    for j0 in range(0, d4, 64):                      # lane L takes float4 j0 + L
        w = min(64, d4 - j0)
        for c in range(4):
            v = X4[:, j0:j0 + w, c]
            s[:, :w] = fma32(v, v, s[:, :w])
    for o in (32, 16, 8, 4, 2, 1):                   # v += shfl_xor(v, o): every lane at once
        s = (s + s[:, np.arange(64) ^ o]).astype(np.float32)
    return s[:, 0].copy()


def dot_chain(q, R):
    """acc = fmaf(q[j], r[j], acc), j = 0 .. d-1, for every row r of R [n, d] against ONE query q [d] (or q [n, d] row-wise)."""
    R = np.ascontiguousarray(R, np.float32)
    q = np.asarray(q, np.float32)
    qq = np.broadcast_to(q, R.shape)
    acc = np.zeros(R.shape[0], np.float32)
    for j in range(R.shape[1]):
        acc = fma32(qq[:, j], R[:, j], acc)
    return acc


def d2(q2, r2, dot):
    """sv_d2: fmaf(-2, dot, q2 + r2) with negative results set to zero (faiss's clamp)."""
    v = fma32(np.float32(-2.0), dot, (np.asarray(q2, np.float32) + np.asarray(r2, np.float32)).astype(np.float32))
    return np.where(v < 0, np.float32(0), v).astype(np.float32)


def check_contested(Q, R, d2_dev, idx_dev, k, queries=None, margin=1e-3, tol64=4e-6, q_aligned=True):
    """The device's top-k lists of query rows `queries` (default: all) against the emulated fp32 reference, bit for bit and ties
    included, and the fp64 oracle beside it.  Q [nq, d], R [n, d]: fp32 torch tensors on the device; d2_dev [nq, k], idx_dev [nq, k]:
    the device's result.  The emulation runs on the CONTESTED rows only: per query every row whose distance by a plain fp32 GEMM
    (a tool of the test, not the product) lies within `margin` x max(1, k-th smallest) of the k-th smallest -- 100 x the worst fp32
    deviation at that magnitude, so no row outside the set can be in anybody's top k.  Every emulated distance of the result lies
    within tol64 x max(1, (||q||^2 + max ||r||^2) / 2) of the fp64 distance (tol64 itself for unit rows).
    q_aligned: the query view the device was handed starts on a 16-byte boundary (row_sumsq's form for the query norms).
    k > n: the first n slots are compared, every slot behind them must hold (+inf, -1).
    Returns (contested pairs, exact-tie neighbours among the results, worst |fp32 - fp64| relative to that scale)."""
    import torch

    nq, n = Q.shape[0], R.shape[0]
    k_all, k = k, min(k, n)
    queries = range(nq) if queries is None else [int(q) for q in queries]
    qsel = torch.as_tensor(list(queries), dtype=torch.int64, device=Q.device)
    Qs = Q[qsel]
    approx = (Qs * Qs).sum(1, keepdim=True) + (R * R).sum(1)[None, :] - 2.0 * (Qs @ R.T)
    kth = torch.kthvalue(approx, k, dim=1).values
    lim = kth + margin * torch.clamp(kth, min=1.0)
    Qn = Q.cpu().numpy()
    q2 = row_sumsq(Qn, aligned=q_aligned)
    dd, ii = d2_dev.cpu().numpy(), idx_dev.cpu().numpy()
    # every query's contested rows in ONE emulated chain (row-wise query operand)
    sel = [torch.nonzero(approx[j] <= lim[j]).flatten() for j in range(len(qsel))]
    for j, q in enumerate(queries):
        assert sel[j].numel() >= k, (q, sel[j].numel())
    ids_all = torch.cat(sel)
    rr_all = R[ids_all].cpu().numpy()
    owner = np.repeat(np.arange(len(sel)), [s.numel() for s in sel])
    qq_all = Qn[np.asarray(list(queries), np.int64)[owner]]
    dist_all = d2(q2[np.asarray(list(queries), np.int64)[owner]], row_sumsq(rr_all), dot_chain(qq_all, rr_all))
    ids_all = ids_all.cpu().numpy()
    n_contested, n_tie_pairs, worst64 = 0, 0, 0.0
    off = 0
    for j, q in enumerate(queries):
        cnt = sel[j].numel()
        ids, dist, rr = ids_all[off:off + cnt], dist_all[off:off + cnt], rr_all[off:off + cnt]
        off += cnt
        order = np.lexsort((ids, dist))[:k]                         # (distance, id): IndexFlatL2's order, ties to the lower id
        assert np.array_equal(ids[order], ii[q, :k]), (q, np.nonzero(ids[order] != ii[q, :k])[0][:5])
        assert np.array_equal(dist[order].view(np.uint32), dd[q, :k].view(np.uint32)), q
        assert (ii[q, k:] == -1).all() and np.isposinf(dd[q, k:]).all(), (q, k, k_all)
        n_contested += cnt
        n_tie_pairs += int((np.diff(dist[order]) == 0).sum())
        d64 = ((Qn[q].astype(np.float64)[None, :] - rr[order].astype(np.float64)) ** 2).sum(1)
        scale = max(1.0, (float(q2[q]) + float(row_sumsq(rr).max())) / 2.0)
        worst64 = max(worst64, float(np.abs(d64 - dist[order]).max()) / scale)
    assert worst64 < tol64, worst64
    return n_contested, n_tie_pairs, worst64
