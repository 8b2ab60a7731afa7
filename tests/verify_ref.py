"""Host reference of segvlad_verify_pairs: a literal NumPy float64 restatement of the contract in include/segvlad.h.  NumPy
rounds every elementwise operation on its own and never fuses a multiplication with an addition, so each decision below is the
one the header prescribes.  `verify_slot` works on one slot's correspondences, `verify_pairs` on the arguments of the entry
point; `verify_slot_complex` is an independent formulation (complex division, |a (p - p_i) - (s - s_i)| < tol) that agrees with
the first wherever no decision sits on a rounding boundary -- integer coordinates, for instance."""
import numpy as np


def correspondences(q_xy, r_xy, rows, fwd, mut):
    """The query rows among `rows` (ascending) that are correspondences of a slot column: mutual != 0, 0 <= fwd < n_r, four
    finite coordinates.  Returns (the rows, p [M][2], s [M][2])."""
    keep = []
    for q, f, m in zip(rows, fwd, mut):
        if m != 0 and 0 <= f < len(r_xy) and np.isfinite(q_xy[q]).all() and np.isfinite(r_xy[f]).all():
            keep.append((q, f))
    qs = np.array([k[0] for k in keep], np.int64)
    fs = np.array([k[1] for k in keep], np.int64)
    return qs, q_xy[qs].reshape(-1, 2), r_xy[fs].reshape(-1, 2)


def verify_slot(p, s, tol, min_scale, max_scale):
    """p, s float64 [M][2].  Returns (count, i, j, flags [M] uint8, model [4]); (0, -1, -1, zeros, NaN) without a winner."""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    s = np.asarray(s, np.float64).reshape(-1, 2)
    M = len(p)
    tol2 = np.float64(tol) * np.float64(tol)
    lo = np.float64(min_scale) * np.float64(min_scale)
    hi = np.float64(max_scale) * np.float64(max_scale)
    best = None
    with np.errstate(all="ignore"):
        for i in range(M - 1):
            # every hypothesis (i, j), j = i + 1 .. M - 1, at once: one row of the arrays per j
            dx, dy = p[i + 1:, 0] - p[i, 0], p[i + 1:, 1] - p[i, 1]
            ex, ey = s[i + 1:, 0] - s[i, 0], s[i + 1:, 1] - s[i, 1]
            n, m = dx * dx + dy * dy, ex * ex + ey * ey
            ar, ai = ex * dx + ey * dy, ey * dx - ex * dy
            ok = (n > 0) & (lo * n <= m) & (m <= hi * n)
            px, py = p[:, 0] - p[i, 0], p[:, 1] - p[i, 1]
            sx, sy = s[:, 0] - s[i, 0], s[:, 1] - s[i, 1]
            ux = (ar[:, None] * px[None, :] - ai[:, None] * py[None, :]) - n[:, None] * sx[None, :]
            uy = (ar[:, None] * py[None, :] + ai[:, None] * px[None, :]) - n[:, None] * sy[None, :]
            inl = ux * ux + uy * uy < ((tol2 * n) * n)[:, None]
            cnt = inl.sum(axis=1)
            for r in np.nonzero(ok)[0]:                                  # ascending j: ascending h
                if best is None or cnt[r] > best[0]:
                    best = (int(cnt[r]), i, i + 1 + int(r), inl[r].astype(np.uint8), float(ar[r]), float(ai[r]), float(n[r]))
        if best is None:
            return 0, -1, -1, np.zeros(M, np.uint8), np.full(4, np.nan)
        cnt, i, j, flags, ar, ai, n = best
        are, aim = np.float64(ar) / np.float64(n), np.float64(ai) / np.float64(n)
        model = np.array([are, aim, s[i, 0] - (are * p[i, 0] - aim * p[i, 1]), s[i, 1] - (are * p[i, 1] + aim * p[i, 0])])
    return cnt, i, j, flags, model


def verify_slot_complex(p, s, tol, min_scale, max_scale):
    """The same question asked the textbook way: a = ds / dp, scale bounds on |a|, residual |a (p - p_i) - (s - s_i)| < tol."""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    s = np.asarray(s, np.float64).reshape(-1, 2)
    pc, sc = p[:, 0] + 1j * p[:, 1], s[:, 0] + 1j * s[:, 1]
    best = (0, -1, -1, np.zeros(len(p), np.uint8))
    found = False
    for i in range(len(p)):
        for j in range(i + 1, len(p)):
            dp, ds = pc[j] - pc[i], sc[j] - sc[i]
            if dp == 0:
                continue
            a = ds / dp
            if not min_scale <= abs(a) <= max_scale:
                continue
            inl = np.abs(a * (pc - pc[i]) - (sc - sc[i])) < tol
            if not found or inl.sum() > best[0]:
                best, found = (int(inl.sum()), i, j, inl.astype(np.uint8)), True
    return best


def verify_pairs(q_xy, r_xy, qoff, fwd_idx, mutual, tol, min_scale=0.5, max_scale=2.0):
    """The outputs of segvlad_verify_pairs as NumPy arrays: n_inlier, pair, model, order, inlier."""
    q_xy = np.asarray(q_xy, np.float64).reshape(-1, 2)
    r_xy = np.asarray(r_xy, np.float64).reshape(-1, 2)
    fwd_idx, mutual = np.asarray(fwd_idx), np.asarray(mutual)
    n_img, (nq, C) = len(qoff) - 1, fwd_idx.shape
    out = {"n_inlier": np.zeros((n_img, C), np.int32), "pair": np.full((n_img, C, 2), -1, np.int32),
           "model": np.full((n_img, C, 4), np.nan), "order": np.zeros((n_img, C), np.int32), "inlier": np.zeros((nq, C), np.uint8)}
    for b in range(n_img):
        rows = np.arange(qoff[b], qoff[b + 1])
        for j in range(C):
            qs, p, s = correspondences(q_xy, r_xy, rows, fwd_idx[rows, j], mutual[rows, j])
            cnt, i, jj, flags, model = verify_slot(p, s, tol, min_scale, max_scale)
            out["n_inlier"][b, j] = cnt
            if i >= 0:
                out["pair"][b, j] = (qs[i], qs[jj])
                out["inlier"][qs, j] = flags
            out["model"][b, j] = model
        out["order"][b] = sorted(range(C), key=lambda j: (-int(out["n_inlier"][b, j]), j))
    return out
