"""The contract of segvlad_match_pairs on the host, for the tests that hold the device against it (tests/test_gpu_match.py, and
tests/test_gpu_shortlist_cases.py for the image -> row map's large images): existing code plus tests/fp32_emu.py, never the code
under test.  Per slot the full A x B matrix of the device's exact fp32 chain, the row minima by (d2, row id), the column minima by
(d2, query row), a pair mutual when the two name each other and d2 < max_d2, the scores (double)(2.0f - d2) added in fp64 in
query-row order."""
import numpy as np

import fp32_emu as E


def _yardstick(Q, R, img, qoff, cand, max_d2):
    """The contract of segvlad_match_pairs on the host (see the module docstring)."""
    qn, rn = E.row_sumsq(Q), E.row_sumsq(R)
    nq, (n_img, C) = Q.shape[0], cand.shape
    n_mut = np.zeros((n_img, C), np.int32)
    score = np.zeros((n_img, C), np.float64)
    order = np.zeros((n_img, C), np.int32)
    fwd_idx = np.full((nq, C), -1, np.int64)
    fwd_d2 = np.full((nq, C), np.inf, np.float32)
    mutual = np.zeros((nq, C), np.uint8)
    lim = np.float32(max_d2)
    for b in range(n_img):
        A = np.arange(qoff[b], qoff[b + 1])
        live = []
        for j in range(C):
            B = np.nonzero(img == cand[b, j])[0] if cand[b, j] >= 0 else np.zeros(0, np.int64)
            live.append(len(B) > 0)
            if not len(A) or not len(B):
                continue
            qi, ri = np.repeat(A, len(B)), np.tile(B, len(A))
            D = E.d2(qn[qi], rn[ri], E.dot_chain(Q[qi], R[ri])).reshape(len(A), len(B))
            assert not np.isnan(D).any()
            f = np.array([np.lexsort((B, D[a]))[0] for a in range(len(A))])       # (d2, row id)
            bw = np.array([np.lexsort((A, D[:, c]))[0] for c in range(len(B))])   # (d2, query row index)
            s = 0.0
            for a in range(len(A)):
                dd = D[a, f[a]]
                fwd_idx[A[a], j], fwd_d2[A[a], j] = B[f[a]], dd
                if bw[f[a]] == a and dd < lim:
                    mutual[A[a], j] = 1
                    n_mut[b, j] += 1
                    s += float(np.float32(2.0) - dd)
            score[b, j] = s
        order[b] = sorted(range(C), key=lambda j: (0, -int(n_mut[b, j]), -score[b, j], j) if live[j] else (1, 0, 0.0, j))
    return {"n_mutual": n_mut, "score": score, "order": order, "fwd_idx": fwd_idx, "fwd_d2": fwd_d2, "mutual": mutual}
