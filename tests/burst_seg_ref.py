"""Burst discount over a segment's own tokens (options vlad_burst=<a>:<b>:<p> with vlad_burst_scope=segment, include/segvlad.h): the
definition restated in NumPy fp64, an fp32 restatement of the discount, and the references of tests/test_burst_seg_cases.py and
tests/test_gpu_burst_seg.py.  A plain module; burst_ref, soft_vlad_ref and describe_shape_cases are imported unchanged.

    U(s)    = the tokens of segment s after the neighbour union, (adj . inc) > 0
    g[s][n] = sum_{m in U(s)} sigmoid(a (2 <x^_n, x^_m> - 2) + b)          n in U(s), m = n included
    u[s][n] = g[s][n]^-p
    V[s][k] = sum_{n in U(s)} u[s][n] w[n][k] (x^_n - c_k)                 w: burst_ref.assign_weights (one-hot | softmax)
    out[s]  = L2(concat_k intra_norm(V[s][k]))                             soft_pooled: K sum u w x^ - (sum u w) sum_c c_c
"""
import functools

import numpy as np

import burst_ref as BR
import describe_shape_cases as T
import soft_vlad_ref as SR

EPS = BR.EPS
PARAMS = BR.PARAMS
ASSIGNS = BR.ASSIGNS
CASES = SR.CASES


def union(inc, adj):
    """U [S][N] bool: the incidence after the neighbour union (adj None: order 0)"""
    inc = np.asarray(inc, dtype=bool)
    S = inc.shape[0]
    return inc if adj is None else (np.asarray(adj, dtype=np.int64).reshape(S, S) @ inc.astype(np.int64)) > 0


def burst_seg(tok_dn, inc, adj, a, b, p):
    """(g [S][N], u [S][N]) of one image, fp64; both 0 outside U(s)"""
    U = union(inc, adj)
    xh = BR.normalised(tok_dn)
    z = float(a) * (2.0 * (xh @ xh.T) - 2.0) + float(b)
    sig = 1.0 / (1.0 + np.exp(-z))
    g = (U.astype(np.float64) @ sig) * U      # row s: the sum over the members m of U(s) (sig is symmetric), kept on U(s)
    for s in np.flatnonzero(U.all(1)):        # a segment of every token: burst_ref.burst's own row sum, addition for addition
        g[s] = sig.sum(1)
    u = np.zeros(U.shape)
    u[U] = g[U] ** (-float(p))
    return g, u


@functools.lru_cache(maxsize=None)
def _sigmoid_fp32(name, b, params):
    """The sigmoid matrix [N][N] of image b of a case with every operation in fp32 and sequential chains over d (burst_ref.burst_u_fp32's
    operations up to the sum over m)"""
    f = np.float32
    a, bb, _ = params
    X = np.ascontiguousarray(np.asarray(T.build(name)["toks"][b], dtype=f))                    # [D][N]
    D, N = X.shape
    ss = np.zeros(N, f)
    dot = np.zeros((N, N), f)
    for d in range(D):
        ss = ss + X[d] * X[d]
        dot = dot + X[d][:, None] * X[d][None, :]
    rn = f(1) / np.maximum(np.sqrt(ss), f(EPS))
    cos = (dot * rn[:, None]) * rn[None, :]
    z = f(a) * (f(2) * cos - f(2)) + f(bb)
    with np.errstate(over="ignore"):
        return f(1) / (f(1) + np.exp(-z, dtype=f))


def burst_seg_u_fp32(sig32, inc, adj, p):
    """u [S][N] from an fp32 sigmoid matrix [N][N] with the sum over the members m of U(s) a sequential fp32 chain, m = 0 .. N-1: the
    counterpart of burst_ref.burst_u_fp32.  Returned as fp64, 0 outside U(s)."""
    f = np.float32
    U = union(inc, adj)
    S, N = U.shape
    g = np.zeros((S, N), f)
    Uf, cols = U.astype(f), np.ascontiguousarray(sig32.T)
    for m in range(N):                        # (a non-member adds an exact 0)
        g = g + Uf[:, m][:, None] * cols[m][None, :]
    u = np.zeros((S, N))
    with np.errstate(divide="ignore"):
        u[U] = np.power(g[U], f(-p), dtype=f).astype(np.float64)
    return u


def weighted_seg_vlad(tok_dn, C, u, w, pooled=False):
    """burst_ref.weighted_vlad's loop with the real-valued mask u [S][N] (0 outside U(s)) in the place of the 0/1 union:
    dict(out [S][K D], block_norms [S][K]), fp64"""
    C = np.asarray(C, dtype=np.float64)
    K, D = C.shape
    S = u.shape[0]
    xh = BR.normalised(tok_dn)
    out = np.zeros((S, K, D))
    bn = np.zeros((S, K))
    for k in range(K):
        Uw = u * w[:, k][None, :]
        if pooled:
            V = K * (Uw @ xh) - Uw.sum(1)[:, None] * C.sum(0)[None, :]
        else:
            V = Uw @ xh - Uw.sum(1)[:, None] * C[k][None, :]
        bn[:, k] = np.sqrt((V * V).sum(1))
        out[:, k] = V / np.maximum(bn[:, k], EPS)[:, None]
    out = out.reshape(S, K * D)
    out = out / np.maximum(np.sqrt((out * out).sum(1, keepdims=True)), EPS)
    return dict(out=out, block_norms=bn)


def seg_vlad(tok_dn, C, inc, adj, assign, params, u=None):
    """One image under vlad_assign=`assign`, vlad_burst=`params`, vlad_burst_scope=segment; u: the mask to use instead of the fp64 one"""
    w = BR.assign_weights(tok_dn, C, assign)
    if u is None:
        u = burst_seg(tok_dn, inc, adj, *params)[1]
    return weighted_seg_vlad(tok_dn, C, np.asarray(u, dtype=np.float64), w, pooled=assign[0] == "soft_pooled")


def batch(toks, incs, adjs, C, with_adj, assign, params, us=None):
    """seg_vlad per image (a repeated image -- the same arrays -- is computed once): dict(out, block_norms, zero_rows)"""
    outs, bns, zero, done = [], [], [], {}
    for b in range(len(toks)):
        key = (id(toks[b]), id(incs[b]))
        if key not in done:
            done[key] = seg_vlad(toks[b], C, incs[b], adjs[b] if with_adj else None, assign, params, None if us is None else us[b])
        outs.append(done[key]["out"]), bns.append(done[key]["block_norms"])
        zero.append(~union(incs[b], adjs[b] if with_adj else None).any(1))
    return dict(out=np.concatenate(outs), block_norms=np.concatenate(bns), zero_rows=np.concatenate(zero))


@functools.lru_cache(maxsize=None)
def reference(name, with_adj, assign, params):
    """The fp64 definition on a case of the shape table, computed once per process and never written to"""
    d = T.build(name)
    return batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj, assign, params)


@functools.lru_cache(maxsize=None)
def case_u_fp32(name, with_adj, params):
    """The fp32 restatement's u [S_b][N] of every image of a case (image 3 is image 0)"""
    d = T.build(name)
    us = [burst_seg_u_fp32(_sigmoid_fp32(name, b, params), d["incs"][b], d["adjs"][b] if with_adj else None, params[2]) for b in range(3)]
    return us + [us[0]]


@functools.lru_cache(maxsize=None)
def e_u_seg(name, assign, params, with_adj=True):
    """e_u_seg(case): max |fp64 descriptor - fp64 descriptor with the fp32 restatement's u in the place of its own|"""
    d = T.build(name)
    alt = batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj, assign, params, us=case_u_fp32(name, with_adj, params))
    return float(np.abs(alt["out"] - reference(name, with_adj, assign, params)["out"]).max())


def union_sizes(name, with_adj):
    """|U(s)| of every segment of a case's batch, [S_tot]"""
    d = T.build(name)
    return np.concatenate([union(d["incs"][b], d["adjs"][b] if with_adj else None).sum(1) for b in range(T.B)])
