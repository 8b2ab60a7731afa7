"""Burst-discounted VLAD (option vlad_burst=<a>:<b>:<p>, include/segvlad.h): the definition restated in NumPy fp64, an fp32
restatement of the discount, and the case builders of tests/test_burst_cases.py and tests/test_gpu_burst.py.  A plain module.

    g[n]    = sum_{m < N} sigmoid(a (2 <x^_n, x^_m> - 2) + b)          over ALL tokens of the image, m = n included
    u[n]    = g[n]^-p
    w[n][k] = u[n] [k = label(n)]                 (vlad_assign=hard: the cosine arg-max)
            = u[n] softmax_k(T <x^_n, c^_k>)      (soft:<T>, soft_pooled:<T>)
    V, intra-normalisation, row L2: tests/soft_vlad_ref.py's loop with these weights.

The shape table is soft_vlad_ref.CASES (describe_shape_cases' inputs, imported unchanged).  The probe table reaches the Gram
kernel's tile edges through an existing output: every token is covered by exactly one single-token segment, so under hard
assignment block_norms[s][label] = u[n] ||x^_n - c_label|| and the other block is exactly 0.
"""
import functools

import numpy as np

import describe_shape_cases as T
import soft_vlad_ref as SR

EPS = 1e-12
PARAMS = ((8.0, 7.0, 1.0), (2.0, 0.0, 0.5))
ASSIGNS = (("hard", None), ("soft", 10.0), ("soft_pooled", 10.0))
CASES = SR.CASES


def normalised(tok_dn):
    X = np.asarray(tok_dn, dtype=np.float64).T
    return X / np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), EPS)


def burst(tok_dn, a, b, p):
    """(g [N], u [N]) of one image, fp64"""
    xh = normalised(tok_dn)
    z = float(a) * (2.0 * (xh @ xh.T) - 2.0) + float(b)
    g = (1.0 / (1.0 + np.exp(-z))).sum(1)
    return g, g ** (-float(p))


def burst_u_fp32(tok_dn, a, b, p):
    """u [N] with every operation in fp32 and sequential chains: the dot products over d = 0 .. D-1, the sum over m = 0 .. N-1.
    (Raw dot product times the two 1 / max(||x||, 1e-12), the sigmoid as 1 / (1 + exp(-z)): the operations the device performs,
    in the plainest order.)"""
    f = np.float32
    X = np.ascontiguousarray(np.asarray(tok_dn, dtype=f))                    # [D][N]
    D, N = X.shape
    ss = np.zeros(N, f)
    dot = np.zeros((N, N), f)
    for d in range(D):
        ss = ss + X[d] * X[d]
        dot = dot + X[d][:, None] * X[d][None, :]
    rn = f(1) / np.maximum(np.sqrt(ss), f(EPS))
    cos = (dot * rn[:, None]) * rn[None, :]
    z = f(a) * (f(2) * cos - f(2)) + f(b)
    with np.errstate(over="ignore"):
        s = f(1) / (f(1) + np.exp(-z, dtype=f))
    g = np.zeros(N, f)
    for m in range(N):
        g = g + s[:, m]
    return np.power(g, f(-p), dtype=f).astype(np.float64)


def assign_weights(tok_dn, C, assign):
    """w [N][K] before the discount: the one-hot of the cosine arg-max (first maximum), or soft_vlad_ref.weights"""
    mode, temp = assign
    if mode != "hard":
        return SR.weights(tok_dn, C, temp)[0]
    C = np.asarray(C, dtype=np.float64)
    ch = C / np.maximum(np.sqrt((C * C).sum(1, keepdims=True)), EPS)
    lab = np.argmax(normalised(tok_dn) @ ch.T, axis=1)
    w = np.zeros((lab.size, C.shape[0]))
    w[np.arange(lab.size), lab] = 1.0
    return w


def weighted_vlad(tok_dn, C, inc, adj, w, pooled=False):
    """soft_vlad_ref.soft_vlad's loop over given weights w [N][K]: dict(out [S][K D], block_norms [S][K]), fp64"""
    C = np.asarray(C, dtype=np.float64)
    K, D = C.shape
    inc = np.asarray(inc, dtype=bool)
    S = inc.shape[0]
    xh = normalised(tok_dn)
    U = inc if adj is None else (np.asarray(adj, dtype=np.int64).reshape(S, S) @ inc.astype(np.int64)) > 0
    Uf = U.astype(np.float64)
    out = np.zeros((S, K, D))
    bn = np.zeros((S, K))
    for k in range(K):
        Uw = Uf * w[:, k][None, :]
        if pooled:
            V = K * (Uw @ xh) - Uw.sum(1)[:, None] * C.sum(0)[None, :]
        else:
            V = Uw @ xh - Uw.sum(1)[:, None] * C[k][None, :]
        bn[:, k] = np.sqrt((V * V).sum(1))
        out[:, k] = V / np.maximum(bn[:, k], EPS)[:, None]
    out = out.reshape(S, K * D)
    out = out / np.maximum(np.sqrt((out * out).sum(1, keepdims=True)), EPS)
    return dict(out=out, block_norms=bn)


def burst_vlad(tok_dn, C, inc, adj, assign, params, u=None):
    """One image under vlad_assign=`assign` and vlad_burst=`params` (None: off); u: the discount to use instead of the fp64 one"""
    w = assign_weights(tok_dn, C, assign)
    if params is not None:
        w = w * (burst(tok_dn, *params)[1] if u is None else np.asarray(u, dtype=np.float64))[:, None]
    return weighted_vlad(tok_dn, C, inc, adj, w, pooled=assign[0] == "soft_pooled")


def batch(toks, incs, adjs, C, with_adj, assign, params, us=None):
    """burst_vlad per image (a repeated image -- the same arrays -- is computed once): dict(out, block_norms, zero_rows)"""
    outs, bns, zero, done = [], [], [], {}
    for b in range(len(toks)):
        key = id(toks[b])
        if key not in done:
            done[key] = burst_vlad(toks[b], C, incs[b], adjs[b] if with_adj else None, assign, params, None if us is None else us[b])
        union = incs[b] if not with_adj else (np.asarray(adjs[b]).astype(np.int64) @ incs[b].astype(np.int64)) > 0
        outs.append(done[key]["out"]), bns.append(done[key]["block_norms"]), zero.append(~union.any(1))
    return dict(out=np.concatenate(outs), block_norms=np.concatenate(bns), zero_rows=np.concatenate(zero))


@functools.lru_cache(maxsize=None)
def reference(name, with_adj, assign, params):
    """The fp64 definition on a case of the shape table, computed once per process and never written to"""
    d = T.build(name)
    return batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj, assign, params)


@functools.lru_cache(maxsize=None)
def case_u_fp32(name, params):
    """The fp32 restatement's u of every image of a case (image 3 is image 0)"""
    d = T.build(name)
    us = [burst_u_fp32(t, *params) for t in d["toks"][:3]]
    return us + [us[0]]


@functools.lru_cache(maxsize=None)
def e_u(name, with_adj, assign, params):
    """E_u(case): max |fp64 descriptor - fp64 descriptor with the fp32 restatement's u in the place of its own|"""
    d = T.build(name)
    alt = batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj, assign, params, us=case_u_fp32(name, params))
    return float(np.abs(alt["out"] - reference(name, with_adj, assign, params)["out"]).max())


def weight_rtol(D, params, temp=0.0):
    """Relative bound on a discounted weight in fp32: |dg| <= g max|dz| (sigmoid' <= sigmoid), |dz| = 2 a |dcos|, u = g^-p, and an
    fp32 D-term dot product of unit vectors is off by sqrt(D) 2^-24 (the bound of tests/test_gpu_soft_vlad.py's 2 T sqrt(D) 2^-24)"""
    a, _, p = params
    return 1e-5 + 2.0 * (p * a + temp) * np.sqrt(D) * 2.0 ** -24


# ---- the probe table: the Gram kernel's edges through block_norms ---------------------------------------------------------------
PROBE_K = 2
PROBE_SEGS = 400        # single-token segments per copy of the image (k32_d32_n1530_s400's S_max: prep_kernel's LDS holds it)
PROBES = [(N, D) for N in (33, 63, 64, 65, 127, 129, 257) for D in (32, 36, 200)] + [(130, 1536), (1530, 32)]


def probe_id(nd):
    return f"n{nd[0]}_d{nd[1]}"


@functools.lru_cache(maxsize=None)
def probe(N, D):
    """One image of N tokens around K = 2 centres, every column scaled by a factor in [0.5, 2] (the kernels normalise), repeated
    ceil(N / 400) times; copy c holds the single-token segments of tokens 400 c .. 400 c + 399, in token order."""
    from revisit_anything_amd import synth

    seed = 9100 + 7 * N + D
    C = synth.make_vocab(PROBE_K, D, seed=seed)
    t = synth.make_tokens(C, N, seed=seed + 1, noise=0.02 if D > 256 else 0.05)
    t = np.ascontiguousarray(t * np.random.Generator(np.random.PCG64(seed + 2)).uniform(0.5, 2.0, N).astype(np.float32)[None, :])
    copies = (N + PROBE_SEGS - 1) // PROBE_SEGS
    eye = np.eye(N, dtype=bool)
    incs = [eye[PROBE_SEGS * c:min(N, PROBE_SEGS * (c + 1))] for c in range(copies)]
    toks = [t] * copies
    tok, bits, offs, _ = T.pack_batch(toks, incs, [np.zeros((0, 0), np.uint8)] * copies)
    return dict(K=PROBE_K, D=D, N=N, C=C, t=t, tok=tok, bits=bits, offs=offs)


def probe_gap(N, D):
    """The top-2 cosine gap of every probe token (fp64)"""
    d = probe(N, D)
    C = d["C"].astype(np.float64)
    s = np.sort(normalised(d["t"]) @ (C / np.sqrt((C * C).sum(1, keepdims=True))).T, axis=1)
    return s[:, -1] - s[:, -2]


def probe_block_norms(N, D, params):
    """[N][2] fp64: u[n] ||x^_n - c_label|| in the label's column, exactly 0 in the other (segment n = token n)"""
    d = probe(N, D)
    w = assign_weights(d["t"], d["C"], ("hard", None))
    res = np.sqrt(((normalised(d["t"])[:, None, :] - d["C"].astype(np.float64)[None]) ** 2).sum(2))     # [N][K]
    return w * res * burst(d["t"], *params)[1][:, None]
