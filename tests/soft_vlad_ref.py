"""Soft-assignment VLAD (option vlad_assign=soft:<T> | soft_pooled:<T>, include/segvlad.h; utilities.py:862-887): the definition restated in NumPy
fp64, cluster by cluster, and the case builders of tests/test_soft_vlad.py and tests/test_gpu_soft_vlad*.py.  A plain module.

    w[n][k] = softmax over the K centres of T <x^_n, c^_k>                              (max-subtracted)
    V[s][k] = sum_{n in U(s)} w[n][k] x^_n - (sum_{n in U(s)} w[n][k]) c_k              U(s): the neighbour union's tokens
    out[s]  = L2(concat_k intra_norm(V[s][k]))                                          both divide by max(norm, 1e-12)

soft_pooled (``pooled=True``) is what the reference's VLAD.generate computes: it reduces `w * residuals` over the tokens AND the
centres (utilities.py:883-884, "q c d -> (q c) d"), so its block k holds the residuals against every centre,
    V[s][k] = sum_{n in U(s)} w[n][k] sum_c (x^_n - c_c) = K sum_n w[n][k] x^_n - (sum_n w[n][k]) sum_c c_c
with the same weights and the same normalisations.  tests/golden/vlad_soft.npz pins it; it does not tend to the hard VLAD as T grows.

The inputs are those of tests/describe_shape_cases.py, imported unchanged.
"""
import functools

import numpy as np

import describe_shape_cases as T

EPS = 1e-12
TEMPS = (1.0, 10.0, 100.0)
# The shape table's cases of the soft kernels, and what each one exercises there
CASES = [
    "k1_d32_n130",          # K = 1: every weight is exactly 1
    "k2_d36_n65",           # narrow assignment, odd N, partial slab
    "k31_d64_n257",         # one padded centre: the padding must not enter the softmax
    "k33_d96_n129",         # Kpad = 64
    "k65_d200_n333",        # Kpad = 128, D % 32 != 0
    "k128_d64_n513_s129",   # SC = 3, top label 127
    "k128_d1536_n130",      # widest D
    "k32_d32_n1530_s400",   # non-staged union, S = 400
]
PCA_CASES = ["k33_d96_n129", "k97_d384_n260"]
# tests/test_describe_shape_cases.py qualifies every case of the table with a top-2 gap >= MIN_GAP; at SATURATING_TEMP every weight
# but the arg-max's is below exp(-120) = 7.7e-53, which is 0 in fp32 (and 1e-52 of the descriptor in fp64)
MIN_GAP = 1e-4
SATURATING_TEMP = 120.0 / MIN_GAP


def weights(tok_dn, C, temp):
    """w [N][K] and the normalised tokens x^ [N][D], fp64"""
    X = np.asarray(tok_dn, dtype=np.float64).T
    C = np.asarray(C, dtype=np.float64)
    xh = X / np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), EPS)
    ch = C / np.maximum(np.sqrt((C * C).sum(1, keepdims=True)), EPS)
    z = float(temp) * (xh @ ch.T)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True), xh


def soft_vlad(tok_dn, C, inc, adj, temp, pooled=False):
    """One image: dict(out [S][K D], block_norms [S][K], w [N][K]), fp64.  adj None: order 0.  pooled: soft_pooled's blocks."""
    C = np.asarray(C, dtype=np.float64)
    K, D = C.shape
    inc = np.asarray(inc, dtype=bool)
    S = inc.shape[0]
    w, xh = weights(tok_dn, C, temp)
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
    return dict(out=out, block_norms=bn, w=w)


def needed_rtol(got, ref, atol=1e-6):
    """The smallest rtol at which np.allclose(got, ref, rtol, atol) holds"""
    dev = np.abs(np.asarray(got, dtype=np.float64) - ref) - atol
    nz = np.abs(ref) > 0
    return float(max(0.0, (dev[nz] / np.abs(ref[nz])).max())) if nz.any() else 0.0


def pooled_block_norms_fp32(tok_dn, C, inc, adj, temp):
    """soft_pooled's block norms [S][K] of one image in the reference's own arithmetic: fp32 torch, cosine_similarity, softmax, the
    residuals summed over the centres and weighted (utilities.py:870-884), over the tokens of the neighbour union"""
    import torch
    import torch.nn.functional as F

    x = F.normalize(torch.from_numpy(np.ascontiguousarray(np.asarray(tok_dn, dtype=np.float32).T)))
    c = torch.from_numpy(np.asarray(C, dtype=np.float32))
    w = F.softmax(float(temp) * F.cosine_similarity(x[:, None, :], c[None], dim=2), dim=1)
    res = (x[:, None, :] - c[None]).sum(1)
    inc = np.asarray(inc, dtype=bool)
    S = inc.shape[0]
    U = inc if adj is None else (np.asarray(adj, dtype=np.int64).reshape(S, S) @ inc.astype(np.int64)) > 0
    V = torch.einsum("sn,nk,nd->skd", torch.from_numpy(U.astype(np.float32)), w, res)
    return V.norm(dim=2).numpy()


def soft_batch(toks, incs, adjs, C, with_adj, temp, pooled=False):
    """soft_vlad per image of a batch (a repeated image -- the same arrays -- is computed once): dict(out [S_tot, K D],
    block_norms [S_tot, K], zero_rows: the segments whose neighbour union holds no token)"""
    outs, bns, zero, done = [], [], [], {}
    for b in range(len(toks)):
        key = id(toks[b])
        if key not in done:
            done[key] = soft_vlad(toks[b], C, incs[b], adjs[b] if with_adj else None, temp, pooled)
        union = incs[b] if not with_adj else (adjs[b].astype(np.int64) @ incs[b].astype(np.int64)) > 0
        outs.append(done[key]["out"]), bns.append(done[key]["block_norms"]), zero.append(~union.any(1))
    return dict(out=np.concatenate(outs), block_norms=np.concatenate(bns), zero_rows=np.concatenate(zero))


@functools.lru_cache(maxsize=None)
def reference(name, with_adj, temp, pooled=False):
    """The restatement on a case of the shape table, computed once per process and never written to"""
    d = T.build(name)
    return soft_batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj, temp, pooled)


def pca_reference(name, with_adj, temp, l2norm):
    """The restatement pushed through the fp64 PCA of the case's model (oracle.pca_transform, whitened; + normalize_feat)"""
    from oracle import segvlad_oracle as O

    y = O.pca_transform(reference(name, with_adj, temp)["out"], *T.pca_model(name), True)
    return O.normalize_feat(y) if l2norm else y


# ---- the fixture pinned to the reference (tools/make_soft_vlad_golden.py) -----------------------------------------------------
GOLDEN_SEEDS = (2010, 2011)
GOLDEN_TEMPS = (1.0, 10.0)


@functools.lru_cache(maxsize=None)
def golden_inputs():
    """(vocabulary [32][1536], the two token sets [1536][1530]) of anyloc_cases.npz / vlad_soft.npz"""
    import os

    from revisit_anything_amd import synth

    voc = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_indoor_k32_d1536.npy"))
    return voc, [synth.make_tokens(voc, 34 * 45, seed=s, noise=0.2) for s in GOLDEN_SEEDS]


def golden_projection(voc):
    return np.random.Generator(np.random.PCG64(780)).standard_normal((voc.size, 8))
