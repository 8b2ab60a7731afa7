"""segvlad_cluster_aggregate's shape table: (num_c, D, N, S) cases of the K-parametric aggregation of given residuals and labels
(csrc/describe.hip; include/segvlad.h promises labels < num_c <= 256).  set_vocab ends at 128 clusters, so this entry alone
brings labels 128 .. 255 and num_c = 129 .. 256 to prep_kernel (kcnt[257], its `k <= K` loop, where thread 0 takes entries 0
and 256 at K = 256) and to the aggregation grid (ceil(num_c / 4) workgroups, the last with num_c % 4 clusters).  A plain module:
tests/test_cluster_aggregate_cases.py qualifies every case with the fp64 oracle alone, tests/test_gpu_cluster_aggregate.py
runs the kernels.

What the launchers take from the shape (tests/describe_shape_cases.py has the rules): nw = ceil(N / 64) words per bit row,
SC = ceil(S / 64) words of segment columns, ceil(D / 128) aggregation waves, the last owning D - 128 (waves - 1) columns,
kpb_tail = num_c % 4.  The entry runs without a vocabulary in the context (centres == nullptr): the residuals are given.

Inputs: a seeded vocabulary C [num_c, D] and unit tokens x^; labels are arbitrary bytes below num_c (not the arg-max), with the top
label present, cluster EMPTY (num_c >= 2) absent and cluster SINGLE (num_c >= 3) on exactly one token, which segment 0 covers;
residuals x^ - C[label] in fp32.  Segment 1 covers no token and, in the adjacency (density 0.1, diagonal set), is isolated.
"""
import functools

import numpy as np

import describe_shape_cases as DS

ADJ_DENSITY = 0.1
EMPTY, SINGLE = 1, 2


def _case(name, num_c, D, N, S, expect, seed=0):
    return dict(name=name, num_c=num_c, D=D, N=N, S=S, seed=seed, expect=expect)


CASES = [
    # The smallest D and num_c: one aggregation workgroup walking one cluster, one wave owning 4 of its 128 columns.  With one
    # cluster none can be empty and none can hold a single token.
    _case("c1_d4_n65_s3", 1, 4, 65, 3, dict(nw=2, SC=1, agg_waves=1, last_slab=4, kpb_tail=1, agg_groups=1)),
    _case("c5_d36_n200_s9", 5, 36, 200, 9, dict(nw=4, SC=1, agg_waves=1, last_slab=36, kpb_tail=1, agg_groups=2)),
    # The first label above 127 (a label path of 7 bits would fold it onto 0).
    _case("c129_d36_n300_s37", 129, 36, 300, 37, dict(nw=5, SC=1, agg_waves=1, last_slab=36, kpb_tail=1, agg_groups=33, top_label=128)),
    # Two aggregation waves, the second owning 4 columns; S = 70: two words of segment columns.
    _case("c200_d132_n513_s70", 200, 132, 513, 70, dict(nw=9, SC=2, agg_waves=2, last_slab=4, kpb_tail=0, agg_groups=50, top_label=199)),
    _case("c255_d64_n257_s9", 255, 64, 257, 9, dict(nw=5, SC=1, agg_waves=1, last_slab=64, kpb_tail=3, agg_groups=64, top_label=254)),
    # The top label 255, K = 256 in prep_kernel (thread 0 takes kcnt[0] and kcnt[256]); S = 129: SC = 3; N = 1030: nw = 17.
    _case("c256_d32_n1030_s129", 256, 32, 1030, 129, dict(nw=17, SC=3, agg_waves=1, last_slab=32, kpb_tail=0, agg_groups=64, top_label=255)),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def launch_facts(c):
    waves = (c["D"] + 127) // 128
    return dict(nw=(c["N"] + 63) // 64, SC=(c["S"] + 63) // 64, agg_waves=waves, last_slab=c["D"] - 128 * (waves - 1),
                kpb_tail=c["num_c"] % 4, agg_groups=(c["num_c"] + 3) // 4, top_label=c["num_c"] - 1,
                prep_lds=DS.prep_lds(c["num_c"], c["N"], c["S"]))


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of a case, built once per process and never written to."""
    from oracle import segvlad_oracle as O
    from revisit_anything_amd import synth

    c = BY_NAME[name]
    K, D, N, S = c["num_c"], c["D"], c["N"], c["S"]
    seed = 12000 + 100 * c["seed"] + 10 * NAMES.index(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    C = synth.make_vocab(K, D, seed=seed + 1)
    xn = O.normalize_tokens_f32(synth.make_tokens(C, N, seed=seed + 2, noise=0.3))              # [N, D] unit rows
    allowed = np.array([k for k in range(K) if K == 1 or k != EMPTY and (K < 3 or k != SINGLE)])
    labels = allowed[rng.integers(0, len(allowed), N)].astype(np.uint8)
    labels[[3, N - 1]] = K - 1                                                                   # the top label, twice
    inc, adj = DS.draw_segments(rng, S, N, ADJ_DENSITY, isolate_1=True)
    single_token = None
    if K >= 3:
        single_token = N // 2
        labels[single_token] = SINGLE
        inc[0, single_token] = True
    inc[0, 3] = True                                                                             # a top-label token is covered
    res = (xn - C[labels]).astype(np.float32)
    bits = np.ascontiguousarray(O.pack_bits_u64(inc)).view(np.int64)
    return dict(case=c, num_c=K, D=D, N=N, S=S, C=C, labels=labels, res=res, inc=inc, adj=adj.astype(np.uint8), bits=bits,
                single_token=single_token)


def oracle(d, labels, with_adj):
    """oracle.vlad_matmuls_per_cluster in fp64: (out [S, num_c D], block norms [S, num_c], the rows that must be exactly 0)"""
    from oracle import segvlad_oracle as O

    adj = d["adj"] if with_adj else None
    out, bn = O.vlad_matmuls_per_cluster(d["num_c"], d["inc"], d["res"].astype(np.float64), np.asarray(labels, dtype=np.int64), adj,
                                         return_block_norms=True)
    union = (d["adj"].astype(np.int64) @ d["inc"].astype(np.int64)) > 0 if with_adj else d["inc"]
    return out, bn, ~union.any(1)


@functools.lru_cache(maxsize=None)
def reference(name, with_adj):
    d = build(name)
    return oracle(d, d["labels"], with_adj)
