"""The describe stage's shape table: hand-chosen (K, D, N, S) cases, one per branch that the launchers of
csrc/assign_kernels.hip, csrc/vlad_kernels.hip, csrc/block_norm_kernels.hip, csrc/project_kernels.hip and csrc/describe.hip take from the shape alone.  A plain module (no
fixtures): tests/test_describe_shape_cases.py checks on the CPU, with the fp64 oracle only, that every case qualifies
(top-2 gap, block-norm floor, the branch it is named for); tests/test_gpu_describe_shapes.py runs the kernels on it.

Every batch has B = 4 images: image 0 (S0 segments), image 1 without segments, image 2 (S2 segments) and image 3 = image 0
again (its rows must be bit-equal to image 0's).  Segment 1 of images 0 and 2 covers no token; in image 0 it also has no
neighbour but itself, so its descriptor row is exactly 0 with and without the adjacency.  Cluster 1 (K >= 2) receives no
token: the tokens are drawn around the other centres.

How the launchers decide (the facts `launch_facts` restates, and the case comments quote):
  set_vocab            Kpad = 32 | 64 | 128 for K <= 32 | <= 64 | <= 128, NT = Kpad / 32
  sv_launch_assign     assign_wide_kernel<NT> (128-token tiles) when NT <= 2 and D % 32 == 0, else assign_kernel<NT> (64-token
                       tiles; 8-byte pair loads when N is even, scalar loads when N is odd)
  sv_launch_prep       nw = ceil(N / 64), ord_n = max(N, S_max) rounded up to even,
                       lds        = (S_max + K) nw 8 + ord_n 4 + nw 8 + (nw + 2) 4            refused above 160 KiB
                       lds_staged = (S_max + K) nw 8 + ord_n 4 + S_max nw 8 + S_max ceil(S_max / 64) 8
                       the neighbour union is staged in LDS when lds_staged <= 150 KiB, else read from global memory
  describe plan        SC = ceil(S_max / 64) words of segment columns per token
  sv_launch_aggregate  ceil(D / 128) waves, wave w owns columns [128 w, 128 w + 128): the last one D - 128 (waves - 1) of them;
                       agg_kpb = 4 clusters per workgroup, the last workgroup K % 4 of them when K % 4 != 0
  pca_set / plan       fp16x3 planes exist when K D % 32 == 0 ("planes" form; "project" form when also D % 32 == 0); otherwise,
                       or with pca_arith=fp32, the plain projection behind the descriptor
  sv_launch_token_norms (project form) a task = the tokens of one image in one cluster: <= 32 one Gram tile, 33 .. 64 two
                       Gram tiles, 65 .. 255 the block-sum kernel with its lists in LDS, >= 256 its BIG instantiation
"""
import functools

import numpy as np

P = 32               # projected width of every case's PCA model (a multiple of 4: the project form takes it)
B = 4
INC_DENSITY = 0.2
EMPTY_CLUSTER = 1    # (K >= 2)
TASK_CLASSES = {"le32": (1, 32), "33to64": (33, 64), "65to255": (65, 255), "ge256": (256, 10 ** 9)}


def _case(name, K, D, N, segs, expect, noise=0.1, adj_density=0.1, seed=0):
    assert len(segs) == 2
    return dict(name=name, K=K, D=D, N=N, segs=(segs[0], 0, segs[1], segs[0]), noise=noise, adj_density=adj_density, seed=seed,
                expect=expect)


CASES = [
    # One cluster: Kpad = 32 with 31 padded centres, the gap output is +inf, no cluster can stay empty.  D = 32 is one chunk of
    # the wide assignment kernel (its loop body runs once, nothing to prefetch); every task holds all N = 130 tokens: 65 .. 255.
    _case("k1_d32_n130", 1, 32, 130, (9, 37), dict(kpad=32, assign="wide<1>", pad_centres=31, task_class="65to255", x3=True, project=True)),
    # D = 36: not a multiple of 32 -> assign_kernel<1>; N = 65 is odd -> its scalar loads, and one token past the first 64-token
    # tile.  K D = 72, not a multiple of 32: no planes, the plain projection.  One aggregation wave owning 36 of its 128 columns.
    _case("k2_d36_n65", 2, 36, 65, (9, 37), dict(kpad=32, assign="narrow<1>", odd_n=True, x3=False, project=False, agg_waves=1,
                                                 last_slab=36, kpb_tail=2)),
    # The shape tests/test_gpu_describe.py compares device against device.  K D = 180: plain projection.  K % 4 = 1.
    _case("k5_d36_n200", 5, 36, 200, (9, 37), dict(kpad=32, assign="narrow<1>", odd_n=False, x3=False, last_slab=36, kpb_tail=1)),
    # The same partial slab with fp16x3 planes: K D = 288 = 9 * 32 while D % 32 != 0 -> "planes" form, no "project" form.
    _case("k8_d36_n99", 8, 36, 99, (9, 37), dict(kpad=32, assign="narrow<1>", odd_n=True, x3=True, project=False, last_slab=36, kpb_tail=0)),
    # One short of the pad (a single padded centre).  N = 257: one token past two 128-token tiles of the wide kernel and past
    # 4 x 64 (the narrow kernel's fifth tile holds one token; N is odd).
    _case("k31_d64_n257", 31, 64, 257, (9, 37), dict(kpad=32, assign="wide<1>", pad_centres=1, odd_n=True, x3=True, project=True, kpb_tail=3)),
    # First K on Kpad = 64: 31 padded centres.  D = 96 = 3 * 32: three chunks of the wide kernel (an odd count: the unrolled-by-two
    # loop ends on its first half), one aggregation wave owning 96 columns, grouped-GEMM depth 96.  N = 129: one past a tile.
    _case("k33_d96_n129", 33, 96, 129, (9, 37), dict(kpad=64, assign="wide<2>", pad_centres=31, x3=True, project=True, agg_waves=1,
                                                     last_slab=96, kpb_tail=1)),
    # Full Kpad = 64.  D = 160: two aggregation waves, the second owns 160 - 128 = 32 columns.
    _case("k64_d160_n300", 64, 160, 300, (9, 37), dict(kpad=64, assign="wide<2>", pad_centres=0, x3=True, project=True, agg_waves=2,
                                                       last_slab=32, kpb_tail=0)),
    # First K on Kpad = 128: assign_kernel<4> whatever D.  D = 200: D % 32 = 8 (and a 64-wide assignment chunk of 8 columns),
    # the second aggregation wave owns 72 columns.  K % 4 = 1: the last aggregation workgroup walks one cluster.  K D = 13000.
    _case("k65_d200_n333", 65, 200, 333, (9, 37), dict(kpad=128, assign="narrow<4>", pad_centres=63, odd_n=True, x3=False, agg_waves=2,
                                                       last_slab=72, kpb_tail=1)),
    # ViT-S width, K % 4 = 1 on Kpad = 128, an image with S = 70 (two words of segment columns, 6 rows in the second) and adjacency.
    _case("k97_d384_n260", 97, 384, 260, (9, 70), dict(kpad=128, assign="narrow<4>", pad_centres=31, x3=True, project=True, agg_waves=3,
                                                       last_slab=128, kpb_tail=1, SC=2)),
    # K = 128: the top label is 127 (the byte labels' largest), 32 aggregation workgroups per image, the project form's per-cluster
    # LDS rows at their most.  S = 129 = 2 * 64 + 1: SC = 3, the third word holds one segment.  N = 513 = 8 * 64 + 1: nw = 9.
    _case("k128_d64_n513_s129", 128, 64, 513, (9, 129), dict(kpad=128, assign="narrow<4>", pad_centres=0, x3=True, project=True, SC=3,
                                                             top_label=127, staged=True)),
    # The widest supported D with the most clusters: 12 aggregation waves (768 threads), 24 chunks of the narrow assignment.
    # (noise 0.02: at D = 1536 a noise of 0.1 per component has norm 3.9 against centre norms <= 1.)
    _case("k128_d1536_n130", 128, 1536, 130, (5, 34), dict(kpad=128, assign="narrow<4>", x3=True, project=True, agg_waves=12, last_slab=128,
                                                           top_label=127), noise=0.02),
    # prep_kernel's non-staged neighbour union.  N = 1530 -> nw = 24, ord_n = 1530; S_max = 400, K = 32:
    #   lds        = 432 * 24 * 8 + 1530 * 4 + 24 * 8 + 26 * 4       =  89360 B  (< 160 KiB = 163840: accepted)
    #   lds_staged = 432 * 24 * 8 + 1530 * 4 + 400 * 24 * 8 + 400 * 7 * 8 = 188264 B  (> 150 KiB = 153600: not staged)
    # SC = ceil(400 / 64) = 7 words of segment columns, the last one holding 16 segments.  (noise 0.05: at D = 32 a noise of 0.1
    # sends tokens to the cluster that has to stay empty.)
    _case("k32_d32_n1530_s400", 32, 32, 1530, (5, 400), dict(kpad=32, assign="wide<1>", x3=True, project=True, SC=7, staged=False),
          noise=0.05, adj_density=0.02),
    # Task-size classes of the project form's token kernels at D = 96 (tests/test_gpu_cover_rows.py has them at D = 64).
    _case("cls_le32_k32_d96_n99", 32, 96, 99, (9, 37), dict(task_class="le32", project=True, kpad=32, assign="wide<1>"),
          seed=1),    # (seed 0: a top-2 gap of 9e-5)
    _case("cls_33to64_k3_d96_n99", 3, 96, 99, (9, 37), dict(task_class="33to64", project=True, kpb_tail=3)),
    _case("cls_65to255_k2_d96_n130", 2, 96, 130, (9, 37), dict(task_class="65to255", project=True)),
    _case("cls_ge256_k2_d96_n300", 2, 96, 300, (9, 37), dict(task_class="ge256", project=True)),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def prep_lds(K, N, S_max):
    """(lds, lds_staged) of sv_launch_prep, in bytes"""
    nw = (N + 63) // 64
    ord_n = (max(N, S_max) + 1) & ~1
    lds = (S_max + K) * nw * 8 + ord_n * 4 + nw * 8 + (nw + 2) * 4
    lds_staged = (S_max + K) * nw * 8 + ord_n * 4 + S_max * nw * 8 + S_max * ((S_max + 63) // 64) * 8
    return lds, lds_staged


def launch_facts(c):
    """What the launchers derive from the case's shape (the module docstring has the rules)."""
    K, D, N = c["K"], c["D"], c["N"]
    S_max = max(c["segs"])
    kpad = 32 if K <= 32 else 64 if K <= 64 else 128
    nt = kpad // 32
    wide = nt <= 2 and D % 32 == 0
    waves = (D + 127) // 128
    lds, lds_staged = prep_lds(K, N, S_max)
    return dict(kpad=kpad, assign=("wide<%d>" if wide else "narrow<%d>") % nt, pad_centres=kpad - K, odd_n=bool(N & 1), agg_waves=waves,
                last_slab=D - 128 * (waves - 1), kpb_tail=K % 4, SC=(S_max + 63) // 64, x3=K * D % 32 == 0,
                project=K * D % 32 == 0 and D % 32 == 0 and P % 4 == 0, prep_lds=lds, prep_lds_staged=lds_staged,
                staged=lds_staged <= 150 * 1024)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


def draw_segments(rng, S, N, adj_density, isolate_1):
    """Incidence [S, N] at INC_DENSITY and adjacency [S, S] (diagonal set) from a seeded generator; segment 1 (S > 2) covers no
    token and, with isolate_1, has no neighbour but itself."""
    inc = rng.random((S, N)) < INC_DENSITY
    adj = (rng.random((S, S)) < adj_density) | np.eye(S, dtype=bool)
    if S > 2:
        inc[1] = False
        if isolate_1:
            adj[1] = False
            adj[1, 1] = True
    return inc, adj


def pack_batch(toks, incs, adjs):
    """The engine's operands: tokens [B, D, N], bit rows (int64 storage), segment offsets, concatenated adjacency blocks"""
    from oracle import segvlad_oracle as O

    N = toks[0].shape[1]
    offs = np.concatenate([[0], np.cumsum([i.shape[0] for i in incs])]).astype(np.int32)
    bits = np.concatenate([O.pack_bits_u64(i) for i in incs]) if offs[-1] else np.zeros((0, (N + 63) // 64), np.uint64)
    adj = np.concatenate([np.asarray(a, dtype=np.uint8).reshape(-1) for a in adjs])
    return np.stack(toks), np.ascontiguousarray(bits).view(np.int64), offs, adj


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of a case, built once per process and never written to."""
    from revisit_anything_amd import synth

    c = BY_NAME[name]
    K, D, N, seed = c["K"], c["D"], c["N"], 7000 + 100 * c["seed"] + 10 * NAMES.index(name)
    C = synth.make_vocab(K, D, seed=seed)
    used = np.delete(C, EMPTY_CLUSTER, axis=0) if K >= 2 else C
    rng = _rng(seed + 1)
    toks, incs, adjs = [], [], []
    for b, S in enumerate(c["segs"][:3]):
        toks.append(synth.make_tokens(used, N, seed=seed + 2 + b, noise=c["noise"]))
        inc, adj = draw_segments(rng, S, N, c["adj_density"], isolate_1=b == 0)
        incs.append(inc)
        adjs.append(adj)
    toks.append(toks[0]), incs.append(incs[0]), adjs.append(adjs[0])      # image 3 = image 0
    tok, bits, offs, adj = pack_batch(toks, incs, adjs)
    return dict(case=c, K=K, D=D, N=N, C=C, toks=toks, incs=incs, adjs=adjs, tok=tok, bits=bits, offs=offs, adj=adj)


@functools.lru_cache(maxsize=None)
def pca_model(name):
    from revisit_anything_amd import synth

    c = BY_NAME[name]
    return synth.make_pca_model(c["K"] * c["D"], P, seed=5000 + NAMES.index(name))


def oracle_batch(toks, incs, adjs, C, with_adj):
    """oracle.segvlad_oracle.seg_vlad per image: dict(out [S_tot, K D] fp64, labels [B, N], gap [B, N], block_norms [S_tot, K],
    zero_rows: the segments whose (neighbour union of the) incidence holds no token)"""
    from oracle import segvlad_oracle as O

    outs, labs, gaps, bns, zero = [], [], [], [], []
    done = {}
    for b in range(len(toks)):
        key = id(toks[b])            # a repeated image (the same arrays) is computed once
        if key not in done:
            a = adjs[b] if with_adj else None
            done[key] = O.seg_vlad(toks[b], incs[b], C, a, return_aux=True)
        ref, aux = done[key]
        union = incs[b] if not with_adj else (adjs[b].astype(np.int64) @ incs[b].astype(np.int64)) > 0
        outs.append(ref), labs.append(aux["labels"]), gaps.append(aux["gap"]), bns.append(aux["block_norms"])
        zero.append(~union.any(1))
    return dict(out=np.concatenate(outs), labels=np.stack(labs), gap=np.stack(gaps), block_norms=np.concatenate(bns),
                zero_rows=np.concatenate(zero))


@functools.lru_cache(maxsize=None)
def reference(name, with_adj):
    d = build(name)
    return oracle_batch(d["toks"], d["incs"], d["adjs"], d["C"], with_adj)


def task_sizes(labels, K):
    """[B, K]: tokens of image b in cluster k"""
    return np.stack([np.bincount(np.asarray(l, dtype=np.int64), minlength=K) for l in labels])


def image_grid(N):
    """(h, w) with h w = N, as square as N allows: the token grid of the fused entry's masks"""
    h = max(f for f in range(1, int(N ** 0.5) + 1) if N % f == 0)
    return h, N // h


# ---- inputs of another kind -------------------------------------------------------------------------------------------------
EXTRA_SHAPES = [(33, 96), (70, 40)]     # a padded K on the wide kernel (31 padded centres); K = 70 on assign_kernel<4> (58 padded)


def oracle_scores(tok_dn, C):
    """The oracle's cosine scores [N, K] (oracle.segvlad_oracle.assign_labels' operands and arithmetic)"""
    from oracle import segvlad_oracle as O

    xn = O.normalize_tokens_f32(tok_dn)
    C = np.asarray(C, dtype=np.float32)
    cn = C / np.maximum(np.sqrt((C.astype(np.float64) ** 2).sum(1)).astype(np.float32), np.float32(O.EPS))[:, None]
    return xn.astype(np.float64) @ cn.astype(np.float64).T


@functools.lru_cache(maxsize=None)
def negative_scores_batch(K, D):
    """Every real centre scores below 0, a padded (all-zero) centre would score exactly 0: the centres share a direction e
    (C_k = make_vocab row + 0.5 e), the tokens are -normalize(mean of the centres) + 0.02 g, un-normalised."""
    from revisit_anything_amd import synth

    N, seed = 130, 10100 + K     # (a seed at which the oracle's gap qualifies: tests/test_describe_shape_cases.py)
    rng = _rng(seed)
    e = rng.standard_normal(D)
    C = (synth.make_vocab(K, D, seed=seed + 1) + 0.5 * e / np.linalg.norm(e)).astype(np.float32)
    m = C.astype(np.float64).mean(0)
    x = -m / np.linalg.norm(m) + 0.02 * rng.standard_normal((2 * N, D))
    toks, incs, adjs = [], [], []
    for b, S in enumerate((6, 3)):
        toks.append(np.ascontiguousarray(x[b * N:(b + 1) * N].T.astype(np.float32)))
        inc, adj = draw_segments(rng, S, N, 0.3, isolate_1=False)
        incs.append(inc), adjs.append(adj)
    tok, bits, offs, adj = pack_batch(toks, incs, adjs)
    return dict(K=K, D=D, N=N, C=C, toks=toks, incs=incs, adjs=adjs, tok=tok, bits=bits, offs=offs, adj=adj)


ZERO_TOKEN = 7   # the all-zero column of image 0


@functools.lru_cache(maxsize=None)
def zero_column_batch(K, D):
    """Image 0 holds an all-zero token (column ZERO_TOKEN, covered by segment 0); every other column of both images is scaled
    by a factor between 1e-3 and 1e3 (the kernels normalise the tokens themselves)."""
    from revisit_anything_amd import synth

    N, seed = 130, 8200 + K
    rng = _rng(seed)
    C = synth.make_vocab(K, D, seed=seed + 1)
    toks, incs, adjs = [], [], []
    for b, S in enumerate((6, 3)):
        t = synth.make_tokens(C, N, seed=seed + 2 + b, noise=0.1 if D > 64 else 0.05)
        t = t * rng.permutation(np.geomspace(1e-3, 1e3, N)).astype(np.float32)[None, :]
        inc, adj = draw_segments(rng, S, N, 0.3, isolate_1=False)
        if b == 0:
            t[:, ZERO_TOKEN] = 0.0
            inc[0, ZERO_TOKEN] = True
        toks.append(np.ascontiguousarray(t.astype(np.float32)))
        incs.append(inc), adjs.append(adj)
    tok, bits, offs, adj = pack_batch(toks, incs, adjs)
    return dict(K=K, D=D, N=N, C=C, toks=toks, incs=incs, adjs=adjs, tok=tok, bits=bits, offs=offs, adj=adj)
