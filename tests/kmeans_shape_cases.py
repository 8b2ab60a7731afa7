"""segvlad_kmeans_step's shape table: hand-chosen (K, D, N, B, batch) cases, one per branch that sv_launch_centroid_sums and
centroid_sums_kernel (csrc/kmeans_kernels.hip) take from the shape alone.  A plain module (no fixtures):
tests/test_kmeans_shape_cases.py checks on the CPU, with the fp64 oracle only, that every case qualifies (top-2 gap, the
branch it is named for, an error bound that a wrong kernel would miss); tests/test_gpu_kmeans_shapes.py runs the kernels on it.

How the launcher decides (the facts `launch_facts` restates):
  CH            256, halved while K CH 4 > 65536: 256 for K <= 64, 128 for K = 65 .. 128 (set_vocab ends at K = 128)
  grid          (ceil(D / CH), images of the call); workgroup j owns columns [CH j, CH j + cw), cw = min(CH, D - CH j)
  LDS           K CH 4 B dynamic ([K][CH] fp32 accumulators) beside 1024 B static (s_cnt[256]): 66560 B at K = 64 and K = 128
  token loop    rounds of 8 tokens; the last round clamps its loads to token N - 1 and guards its adds with t0 + u < N:
                (-N) % 8 padding lanes
  histogram     chunk 0's workgroup, ceil(N / 256) strided rounds of its 256 threads
  partials      [B_call][K][D] fp32, reduced over the call's images in fp64 and ADDED to sums / counts: ceil(B / batch) calls
The assignment pass in front of it is the describe stage's (tests/describe_shape_cases.py: Kpad, wide / narrow kernel).

Inputs, like test_kmeans_step_kernel_with_a_converged_and_an_empty_cluster: centres normalize(g) u with u in [0.4, 1], tokens
(C[z] + noise g) f with a factor f in [0.5, 3] per token (the kernel normalises them itself).  With K >= 3, cluster 1 is never
drawn and cluster 2 is drawn for exactly one token of one image; the CPU test asserts that the oracle's labels keep both.

The error bound of the sums (the derivation is in tests/test_gpu_kmeans_shapes.py) is computed here, by `bound`, for both tests.
"""
import functools

import numpy as np

U = 2.0 ** -24              # fp32 unit roundoff
EMPTY_CLUSTER = 1           # (K >= 2) receives no token
SINGLE_CLUSTER = 2          # (K >= 3) receives one token, in image SINGLE_IMAGE(B)


def _case(name, K, D, N, B, batch, expect, noise=0.1, seed=0):
    return dict(name=name, K=K, D=D, N=N, B=B, batch=batch, noise=noise, seed=seed, expect=expect)


CASES = [
    # One label; D = 32 < CH = 256: 224 of the 256 threads idle, cw = 32; N = 7: less than one round of 8 (one padding lane);
    # K = 1: part_cnt written by thread 0 only.  No cluster can stay empty and none can hold a single token: K = 1.
    _case("k1_d32_n7_b1", 1, 32, 7, 1, 1, dict(CH=256, chunks=1, last_cw=32, rounds8=1, pad_lanes=1, hist_rounds=1, calls=1,
                                               assign="wide<1>")),
    # D = 36: the narrow assignment kernel; N = 9: the second round of 8 holds one token (7 padding lanes); cluster 1 receives
    # nothing.  K = 2 with cluster 1 empty leaves every token in cluster 0: no cluster with a single token at this shape.
    _case("k2_d36_n9_b3", 2, 36, 9, 3, 3, dict(CH=256, chunks=1, last_cw=36, rounds8=2, pad_lanes=7, hist_rounds=1, calls=1,
                                               assign="narrow<1>")),
    # First K on Kpad = 64; N = 513 = 2 * 256 + 1: the histogram runs three strided rounds, the third with thread 0 alone.
    _case("k33_d96_n513_b2", 33, 96, 513, 2, 2, dict(CH=256, chunks=1, last_cw=96, rounds8=65, pad_lanes=7, hist_rounds=3, calls=1,
                                                     kpad=64, assign="wide<2>"), noise=0.05),   # (noise 0.1: a token lands in cluster 1)
    # K = 64: the last K with CH = 256, 65536 B dynamic + 1024 B static = 66560 B of LDS; D == CH: every thread owns a column.
    _case("k64_d256_n300_b2", 64, 256, 300, 2, 2, dict(CH=256, chunks=1, last_cw=256, dyn_lds=65536, lds=66560, hist_rounds=2,
                                                       pad_lanes=4, calls=1), noise=0.05),   # (noise 0.1: a token lands in cluster 1)
    # D = 260 = 256 + 4: a second chunk of 4 columns (252 idle threads, its histogram not taken).  N = 64: no padding lane.
    _case("k64_d260_n64_b2", 64, 260, 64, 2, 2, dict(CH=256, chunks=2, last_cw=4, lds=66560, pad_lanes=0, hist_rounds=1, calls=1)),
    # K = 65: the first K with CH = 128 (65 * 128 * 4 = 33280 B); D == CH.  Half of the threads idle whatever D.
    _case("k65_d128_n130_b2", 65, 128, 130, 2, 2, dict(CH=128, chunks=1, last_cw=128, dyn_lds=33280, pad_lanes=6, calls=1,
                                                       kpad=128, assign="narrow<4>")),
    # Three full chunks of 128; B = 3 in calls of 2 + 1 images: the second call's partials hold one image.
    _case("k97_d384_n260_b3", 97, 384, 260, 3, 2, dict(CH=128, chunks=3, last_cw=128, hist_rounds=2, pad_lanes=4, calls=2)),
    # K = 128: CH = 128 at 65536 + 1024 B; the top label is 127; D = 132 = 128 + 4: a 4-column tail; N = 257: one token past
    # 256 for the histogram and past 32 rounds of 8; B = 5 in calls of 2 + 2 + 1: accumulation over three calls.
    _case("k128_d132_n257_b5", 128, 132, 257, 5, 2, dict(CH=128, chunks=2, last_cw=4, dyn_lds=65536, lds=66560, hist_rounds=2,
                                                         pad_lanes=7, calls=3, top_label=127), noise=0.05),   # (noise 0.1: a token in cluster 1)
    # The widest D with the most clusters: 12 chunks.  (noise 0.02 as in the describe table: at D = 1536 a noise of 0.1 per
    # component has norm 3.9 against centre norms <= 1.)
    _case("k128_d1536_n130_b2", 128, 1536, 130, 2, 2, dict(CH=128, chunks=12, last_cw=128, lds=66560, pad_lanes=6, calls=1,
                                                           top_label=127), noise=0.02),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def single_image(B):
    """the image that holds SINGLE_CLUSTER's token: the second one where there is one"""
    return min(1, B - 1)


def launch_facts(c):
    """What sv_launch_centroid_sums and its kernel derive from the case's shape (the module docstring has the rules)."""
    K, D, N, B = c["K"], c["D"], c["N"], c["B"]
    CH = 256
    while K * CH * 4 > 64 * 1024:
        CH >>= 1
    chunks = (D + CH - 1) // CH
    kpad = 32 if K <= 32 else 64 if K <= 64 else 128
    wide = kpad <= 64 and D % 32 == 0
    return dict(CH=CH, chunks=chunks, last_cw=D - CH * (chunks - 1), dyn_lds=K * CH * 4, lds=K * CH * 4 + 256 * 4,
                rounds8=(N + 7) // 8, pad_lanes=(-N) % 8, hist_rounds=(N + 255) // 256, calls=(B + c["batch"] - 1) // c["batch"],
                kpad=kpad, assign=("wide<%d>" if wide else "narrow<%d>") % (kpad // 32), top_label=K - 1)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of a case, built once per process and never written to: C [K, D] fp32, tok [B, D, N] fp32"""
    c = BY_NAME[name]
    K, D, N, B = c["K"], c["D"], c["N"], c["B"]
    seed = 9000 + 100 * c["seed"] + 10 * NAMES.index(name)
    rng = _rng(seed)
    C = rng.standard_normal((K, D))
    C = C / np.linalg.norm(C, axis=1, keepdims=True) * rng.uniform(0.4, 1.0, (K, 1))
    drawn = np.array([k for k in range(K) if K == 1 or k != EMPTY_CLUSTER and (K < 3 or k != SINGLE_CLUSTER)])
    z = drawn[rng.integers(0, len(drawn), (B, N))]
    z[:, -1] = drawn[-1]                       # the top label is there, on the last token of every image
    single = None
    if K >= 3:
        single = (single_image(B), N // 2)
        z[single] = SINGLE_CLUSTER
    X = C[z] + c["noise"] * rng.standard_normal((B, N, D))
    X *= rng.uniform(0.5, 3.0, (B, N, 1))
    tok = np.ascontiguousarray(X.transpose(0, 2, 1)).astype(np.float32)
    return dict(case=c, K=K, D=D, N=N, B=B, C=C.astype(np.float32), tok=tok, drawn=z, single=single)


def rho(D):
    """Relative error of 1 / max(sqrtf(s2), 1e-12) in units of U: the assignment kernels' s2 rounds at most D / 2 + 3 times,
    sqrt halves that, then one rounding each for the square root and the division (tests/test_gpu_kmeans_shapes.py)."""
    return (D / 2 + 3) / 2 + 2


@functools.lru_cache(maxsize=None)
def reference(name):
    """From the fp32 tokens in fp64, per image: x^ = x / ||x||, labels and top-2 gap of oracle.assign_labels, partial sums
    part [B, K, D] = sum of x^ over the image's tokens of a label, absolute sums apart [B, K, D], counts cnt [B, K]."""
    from oracle import segvlad_oracle as O

    d = build(name)
    K, D, N, B = d["K"], d["D"], d["N"], d["B"]
    xh = np.empty((B, N, D))
    labels = np.empty((B, N), np.int64)
    gap = np.empty((B, N))
    part, apart = np.zeros((B, K, D)), np.zeros((B, K, D))
    cnt = np.zeros((B, K), np.int64)
    for b in range(B):
        x = d["tok"][b].T.astype(np.float64)
        xh[b] = x / np.sqrt((x * x).sum(1, keepdims=True))
        labels[b], gap[b] = O.assign_labels(O.normalize_tokens_f32(d["tok"][b]), d["C"])
        np.add.at(part[b], labels[b], xh[b])
        np.add.at(apart[b], labels[b], np.abs(xh[b]))
        cnt[b] = np.bincount(labels[b], minlength=K)
    return dict(xh=xh, labels=labels, gap=gap, part=part, apart=apart, cnt=cnt, sums=part.sum(0), counts=cnt.sum(0))


def bound(name, passes=1):
    """[K, D]: U sum_b (n_bk - 1 + 2 + rho) sum_{t in image b, label k} |x^_tc|; `passes` full passes over the images"""
    r = reference(name)
    n = r["cnt"].astype(np.float64)[:, :, None]
    return passes * U * ((n + 1 + rho(BY_NAME[name]["D"])) * r["apart"]).sum(0)


def existing_figure(name):
    """[K, 1]: tests/test_gpu_frows.py's measured 1e-6 max|sums[k]| max(1, sqrt(n_k)) per cluster"""
    r = reference(name)
    return (1e-6 * np.abs(r["sums"]).max(1) * np.maximum(1.0, np.sqrt(r["counts"])))[:, None]


def calls(c):
    """[(first image, images)] of the calls that a case is fed in"""
    return [(b0, min(c["batch"], c["B"] - b0)) for b0 in range(0, c["B"], c["batch"])]


# ---- what a subtly wrong kernel would compute: (sums, counts) from the reference's per-image parts, or None where the case's
# shape makes the mistake a no-op (tests/test_kmeans_shape_cases.py asserts that it is one) -----------------------------------
def _last(r, K):
    """[B, K, D]: x^ of every image's last token in the row of its label, and the labels [B]"""
    B, N, D = r["xh"].shape
    e = np.zeros((B, K, D))
    lab = r["labels"][:, -1]
    e[np.arange(B), lab] = r["xh"][:, -1]
    return e, lab


def p_drop_last_token(c, r):
    e, lab = _last(r, c["K"])
    cnt = r["cnt"].copy()
    cnt[np.arange(c["B"]), lab] -= 1
    return (r["part"] - e).sum(0), cnt.sum(0)


def p_padding_lanes_added(c, r):
    pad = (-c["N"]) % 8
    return ((r["part"] + pad * _last(r, c["K"])[0]).sum(0), r["counts"]) if pad else None


def p_ragged_chunk_zero(c, r):
    f = launch_facts(c)
    if f["last_cw"] == f["CH"]:
        return None
    s = r["sums"].copy()
    s[:, f["CH"] * (f["chunks"] - 1):] = 0
    return s, r["counts"]


def p_chunk_offset_256(c, r):
    f = launch_facts(c)
    if c["K"] <= 64 or f["chunks"] == 1:
        return None
    s = np.zeros_like(r["sums"])
    for j in range(f["chunks"]):
        w = min(min(128, c["D"] - 128 * j), max(0, c["D"] - 256 * j))
        s[:, 256 * j:256 * j + w] = r["sums"][:, 128 * j:128 * j + w]
    return s, r["counts"]


def p_histogram_first_256(c, r):
    if c["N"] <= 256:
        return None
    return r["sums"], np.stack([np.bincount(l[:256], minlength=c["K"]) for l in r["labels"]]).sum(0)


def p_second_call_overwrites(c, r):
    if len(calls(c)) == 1:
        return None
    b0, nb = calls(c)[-1]
    return r["part"][b0:b0 + nb].sum(0), r["cnt"][b0:b0 + nb].sum(0)


def p_image1_from_image0(c, r):
    if c["B"] == 1:
        return None
    return r["sums"] - r["part"][1] + r["part"][0], r["counts"] - r["cnt"][1] + r["cnt"][0]


PERTURBATIONS = [("last token dropped", p_drop_last_token), ("last token added per padding lane", p_padding_lanes_added),
                 ("ragged last chunk left at zero", p_ragged_chunk_zero), ("chunk offset 256 j at K > 64", p_chunk_offset_256),
                 ("histogram of the first 256 tokens", p_histogram_first_256), ("second call overwrites", p_second_call_overwrites),
                 ("image 1's partial from image 0", p_image1_from_image0)]
