"""Plain reference of the vote's one-to-one flag (SEGVLAD_VOTE_UNIQUE_REF, include/segvlad.h), a mirror of its launcher's regime
rule and hash, and the inputs that the flag's tests share.  NumPy and python only, written to be read; it never calls product code.

The flag is defined by equivalence: the flagged vote over `matches` is the plain vote (tests/search_tail_ref.py) over
blank_unique(matches, sims, off, n_ref); with a cap m in the same mode word, over vote_cap_ref.blank(blank_unique(...), img, m)."""
import functools

import numpy as np

import search_tail_ref as R
import vote_cap_ref as V

NAN, INF = float("nan"), float("inf")


def blank_unique(matches, sims, off, n_ref):
    """A copy of matches [nq][k] in which, among the valid entries (0 <= id < n_ref) of one query image that carry the same id, only
    the winner keeps its id: the largest sim (a NaN loses to every number; +0.0 == -0.0), on a tie the first in the visiting order
    (rank-major, then segment); without sims the first in the visiting order."""
    out = matches.copy()
    for b in range(len(off) - 1):
        best = {}                                   # id -> (q, r, sim)
        for r in range(matches.shape[1]):           # visiting order
            for q in range(off[b], off[b + 1]):
                i = int(matches[q, r])
                if not 0 <= i < n_ref:
                    continue
                s = None if sims is None else float(sims[q, r])
                if i not in best:
                    best[i] = (q, r, s)
                    continue
                bq, br, bs = best[i]
                if sims is not None and (s > bs or (bs != bs and s == s)):
                    out[bq, br] = -1
                    best[i] = (q, r, s)
                else:
                    out[q, r] = -1
    return out


def blank(c, sims, cap=None):
    """The lists that the vote reads for mode = base | UNIQUE_REF | PER_IMAGE(cap): one-to-one first, then the cap over the result."""
    b = blank_unique(c["matches"], sims, c["off"], len(c["img_of_seg"]))
    return b if cap is None else V.blank(b, c["img_of_seg"], cap)


# =====================================================================================================================
# mirror of sv_launch_vote_unique (csrc/vote_kernels.hip)
# =====================================================================================================================
LDS_TABLE_BYTES = 128 * 1024                             # of the CU's 160 KiB
SLOT_BYTES = 16                                          # {id + 1, best key}
SLOTS_PER_ENTRY = 2
LDS_ENTRIES = LDS_TABLE_BYTES // SLOT_BYTES // SLOTS_PER_ENTRY   # the last entry count (segments x k) the in-LDS table holds


def table_size(entries):
    return SLOTS_PER_ENTRY * entries


def home_slot(i, T):
    """The slot at which the probe for id i starts in a table of T slots; the probe goes on at +1, wrapping to 0 behind T - 1."""
    h = ((int(i) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 32
    return (h * T) >> 32


def launch_regime(seg_counts, k):
    """(images the LDS launch handles, images left to the global launches, launches the flag adds)."""
    lds = [b for b, s in enumerate(seg_counts) if 0 < s * k <= LDS_ENTRIES]
    big = [b for b, s in enumerate(seg_counts) if s * k > LDS_ENTRIES]
    return lds, big, (1 if lds else 0) + (3 if big else 0)


def global_scratch_bytes(seg_counts, k):
    """Table bytes the global launches zero: 2 slots per entry of the rows from the first to the last large image."""
    _, big, _ = launch_regime(seg_counts, k)
    if not big:
        return 0
    return sum(seg_counts[big[0]:big[-1] + 1]) * k * SLOTS_PER_ENTRY * SLOT_BYTES


def probe_chain(ids, T):
    """Insert the distinct ids in the order given; returns (slot of every id, number of probe steps that wrapped from T - 1 to 0)."""
    slot_of, taken, wraps = {}, set(), 0
    for i in ids:
        i = int(i)
        if i in slot_of:
            continue
        h = home_slot(i, T)
        while h in taken:
            h += 1
            if h == T:
                h, wraps = 0, wraps + 1
        taken.add(h)
        slot_of[i] = h
    return slot_of, wraps


# =====================================================================================================================
# literal lists: matches, sims, off, n_ref, the blanked lists with sims, the blanked lists without
# =====================================================================================================================
def _lit(matches, sims, off, n_ref, with_sims, without):
    return dict(matches=np.array(matches, np.int64), sims=np.array(sims, np.float32), off=np.array(off, np.int32), n_ref=n_ref,
                with_sims=np.array(with_sims, np.int64), without=np.array(without, np.int64))


LITERAL = {
    # one image, two segments, k = 2: (q=0, r=1) and (q=1, r=0) carry id 5 at equal sims; p = r * S + q: 2 against 1 -- (1, 0) wins
    "rank_major_tie": _lit([[1, 5], [5, 2]], [[0.9, 0.5], [0.5, 0.1]], [0, 2], 8, [[1, -1], [5, 2]], [[1, -1], [5, 2]]),
    # id 3: NaN at p = 0 against 0.25 at p = 1 -- the number wins; id 4: NaN at p = 2 and p = 3 -- the first wins
    "nan": _lit([[3, 4], [3, 4]], [[NAN, NAN], [0.25, NAN]], [0, 2], 8, [[-1, 4], [3, -1]], [[3, 4], [-1, -1]]),
    # id 6: -0.0 at p = 0, +0.0 at p = 1: equal, the first wins; id 7: -1e-30 at p = 2 loses to -0.0 at p = 3
    "zeros": _lit([[6, 7], [6, 7]], [[-0.0, -1e-30], [0.0, -0.0]], [0, 2], 8, [[6, -1], [-1, 7]], [[6, 7], [-1, -1]]),
    # id 1: -inf, 3.0, +inf at p = 0, 1, 2: +inf wins; id 2: -inf at p = 3 against NaN at p = 4: -inf is a number and wins
    "inf": _lit([[1, 2, 0], [1, 2, 0], [1, 9, 0]], [[-INF, -INF, 1.0], [3.0, NAN, 2.0], [INF, 0.0, 2.0]], [0, 3], 8,
                [[-1, 2, -1], [-1, -1, 0], [1, 9, -1]], [[1, 2, 0], [-1, -1, -1], [-1, 9, -1]]),
    # a duplicate inside one row (k = 3, one segment): the later, larger one wins
    "inside_one_row": _lit([[4, 4, 4]], [[0.5, 0.75, 0.75]], [0, 1], 8, [[-1, 4, -1]], [[4, -1, -1]]),
    # the same id in two query images: no interaction; ids past the map and below 0 stay what they are, duplicates or not
    "two_images": _lit([[2, 8], [2, -1], [2, 8]], [[0.1, 0.9], [0.2, 0.9], [0.9, 0.3]], [0, 1, 3], 8,
                       [[2, 8], [-1, -1], [2, 8]], [[2, 8], [2, -1], [-1, 8]]),
    # an image without segments between two others, and ids that differ only above bit 31
    "wide_ids": _lit([[1 << 32, 1], [1, (1 << 32) + 1], [1 << 32, 1 << 32]], [[0.5, 0.4], [0.6, 0.1], [0.2, 0.3]], [0, 2, 2, 3], (1 << 32) + 2,
                     [[1 << 32, -1], [1, (1 << 32) + 1], [-1, 1 << 32]], [[1 << 32, -1], [1, (1 << 32) + 1], [1 << 32, -1]]),
}


LITERAL_GPU = [n for n in LITERAL if n != "wide_ids"]     # (a segment -> image map of 2^32 entries is not a test input)


# =====================================================================================================================
# generated inputs
# =====================================================================================================================
SHAPES = V.SHAPES                                        # one per launch regime of the vote, and the benchmark's depth
CAPS = [None, 1, 2]


def case(name, invalid):
    return V.case(name, invalid)


@functools.lru_cache(maxsize=None)
def blanked(name, invalid, use_sims, cap):
    c = case(name, invalid)
    return blank(c, c["sims"] if use_sims else None, cap)


def largest_image_share(c, b):
    """Share of the valid entries of the case's largest image that b blanks."""
    rows = slice(c["off"][R.LARGEST], c["off"][R.LARGEST + 1])
    m = c["matches"][rows]
    valid = (m >= 0) & (m < len(c["img_of_seg"]))
    return float(((b[rows] != m) & valid).sum()) / float(valid.sum())


# (segments, k) of the image under test: the last entry count of the in-LDS table, the first beyond it, and the vote's largest test image
EDGE_SHAPES = [(64, 64), (241, 17), (145, 113)]
STRESS_KINDS = ["one_id", "table_multiples", "wrap_chain"]
N_REF_STRESS = 400_000


def wrap_ids(T, n_ref=N_REF_STRESS, tail=3):
    """Every id below n_ref whose probe starts in the last `tail` slots of a table of T slots: more ids than slots, so the chain runs
    past the table's end."""
    i = np.arange(n_ref, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)
    return np.nonzero(((h * np.uint64(T)) >> np.uint64(32)) >= np.uint64(T - tail))[0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def stress_case(kind, segs, k):
    """A 3-segment image, the image under test (segs x k entries), a 2-segment image; the ids of the image under test planted:
    one_id -- all of its entries on one id; table_multiples -- ids that are multiples of its table size; wrap_chain -- ids whose probes
    start in the table's last three slots.  Similarities from a small set of values, so that equal sims meet on one id."""
    rng = np.random.default_rng(segs * 1000 + k + 7 * STRESS_KINDS.index(kind))
    counts = [3, segs, 2]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    T = table_size(segs * k)
    im = rng.integers(0, 50, size=N_REF_STRESS).astype(np.int32)
    matches = rng.integers(0, N_REF_STRESS, size=(int(off[-1]), k)).astype(np.int64)
    big = slice(off[1], off[2])
    if kind == "one_id":
        matches[big] = 123_457
    elif kind == "table_multiples":
        matches[big] = T * rng.integers(0, N_REF_STRESS // T, size=(segs, k))
    else:
        matches[big] = rng.choice(wrap_ids(T), size=(segs, k))
    matches[:3, 0] = matches[off[1], 0]                  # the small images list ids of the large one: no interaction
    sims = rng.choice(np.array([0.125, 0.5, 0.75, 1.0, 1.5], np.float32), size=matches.shape)
    sims[off[1] + segs // 2, k // 2] = np.float32(1.75)  # one entry above all the others
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)


def no_duplicates_case():
    """Lists in which no id appears twice in a query image (invalid ids appear often): the flag blanks nothing."""
    rng = np.random.default_rng(77)
    counts = [3, 40, 0, 90]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    k = 50
    im = rng.integers(0, 60, size=20_000).astype(np.int32)
    matches = rng.permutation(20_000)[:int(off[-1]) * k].reshape(-1, k).astype(np.int64)
    matches[rng.random(matches.shape) < 0.05] = -1
    matches[rng.random(matches.shape) < 0.02] = 20_000
    sims = rng.uniform(0.2, 1.9, size=matches.shape).astype(np.float32)
    return dict(matches=matches, sims=sims, off=off, img_of_seg=im, k=k, counts=counts)
