"""NumPy reference of segvlad_sequence_rerank: a literal restatement of the contract in include/segvlad.h, never the code under
test.  Vectorised over the slots and the velocities of a frame; the frames t and the offsets tau are Python loops, so every
accumulator takes its additions in the contract's order (``acc = np.where(hit, acc + sup, acc)``: NumPy adds fp64 values one
operation at a time and never fuses)."""
import numpy as np


def empty_slots(cand, score):
    """[T][C] bool: cand < 0 or a score that is not finite."""
    return (np.asarray(cand) < 0) | ~np.isfinite(np.asarray(score, dtype=np.float64))


def frame_order(seq_score, empty):
    """One frame's slots by (seq_score descending, slot ascending), a NaN sum behind every number, empty slots last in slot order."""
    def key(c):
        if empty[c]:
            return (1, 0, 0.0, c)
        s = float(seq_score[c])
        return (0, 1, 0.0, c) if s != s else (0, 0, -s, c)

    return np.array(sorted(range(len(empty)), key=key), dtype=np.int32)


def sequence_rerank(cand, score, seq_offsets=None, back=5, fwd=5, vel=(0.8, 0.9, 1.0, 1.1, 1.2), tol=1):
    """Returns {"seq_score" fp64, "n_hit" int32, "vel" int32, "order" int32}, each [T][C]."""
    cand = np.asarray(cand).astype(np.int64)
    score = np.asarray(score, dtype=np.float64)
    T, C = cand.shape
    vel = np.asarray(vel, dtype=np.float64).reshape(-1)
    V = len(vel)
    so = [0, T] if seq_offsets is None else [int(x) for x in seq_offsets]
    empty = empty_slots(cand, score)
    out = {"seq_score": np.zeros((T, C), np.float64), "n_hit": np.zeros((T, C), np.int32), "vel": np.full((T, C), -1, np.int32),
           "order": np.zeros((T, C), np.int32)}
    with np.errstate(all="ignore"):
        for s in range(len(so) - 1):
            lo, hi = so[s], so[s + 1]
            for t in range(lo, hi):
                acc = np.zeros((C, V), np.float64)
                hits = np.zeros((C, V), np.int32)
                for tau in range(-back, fwd + 1):
                    if tau == 0:
                        acc = acc + score[t][:, None]
                        continue
                    tp = t + tau
                    if not lo <= tp < hi:
                        continue
                    p = cand[t][:, None] + np.rint(vel[None, :] * float(tau)).astype(np.int64)          # [C][V] int64
                    near = (np.abs(cand[tp][None, None, :] - p[:, :, None]) <= tol) & ~empty[tp][None, None, :]   # [C][V][C']
                    hit = near.any(axis=2)
                    sup = np.where(near, score[tp][None, None, :], -np.inf).max(axis=2)
                    acc = np.where(hit, acc + sup, acc)
                    hits = hits + hit
                best, bh, bu = acc[:, 0].copy(), hits[:, 0].copy(), np.zeros(C, np.int32)
                for u in range(1, V):   # the largest acc, ties to the lowest u
                    better = acc[:, u] > best
                    best, bh, bu = np.where(better, acc[:, u], best), np.where(better, hits[:, u], bh), np.where(better, u, bu)
                out["seq_score"][t] = np.where(empty[t], 0.0, best)
                out["n_hit"][t] = np.where(empty[t], 0, bh)
                out["vel"][t] = np.where(empty[t], -1, bu)
                out["order"][t] = frame_order(out["seq_score"][t], empty[t])
    return out


def planted_case(v_true, seed=0, T=40, C=8):
    """The planted traversal of the tests: frame t's true place 5000 + floor(v_true t) at a random slot with score 1.0; the other
    slots are distractors 1 000 000 + 10 000 t + 100 j -- no two within reach of one line --, one of them with score 1.5, the
    rest below 1.  Returns (cand int32 [T][C], score fp64 [T][C], true_slot [T])."""
    rng = np.random.default_rng(seed)
    cand = (1_000_000 + 10_000 * np.arange(T)[:, None] + 100 * np.arange(C)[None, :]).astype(np.int32)
    score = rng.integers(1, 8, (T, C)) / 8.0                      # (eighths: every sum of the case is exact)
    slot = rng.integers(0, C, T)
    loud = (slot + rng.integers(1, C, T)) % C                     # another slot
    score[np.arange(T), loud] = 1.5
    cand[np.arange(T), slot] = 5000 + np.floor(v_true * np.arange(T)).astype(np.int64)
    score[np.arange(T), slot] = 1.0
    return cand, score, slot
