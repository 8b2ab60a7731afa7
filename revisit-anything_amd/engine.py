"""SegVLADEngine: thin object wrapper over the C-ABI (include/segvlad.h) for PyTorch-ROCm host code.

PyTorch is plumbing here: device memory (tensors handed over as raw pointers), the current HIP
stream, and -- in sharded.py -- torch.distributed.  All arithmetic happens in libsegvlad_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import SegVLADDegenerateError, SegVLADError
from .rle import RLE_CHUNK_RUNS, RLE_ENCODE_ROWS, RleMasks  # noqa: F401  (the kernels' chunk of runs and rows of a unit, for callers and tests)


def _ptr(x) -> int:
    """Raw address of a torch tensor (host or device) or a NumPy array; None -> NULL."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data
    raise TypeError(f"unsupported buffer type {type(x)}")


def _as(x, dtype_np, dtype_t):
    """Coerce to a contiguous array/tensor of the wanted dtype without moving it between host/device."""
    if isinstance(x, torch.Tensor):
        return x.to(dtype_t).contiguous()
    return np.ascontiguousarray(x, dtype=dtype_np)


def pad_shortlists(lists, M: Optional[int] = None) -> np.ndarray:
    """Ragged per-image shortlists (a sequence of sequences of reference image ids) -> the padded ``int32 [n_img][M]`` array
    of segvlad_search_shortlist: each row's ids in their given order, then -1.  M defaults to the longest list (at least 1)."""
    rows = [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
    longest = max((len(r) for r in rows), default=0)
    M = max(1, longest) if M is None else int(M)
    if longest > M:
        raise ValueError(f"a shortlist holds {longest} ids, more than M={M}")
    out = np.full((len(rows), M), -1, dtype=np.int32)
    for b, r in enumerate(rows):
        if r.size and (r.min() < np.iinfo(np.int32).min or r.max() > np.iinfo(np.int32).max):
            raise ValueError(f"shortlist {b}: id out of the int32 range")
        out[b, :len(r)] = r
    return out


def check_shortlist(shortlist: np.ndarray, n_img: int, n_img_ref: int) -> None:
    """Host-side validation of a padded shortlist: shape [n_img][M] with 1 <= M <= 4096, ids in -1 .. n_img_ref - 1
    (-1 is padding); raises ValueError otherwise."""
    if shortlist.ndim != 2 or shortlist.shape[0] != n_img:
        raise ValueError(f"shortlist must be [n_img={n_img}][M], got shape {tuple(shortlist.shape)}")
    if not 1 <= shortlist.shape[1] <= 4096:
        raise ValueError(f"shortlist width M={shortlist.shape[1]} outside 1 .. 4096")
    if shortlist.size:
        lo, hi = int(shortlist.min()), int(shortlist.max())
        if lo < -1:
            raise ValueError(f"shortlist id {lo} < -1 (-1 is the only padding value)")
        if hi >= n_img_ref:
            raise ValueError(f"shortlist id {hi} >= the number of reference images {n_img_ref}")


MAX_CANDIDATES = 64   # C of segvlad_match_pairs


def pad_candidates(lists, C: Optional[int] = None) -> np.ndarray:
    """Ragged per-image candidate lists (a sequence of sequences of reference image ids, best first) -> the padded
    ``int32 [n_img][C]`` array of segvlad_match_pairs: each row's ids in their given order, then -1.  C defaults to the longest
    list (at least 1); more than 64 raise ValueError."""
    rows = [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
    longest = max((len(r) for r in rows), default=0)
    C = max(1, longest) if C is None else int(C)
    if not 1 <= C <= MAX_CANDIDATES:
        raise ValueError(f"C={C} candidates per image outside 1 .. {MAX_CANDIDATES}")
    if longest > C:
        raise ValueError(f"a candidate list holds {longest} ids, more than C={C}")
    out = np.full((len(rows), C), -1, dtype=np.int32)
    info = np.iinfo(np.int32)
    for b, r in enumerate(rows):
        if r.size and (r.min() < info.min or r.max() > info.max):
            raise ValueError(f"candidate list {b}: id out of the int32 range")
        out[b, :len(r)] = r
    return out


def check_candidates(cand: np.ndarray, n_img: int) -> None:
    """Host-side validation of a padded candidate array: integers, shape [n_img][C] with 1 <= C <= 64, ids in -1 .. 2^31 - 1
    (-1 is padding; an id no row carries is allowed and behaves like padding); raises ValueError otherwise."""
    cand = np.asarray(cand)
    if cand.dtype.kind not in "iu":
        raise ValueError(f"candidates must be integers, got dtype {cand.dtype}")
    if cand.ndim != 2 or cand.shape[0] != n_img:
        raise ValueError(f"candidates must be [n_img={n_img}][C], got shape {tuple(cand.shape)}")
    if not 1 <= cand.shape[1] <= MAX_CANDIDATES:
        raise ValueError(f"candidate width C={cand.shape[1]} outside 1 .. {MAX_CANDIDATES}")
    if cand.size:
        lo, hi = int(cand.min()), int(cand.max())
        if lo < -1:
            raise ValueError(f"candidate id {lo} < -1 (-1 is the only padding value)")
        if hi > np.iinfo(np.int32).max:
            raise ValueError(f"candidate id {hi} out of the int32 range")


MAX_SEQ_WINDOW = 32       # back / fwd of segvlad_sequence_rerank
MAX_SEQ_VELOCITIES = 16   # its n_vel
MAX_SEQ_VELOCITY = float(2 ** 20)
MAX_SEQ_TOL = 2 ** 30


def velocity_grid(vmin: float = 0.8, vmax: float = 1.2, n: int = 5) -> np.ndarray:
    """``n`` evenly spaced velocities (map frames per query frame) from ``vmin`` to ``vmax``, both included, as the fp64 array
    of segvlad_sequence_rerank; n == 1 gives ``[vmin]``.  Negative values describe a reverse traversal."""
    n = int(n)
    if not 1 <= n <= MAX_SEQ_VELOCITIES:
        raise ValueError(f"n={n} velocities outside 1 .. {MAX_SEQ_VELOCITIES}")
    vmin, vmax = float(vmin), float(vmax)
    if not (np.isfinite(vmin) and np.isfinite(vmax)) or max(abs(vmin), abs(vmax)) > MAX_SEQ_VELOCITY or vmin > vmax:
        raise ValueError(f"need finite vmin <= vmax within +-2^20, got {vmin}, {vmax}")
    return np.linspace(vmin, vmax, n, dtype=np.float64)


def check_sequence_args(T: int, C: int, seq_offsets=None, back: int = 5, fwd: int = 5, velocities=None, tol: int = 1):
    """Host-side validation of segvlad_sequence_rerank's arguments beside the lists [T][C]: raises ValueError for what the C
    call would reject.  Returns ``(seq_offsets, velocities)`` as the int32 / fp64 host arrays the call takes
    (``seq_offsets=None``: one sequence; ``velocities=None``: velocity_grid())."""
    T, C = int(T), int(C)
    if T < 0 or not 1 <= C <= MAX_CANDIDATES:
        raise ValueError(f"need T >= 0 and 1 <= C <= {MAX_CANDIDATES}, got T={T}, C={C}")
    so = np.array([0, T], dtype=np.int64) if seq_offsets is None else np.asarray(seq_offsets)
    if so.dtype.kind not in "iu" or so.ndim != 1:
        raise ValueError("seq_offsets must be a 1-D array of integers")
    if len(so) < 1 or so[0] != 0 or so[-1] != T or (np.diff(so.astype(np.int64)) < 0).any():
        raise ValueError(f"seq_offsets must run from 0 to T={T} and never decrease")
    for name, w in (("back", back), ("fwd", fwd)):
        if int(w) != w or not 0 <= int(w) <= MAX_SEQ_WINDOW:
            raise ValueError(f"{name}={w} outside 0 .. {MAX_SEQ_WINDOW}")
    if int(tol) != tol or not 0 <= int(tol) <= MAX_SEQ_TOL:
        raise ValueError(f"tol={tol} outside 0 .. 2^30 (map frames, an integer)")
    vel = velocity_grid() if velocities is None else np.ascontiguousarray(velocities, dtype=np.float64)
    if vel.ndim != 1 or not 1 <= len(vel) <= MAX_SEQ_VELOCITIES:
        raise ValueError(f"velocities must be a 1-D array of 1 .. {MAX_SEQ_VELOCITIES} values, got shape {tuple(vel.shape)}")
    if not np.isfinite(vel).all() or np.abs(vel).max() > MAX_SEQ_VELOCITY:
        raise ValueError("every velocity must be finite and within +-2^20")
    return np.ascontiguousarray(so, dtype=np.int32), vel


MAX_VERIFY_ROWS = 256   # rows per query image of segvlad_verify_pairs


def _is_integral(x) -> bool:
    """Integers or booleans, as a tensor, an array or anything NumPy makes an array of?"""
    if isinstance(x, torch.Tensor):
        return not (x.dtype.is_floating_point or x.dtype.is_complex)
    return np.asarray(x).dtype.kind in "iub"


MAX_EXCLUDE_INTERVALS = 8   # E of segvlad_search_excluding


def pad_intervals(lists, E: Optional[int] = None) -> np.ndarray:
    """Ragged per-image exclusion intervals (a sequence, per query image, of ``(lo, hi)`` pairs of reference image ids, both
    ends inclusive) -> the padded ``int32 [n_img][E][2]`` array of segvlad_search_excluding: each image's intervals in their
    given order, then empty ones ``(0, -1)``.  E defaults to the longest list (at least 1); more than 8 raise ValueError."""
    rows = []
    for b, x in enumerate(lists):
        r = np.asarray(x, dtype=np.int64)
        if r.size == 0:
            r = r.reshape(0, 2)
        if r.ndim != 2 or r.shape[1] != 2:
            raise ValueError(f"image {b}: intervals must be (lo, hi) pairs, got shape {tuple(r.shape)}")
        rows.append(r)
    longest = max((len(r) for r in rows), default=0)
    E = max(1, longest) if E is None else int(E)
    if not 1 <= E <= MAX_EXCLUDE_INTERVALS:
        raise ValueError(f"E={E} intervals per image outside 1 .. {MAX_EXCLUDE_INTERVALS}")
    if longest > E:
        raise ValueError(f"an image holds {longest} intervals, more than E={E}")
    out = np.empty((len(rows), E, 2), dtype=np.int32)
    out[:, :, 0] = 0
    out[:, :, 1] = -1
    info = np.iinfo(np.int32)
    for b, r in enumerate(rows):
        if r.size and (r.min() < info.min or r.max() > info.max):
            raise ValueError(f"image {b}: id out of the int32 range")
        out[b, :len(r)] = r
    return out


def window_intervals(frame_ids, radius: int) -> np.ndarray:
    """The exclusion array of a self-query: query image i is frame ``frame_ids[i]`` of the map, and must not match the frames
    ``frame_ids[i] - radius .. frame_ids[i] + radius`` (radius 0: itself only).  ``int32 [n_img][1][2]``."""
    f = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
    radius = int(radius)
    if radius < 0:
        raise ValueError(f"radius={radius} < 0")
    info = np.iinfo(np.int32)
    lo, hi = f - radius, f + radius
    if f.size and (lo.min() < info.min or hi.max() > info.max):
        raise ValueError("frame id +- radius out of the int32 range")
    return np.stack([lo, hi], axis=1).astype(np.int32).reshape(-1, 1, 2)


def merge_intervals(intervals) -> list:
    """One image's ``(lo, hi)`` intervals with the empty ones (lo > hi) dropped, sorted, and overlapping or adjacent ones joined
    -- what segvlad_search_excluding makes of them (there after clamping to the ids the index holds)."""
    iv = sorted((int(lo), int(hi)) for lo, hi in np.asarray(intervals, dtype=np.int64).reshape(-1, 2) if lo <= hi)
    out = []
    for lo, hi in iv:
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


def excluded_rows(exclude, rows_per_image) -> np.ndarray:
    """X_b of segvlad_search_excluding on the host: per query image the number of index rows its intervals cover, from
    ``rows_per_image`` (rows of reference image 0, 1, ...).  ``exclude``: ``[n_img][E][2]``.  The inner search runs at depth
    ``min(1024, k + max X_b)``; an image with ``k + X_b <= 1024`` never needs the exact tail."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(rows_per_image, dtype=np.int64))])
    n = len(cum) - 1
    ex = np.asarray(exclude, dtype=np.int64)
    out = np.zeros(len(ex), dtype=np.int64)
    for b in range(len(ex)):
        for lo, hi in merge_intervals(ex[b]):
            lo, hi = max(lo, 0), min(hi, n - 1)
            if lo <= hi:
                out[b] += cum[hi + 1] - cum[lo]
    return out


def check_intervals(exclude: np.ndarray, n_img: int) -> None:
    """Host-side validation of an exclusion array: shape [n_img][E][2] with 1 <= E <= 8; raises ValueError otherwise."""
    if exclude.ndim != 3 or exclude.shape[0] != n_img or exclude.shape[2] != 2:
        raise ValueError(f"exclude must be [n_img={n_img}][E][2], got shape {tuple(exclude.shape)}")
    if not 1 <= exclude.shape[1] <= MAX_EXCLUDE_INTERVALS:
        raise ValueError(f"exclude holds E={exclude.shape[1]} intervals per image, outside 1 .. {MAX_EXCLUDE_INTERVALS}")
    if exclude.size:
        info = np.iinfo(np.int32)
        if int(exclude.min()) < info.min or int(exclude.max()) > info.max:
            raise ValueError("exclude: id out of the int32 range")


def radius2_from_sim(sim):
    """Squared radius of a similarity floor: the reference turns distances into similarities with ``2 - d^2`` (unit rows), so
    ``sim > s`` is ``d^2 < 2 - s``.  Scalar or array; fp32."""
    out = np.float32(2.0) - np.asarray(sim, dtype=np.float32)
    return np.float32(out) if out.ndim == 0 else out.astype(np.float32)


def range_from_topk(d2, idx, radius2):
    """Cut top-k lists at a radius: ``(lims, d2, idx)`` of the entries with ``d2 < radius2[q]`` (strictly), each row's in
    list order -- what segvlad_range_search returns when the lists are deep enough.  ``d2`` / ``idx``: ``[nq][k]`` ascending
    lists as search() returns them ((+inf, -1) beyond the index); ``radius2``: scalar or ``[nq]``.  A NaN, zero or negative
    radius yields no hit.  Raises ValueError when a row's list is full (its last slot holds a row) and its last entry is still
    below the radius: the list was too shallow to decide."""
    d2 = np.asarray(d2, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    if d2.ndim != 2 or idx.shape != d2.shape:
        raise ValueError(f"d2 / idx must be [nq][k] of one shape, got {d2.shape} and {idx.shape}")
    nq, k = d2.shape
    r = np.broadcast_to(np.asarray(radius2, dtype=np.float32), (nq,)) if np.ndim(radius2) == 0 else np.asarray(radius2, dtype=np.float32)
    if r.shape != (nq,):
        raise ValueError(f"radius2 must be a scalar or [nq={nq}], got shape {r.shape}")
    with np.errstate(invalid="ignore"):
        hit = (d2 < r[:, None]) & (idx >= 0) & (r[:, None] > 0)
    if k > 0:
        shallow = np.nonzero(hit[:, k - 1])[0]
        if shallow.size:
            raise ValueError(f"range_from_topk: the lists of {shallow.size} rows (first: {int(shallow[0])}) are full and still below "
                             f"the radius at depth {k}: too shallow to decide")
    lims = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(hit.sum(1), out=lims[1:])
    return lims, d2[hit].astype(np.float32), idx[hit].astype(np.int64)


def range_image_counts(lims, idx, img_of_seg, qseg_offsets) -> list:
    """The count vote over a radius: per query image the reference images its rows hit and how many hits each --
    ``(image ids ascending int64, counts int64)``.  ``lims`` / ``idx``: a range result; ``img_of_seg [n_ref_seg]``: the image of
    every index row; ``qseg_offsets [n_img + 1]``: the query images' rows."""
    lims = np.asarray(lims, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    img = np.asarray(img_of_seg, dtype=np.int64)
    qo = np.asarray(qseg_offsets, dtype=np.int64)
    if qo.ndim != 1 or qo.size < 1 or qo[-1] + 1 != lims.size:
        raise ValueError("qseg_offsets must end at the number of query rows of lims")
    out = []
    for b in range(qo.size - 1):
        ids, cnt = np.unique(img[idx[lims[qo[b]]:lims[qo[b + 1]]]], return_counts=True)
        out.append((ids.astype(np.int64), cnt.astype(np.int64)))
    return out


def collapse_lists(d2, idx, img_of_seg, k: int, per_image: int = 1):
    """The rule of segvlad_search_grouped, stated on the host: ``d2`` / ``idx`` ``[nq][L]`` are ordered lists as search()
    returns them (ascending (d2, lower id); slots with ``idx < 0`` are padding and skipped), ``img_of_seg [n_ref_seg]`` the
    image id of every index row.  An entry is kept when fewer than ``per_image`` EARLIER entries of its row carry its image
    id; a row with a negative image id is a group of its own, always kept.  Returns ``(d2 [nq][k] fp32, idx [nq][k] int64)``:
    each row's first ``k`` kept entries in their order, (+inf, -1) behind them.  With unbounded lists (L = the index size)
    this IS the grouped search's result; with shorter ones, a row that neither fills its k slots nor meets a padding slot is
    undecided at that depth."""
    d2 = np.asarray(d2, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    img = np.asarray(img_of_seg, dtype=np.int64).reshape(-1)
    if d2.ndim != 2 or idx.shape != d2.shape:
        raise ValueError(f"d2 / idx must be [nq][L] of one shape, got {d2.shape} and {idx.shape}")
    if k < 1 or per_image < 1:
        raise ValueError("k and per_image must be >= 1")
    if idx.size and int(idx.max()) >= img.size:
        raise ValueError("idx names a row img_of_seg does not cover")
    nq = d2.shape[0]
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = np.nonzero(idx[q] >= 0)[0]
        g = img[idx[q, pos]]
        order = np.argsort(g, kind="stable")               # equal ids stay in list order
        gs = g[order]
        first = np.r_[True, gs[1:] != gs[:-1]] if gs.size else np.zeros(0, bool)
        run_start = np.maximum.accumulate(np.where(first, np.arange(gs.size), 0)) if gs.size else gs
        earlier = np.empty(gs.size, dtype=np.int64)
        earlier[order] = np.arange(gs.size) - run_start    # earlier entries of the same image
        kept = pos[(g < 0) | (earlier < per_image)][:k]
        out_d[q, :kept.size] = d2[q, kept]
        out_i[q, :kept.size] = idx[q, kept]
    return out_d, out_i


def blank_capped(idx, img_of_seg, per_image: int) -> np.ndarray:
    """The rule of segvlad_vote's per-image cap (SEGVLAD_VOTE_PER_IMAGE), stated on the host for callers that already hold
    lists: ``idx [nq][k]`` int64, ``img_of_seg [n_ref_seg]``.  An entry is valid when ``0 <= idx < n_ref_seg``; it votes when
    fewer than ``per_image`` valid entries at EARLIER ranks of its row carry its image id (ids compare as 32-bit values,
    negative ones included).  Returns a copy of ``idx`` with every valid entry that does not vote set to -1: the plain vote over
    it is the capped vote over ``idx``.  Unlike collapse_lists() nothing moves up into the blanked slots."""
    idx = np.asarray(idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64)
    img = np.asarray(img_of_seg.detach().cpu().numpy() if isinstance(img_of_seg, torch.Tensor) else img_of_seg).reshape(-1)
    if idx.ndim != 2:
        raise ValueError(f"idx must be [nq][k], got {idx.shape}")
    if isinstance(per_image, bool) or int(per_image) != per_image or not 1 <= int(per_image) <= 255:
        raise ValueError(f"per_image must be an integer in 1 .. 255, got {per_image!r}")
    out = idx.copy()
    if idx.size == 0:
        return out
    nq, k = idx.shape
    valid = (idx >= 0) & (idx < img.size)
    g = img.astype(np.int64)[np.where(valid, idx, 0)]
    # one stable sort of every row by (invalid last, image id): an entry's position inside its image's run is the number of
    # earlier valid entries of the row that carry the image
    order = np.lexsort((g, ~valid), axis=1)
    gs = np.take_along_axis(g, order, 1)
    pos = np.broadcast_to(np.arange(k), (nq, k))
    first = np.ones((nq, k), bool)
    first[:, 1:] = gs[:, 1:] != gs[:, :-1]
    earlier_sorted = pos - np.maximum.accumulate(np.where(first, pos, 0), axis=1)
    earlier = np.empty((nq, k), np.int64)
    np.put_along_axis(earlier, order, earlier_sorted, 1)
    out[valid & (earlier >= int(per_image))] = -1
    return out


def blank_unique(idx, sims, qseg_offsets, n_ref_seg: int) -> np.ndarray:
    """The rule of segvlad_vote's one-to-one flag (SEGVLAD_VOTE_UNIQUE_REF), stated on the host: ``idx [nq][k]`` int64, ``sims
    [nq][k]`` float32 or None, ``qseg_offsets [n_img + 1]``.  An entry is valid when ``0 <= idx < n_ref_seg``.  Among the valid
    entries of one query image that carry the same id one wins: the largest sim (a NaN loses to every number, -0.0 == +0.0),
    then -- on a tie, or without ``sims`` -- the first in the vote's visiting order (rank-major, then segment).  Returns a copy of
    ``idx`` with every other valid entry set to -1: the plain vote over it is the flagged vote over ``idx``.  A per-image cap in
    the same mode word is applied behind it: blank_capped(blank_unique(...), img_of_seg, m)."""
    idx = np.asarray(idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64)
    if idx.ndim != 2:
        raise ValueError(f"idx must be [nq][k], got {idx.shape}")
    if sims is not None:
        sims = np.asarray(sims.detach().cpu().numpy() if isinstance(sims, torch.Tensor) else sims, dtype=np.float32)
        if sims.shape != idx.shape:
            raise ValueError(f"sims must have idx's shape {idx.shape}, got {sims.shape}")
    off = np.asarray(qseg_offsets, dtype=np.int64).reshape(-1)
    out = idx.copy()
    for b in range(len(off) - 1):
        rows = slice(off[b], off[b + 1])
        ids = idx[rows].T.reshape(-1)                        # visiting order: position p
        pos = np.nonzero((ids >= 0) & (ids < n_ref_seg))[0]
        if len(pos) == 0:
            continue
        if sims is None:
            order = np.lexsort((pos, ids[pos]))
        else:
            s = sims[rows].T.reshape(-1)[pos]
            nan = np.isnan(s)
            order = np.lexsort((pos, -np.where(nan, np.float32(0), s), nan, ids[pos]))   # by id; numbers first, descending; then p
        sorted_ids = ids[pos][order]
        lose = np.ones(len(pos), bool)
        lose[order[np.concatenate([[True], sorted_ids[1:] != sorted_ids[:-1]])]] = False
        view = out[rows].T.reshape(-1)                       # (a copy: the transpose of a slice is not contiguous)
        view[pos[lose]] = -1
        out[rows] = view.reshape(idx.shape[1], -1).T
    return out


def vlad_assign_value(mode: str = "hard", temp=None) -> str:
    """The value of the option ``vlad_assign`` for ``mode`` in {'hard', 'soft', 'soft_pooled'}: 'hard', or 'soft:<T>' /
    'soft_pooled:<T>' with T printed so that it reads back as the same fp32.  Refuses what segvlad_set_option refuses: another mode, a temperature with 'hard', and a soft
    temperature that is missing, not a number, not finite as fp32, or <= 0."""
    if mode == "hard":
        if temp is not None:
            raise ValueError("vlad_assign: hard assignment takes no temperature")
        return "hard"
    if not isinstance(mode, str) or mode not in ("soft", "soft_pooled"):
        raise ValueError(f"vlad_assign: mode must be 'hard', 'soft' or 'soft_pooled', got {mode!r}")
    if temp is None or isinstance(temp, (bool, str, bytes)):
        raise ValueError(f"vlad_assign: soft assignment needs a temperature, got {temp!r}")
    try:
        with np.errstate(over="ignore"):
            t = np.float32(temp)
    except (TypeError, ValueError):
        raise ValueError(f"vlad_assign: the temperature must be a number, got {temp!r}") from None
    if not np.isfinite(t) or not t > 0:
        raise ValueError(f"vlad_assign: the temperature must be a finite fp32 > 0, got {temp!r}")
    return mode + ":" + np.format_float_scientific(t, unique=True, trim="0")


BURST_RANGES = ((0.0, 64.0), (-8.0, 16.0), (0.0, 2.0))   # of a, b, p of the option vlad_burst (include/segvlad.h)


def vlad_burst_value(a, b, p) -> str:
    """The value ``<a>:<b>:<p>`` of the option ``vlad_burst``, every field printed so that it reads back as the same fp32.  Refuses
    what segvlad_set_option refuses: a field that is missing, not a number, not finite as fp32, or outside 0 <= a <= 64,
    -8 <= b <= 16, 0 <= p <= 2."""
    fields = []
    for name, x, (lo, hi) in zip("abp", (a, b, p), BURST_RANGES):
        if x is None or isinstance(x, (bool, str, bytes)) or np.ndim(x) != 0:
            raise ValueError(f"vlad_burst: {name} must be a number, got {x!r}")
        try:
            with np.errstate(over="ignore"):
                v = np.float32(x)
        except (TypeError, ValueError):
            raise ValueError(f"vlad_burst: {name} must be a number, got {x!r}") from None
        if not np.isfinite(v) or not lo <= v <= hi:
            raise ValueError(f"vlad_burst: {name} must be a finite fp32 in [{lo:g}, {hi:g}], got {x!r}")
        fields.append(np.format_float_scientific(v, unique=True, trim="0"))
    return ":".join(fields)


def burst_reference(tokens, a, b, p):
    """The definition of ``vlad_burst=<a>:<b>:<p>`` (include/segvlad.h) for ONE image, in NumPy fp64: ``tokens [D][N]`` as the engine
    takes them, ALL of them, covered by a segment or not.

        g[n] = sum_{m < N} sigmoid(a (2 <x^_n, x^_m> - 2) + b)        (m = n included; an all-zero token has x^ = 0: cosine 0)
        u[n] = g[n]^-p

    Returns ``(g [N], u [N])``."""
    X = np.asarray(tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else tokens).astype(np.float64).T
    if X.ndim != 2:
        raise ValueError(f"burst_reference: tokens [D][N], got {X.T.shape}")
    xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
    z = float(a) * (2.0 * (xh @ xh.T) - 2.0) + float(b)
    g = (1.0 / (1.0 + np.exp(-z))).sum(axis=1)
    return g, g ** (-float(p))


BURST_SCOPES = ("image", "segment")   # of the option vlad_burst_scope (include/segvlad.h)


def burst_segment_reference(tokens, inc, adj, a, b, p):
    """The definition of ``vlad_burst=<a>:<b>:<p>`` under ``vlad_burst_scope=segment`` (include/segvlad.h) for ONE image, in NumPy
    fp64: ``tokens [D][N]`` as the engine takes them, ``inc [S][N]`` bool incidence, ``adj [S][S]`` or None (order 0).

        U(s)    = the tokens of segment s after the neighbour union, (adj . inc) > 0
        g[s][n] = sum_{m in U(s)} sigmoid(a (2 <x^_n, x^_m> - 2) + b)      n in U(s), m = n included (an all-zero token: cosine 0)
        u[s][n] = g[s][n]^-p                                               0 outside U(s)

    Returns ``(g [S][N], u [S][N])``, both 0 outside U(s)."""
    X = np.asarray(tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else tokens).astype(np.float64).T
    inc = np.asarray(inc.detach().cpu().numpy() if isinstance(inc, torch.Tensor) else inc).astype(bool)
    if X.ndim != 2 or inc.ndim != 2 or inc.shape[1] != X.shape[0]:
        raise ValueError(f"burst_segment_reference: tokens [D][N] and inc [S][N], got {X.T.shape} and {inc.shape}")
    S = inc.shape[0]
    if adj is not None:
        adj = np.asarray(adj.detach().cpu().numpy() if isinstance(adj, torch.Tensor) else adj).astype(np.float64).reshape(S, S)
    U = inc if adj is None else (adj @ inc.astype(np.float64)) > 0
    xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
    z = float(a) * (2.0 * (xh @ xh.T) - 2.0) + float(b)
    g = (U.astype(np.float64) @ (1.0 / (1.0 + np.exp(-z)))) * U          # [S][N]: row s sums the columns m in U(s)
    u = np.zeros_like(g)
    u[U] = g[U] ** (-float(p))
    return g, u


def soft_vlad_reference(tokens, centres, inc, adj=None, temp: float = 1.0, parts: bool = False, pooled: bool = False, burst=None,
                        burst_scope: str = "image"):
    """The definition of ``vlad_assign=soft:<T>`` (include/segvlad.h; utilities.py:862-887) for ONE image, in NumPy fp64:
    ``tokens [D][N]`` as the engine takes them, ``centres [K][D]`` raw, ``inc [S][N]`` bool incidence, ``adj [S][S]`` or None
    (order 0), ``temp`` = T.

        w[n][k] = softmax_k(T <x^_n, c^_k>)                          max-subtracted, over the K centres
        V[s][k] = sum_{n in U(s)} w[n][k] x^_n - (sum_{n in U(s)} w[n][k]) c_k       U(s) = tokens of (adj . inc)[s] > 0
        out[s]  = L2(concat_k intra_norm(V[s][k]))                   both divide by max(norm, 1e-12)

    ``pooled``: the definition of ``vlad_assign=soft_pooled:<T>``, what the reference's ``VLAD.generate`` computes -- block k holds
    the residuals against ALL centres, ``V[s][k] = K sum_n w[n][k] x^_n - (sum_n w[n][k]) sum_c c_c`` (utilities.py:883-884).

    ``burst``: None, or ``(a, b, p)`` of the option ``vlad_burst`` -- every row of w is multiplied by ``u[n]`` of ``burst_reference``
    (the returned ``w`` holds the discounted weights).  ``burst_scope='segment'``: the option ``vlad_burst_scope`` -- the incidence
    of (segment, token) is multiplied by ``u[s][n]`` of ``burst_segment_reference`` instead, and ``w`` stays the softmax.

    Returns ``out [S][K*D]``; with ``parts`` a dict that also holds ``w [N][K]`` and ``block_norms [S][K]``."""
    def host(x):
        return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x)

    X = host(tokens).astype(np.float64).T                       # [N][D]
    Cm = host(centres).astype(np.float64)                       # [K][D]
    inc = host(inc).astype(bool)
    if X.ndim != 2 or Cm.ndim != 2 or X.shape[1] != Cm.shape[1] or inc.ndim != 2 or inc.shape[1] != X.shape[0]:
        raise ValueError(f"soft_vlad_reference: tokens [D][N], centres [K][D], inc [S][N]; got {X.T.shape}, {Cm.shape}, {inc.shape}")
    if not (np.isfinite(temp) and temp > 0):
        raise ValueError(f"soft_vlad_reference: temp must be finite and > 0, got {temp!r}")
    S, (K, D) = inc.shape[0], Cm.shape
    xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
    ch = Cm / np.maximum(np.linalg.norm(Cm, axis=1, keepdims=True), 1e-12)
    z = float(temp) * (xh @ ch.T)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)                        # [N][K]
    if burst_scope not in BURST_SCOPES:
        raise ValueError(f"soft_vlad_reference: burst_scope must be one of {BURST_SCOPES}, got {burst_scope!r}")
    if burst is not None and burst_scope == "image":
        w = w * burst_reference(X.T, *burst)[1][:, None]
    U = inc if adj is None else (host(adj).astype(np.float64).reshape(S, S) @ inc.astype(np.float64)) > 0
    Uf = U.astype(np.float64)
    if burst is not None and burst_scope == "segment":
        Uf = burst_segment_reference(X.T, inc, None if adj is None else host(adj), *burst)[1]
    V = np.einsum("sn,nk,nd->skd", Uf, w, xh, optimize=True)
    V = K * V - (Uf @ w)[:, :, None] * Cm.sum(0)[None, None] if pooled else V - (Uf @ w)[:, :, None] * Cm[None]
    bn = np.linalg.norm(V, axis=2)                              # [S][K]
    V = V / np.maximum(bn, 1e-12)[:, :, None]
    out = V.reshape(S, K * D)
    out = out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
    return {"out": out, "w": w, "block_norms": bn} if parts else out


def expand_radius2(radius2, nq: int, qseg_offsets=None) -> np.ndarray:
    """``radius2`` of range_search as one fp32 value per query row: a scalar, ``[nq]``, or -- with ``qseg_offsets`` --
    ``[n_img]`` (repeated over each image's rows).  Raises ValueError on any other shape."""
    r = np.asarray(radius2.detach().cpu().numpy() if isinstance(radius2, torch.Tensor) else radius2, dtype=np.float32)
    if r.ndim == 0:
        return np.full(nq, r, dtype=np.float32)
    if qseg_offsets is not None:
        qo = np.asarray(qseg_offsets, dtype=np.int64)
        if qo.ndim != 1 or qo.size < 1 or qo[0] != 0 or qo[-1] != nq or np.any(np.diff(qo) < 0):
            raise ValueError(f"qseg_offsets must rise from 0 to nq={nq}")
        if r.shape == (qo.size - 1,) and r.shape != (nq,):
            return np.repeat(r, np.diff(qo)).astype(np.float32)
        if r.shape != (nq,):
            raise ValueError(f"radius2 must be a scalar, [nq={nq}] or [n_img={qo.size - 1}], got shape {r.shape}")
        return np.ascontiguousarray(r)
    if r.shape != (nq,):
        raise ValueError(f"radius2 must be a scalar or [nq={nq}], got shape {r.shape}")
    return np.ascontiguousarray(r)


class SegVLADEngine:
    """One context per (device, stream user).  Not thread-safe (the C context is not re-entrant)."""

    def __init__(self, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise SegVLADError("SegVLADEngine needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.device = dev
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.segvlad_create(C.byref(h), dev.index or 0)
        if rc != 0:
            raise SegVLADError(f"segvlad_create(device={dev.index}) failed with {rc}")
        self._h = h
        self.K = self.D = 0
        self.P = self.KD = 0
        self.vocab_generation = 0   # bumped by every set_vocab / pca_set: lets callers cache "my model is resident"
        self.pca_generation = 0
        self._keep = []  # tensors that must outlive async kernels of the last call
        self.n_img_ref = 0   # 1 + the largest img_of_seg id given to db_add since the last db_reset
        self.vlad_assign = "hard"   # the value of the option vlad_assign as last set through set_vlad_assign / set_option
        self.vlad_burst = "off"     # ... of the option vlad_burst (set_vlad_burst / set_option)
        self.vlad_burst_scope = "image"   # ... of the option vlad_burst_scope (set_vlad_burst_scope / set_option)

    # ---- plumbing ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.segvlad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.segvlad_last_error(self._h)
            raise SegVLADError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}", code=int(rc))

    def _stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.lib.segvlad_set_stream(self._h, C.c_void_p(s))

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def synchronize(self):
        self._stream()
        self._check(self.lib.segvlad_synchronize(self._h), "synchronize")

    def set_profiling(self, on: bool):
        self.lib.segvlad_set_profiling(self._h, int(on))

    def profile_reset(self):
        self.lib.segvlad_profile_reset(self._h)

    def set_option(self, key: str, value):
        """segvlad_set_option: arithmetic / tuning switches of this context (see include/segvlad.h)."""
        self._check(self.lib.segvlad_set_option(self._h, str(key).encode(), str(value).encode()), f"set_option({key})")
        if key == "vlad_assign":
            self.vlad_assign = str(value)
        if key == "vlad_burst":
            self.vlad_burst = str(value)
        if key == "vlad_burst_scope":
            self.vlad_burst_scope = str(value)

    def set_vlad_assign(self, mode: str = "hard", temp=None) -> str:
        """Option ``vlad_assign`` (include/segvlad.h): ``'hard'``, or ``'soft'`` / ``'soft_pooled'`` with the temperature of
        ``softmax_k(temp * cos(x_n, c_k))``.  ``'soft'`` takes block k's residuals against c_k; ``'soft_pooled'`` against all
        centres, which is what the reference's ``VLAD(vlad_mode='soft', soft_temp=...)`` computes.  Holds for every later
        seg_vlad / seg_vlad_pca / describe* of this context; kmeans_step and cluster_aggregate ignore it.  Returns the value that
        was in force before, in the form set_option takes (for callers that restore it).

        That value is this object's own record (``self.vlad_assign``: 'hard' at creation, updated by its ``set_option``); the C
        interface has no getter for options.  An option given to the context behind this object's back -- another wrapper on the
        same handle -- is not seen, and a restore then puts back what THIS object last set."""
        value = vlad_assign_value(mode, temp)
        before = self.vlad_assign
        self.set_option("vlad_assign", value)
        return before

    def set_vlad_burst(self, params=None) -> str:
        """Option ``vlad_burst`` (include/segvlad.h): None switches it off, ``(a, b, p)`` multiplies every token's assignment weight
        by ``g[n]^-p``, ``g[n] = sum_m sigmoid(a (2 cos(x_n, x_m) - 2) + b)`` over ALL tokens of the token's image (the fixed
        test-time setting of the burst-aware aggregator is ``(8, 7, 1)``).  Holds for every later seg_vlad / seg_vlad_pca / describe* of
        this context under hard and soft assignment alike; kmeans_step and cluster_aggregate ignore it.  Hard assignment with the
        discount aggregates from a one-hot weight buffer on the soft path's kernel: K times the hard aggregation's matrix work.
        Returns the value that was in force before, in the form set_option takes (this object's own record, like set_vlad_assign's)."""
        value = "off" if params is None else vlad_burst_value(*params)
        before = self.vlad_burst
        self.set_option("vlad_burst", value)
        return before

    def set_vlad_burst_scope(self, scope: str = "image") -> str:
        """Option ``vlad_burst_scope`` (include/segvlad.h): over which tokens the burst discount counts.  ``'image'`` (the default):
        all N tokens of the token's image, one weight per token.  ``'segment'``: the tokens of U(s), the segment's own after the
        neighbour union -- one weight per (segment, token), ``g[s][n] = sum_{m in U(s)} sigmoid(a (2 cos(x_n, x_m) - 2) + b)``;
        hard assignment then aggregates at the hard path's matrix work.  Read only while ``vlad_burst`` is on; with it off the value
        is stored and changes nothing.  Anything else is a ValueError and leaves the option as it was.  Returns the value that was
        in force before (this object's own record, like set_vlad_burst's)."""
        if not isinstance(scope, str) or scope not in BURST_SCOPES:
            raise ValueError(f"vlad_burst_scope: want one of {BURST_SCOPES}, got {scope!r}")
        before = self.vlad_burst_scope
        self.set_option("vlad_burst_scope", scope)
        return before

    def hint_query_groups(self, qseg_offsets) -> int:
        """Tell the search how the query rows of the coming batches are grouped (option ``query_group``): when every query
        image brings the same number of rows (<= 64) the exact refinement takes an image's rows as one group -- the bands of
        an image's segments share most of their rows (csrc/refine_group_kernels.hip).  Never changes a result."""
        runs = np.diff(np.asarray(qseg_offsets, dtype=np.int64))
        hint = int(runs[0]) if runs.size and int(runs.min()) == int(runs.max()) and 1 <= int(runs[0]) <= 64 else 0
        if hint != getattr(self, "_group_hint", None):
            self.set_option("query_group", hint)
            self._group_hint = hint
        return hint

    def search_stats(self) -> dict:
        """Statistics of the last search(): levels, filter arithmetic, rows redone on the exact path, list occupancies."""
        v = (C.c_int64 * 13)()
        self._check(self.lib.segvlad_search_stats(self._h, v, 13), "search_stats")
        names = ("levels", "filter", "n_fallback", "cand_max", "cand_sum", "refine_max", "refine_sum", "n_queries", "n_redo",
                 "n_refine2", "grp_groups", "grp_union_sum", "carry_rows")
        d = dict(zip(names, [int(x) for x in v]))
        d["filter"] = {0: "none", 1: "f16", 2: "bf16x3", 3: "fp32"}[d["filter"]]
        return d

    def stage_ms(self, stage: str):
        """(total ms, kernel launches) of the stage since the last profile_reset()."""
        ms, n = C.c_float(), C.c_int()
        self._stream()
        self._check(self.lib.segvlad_stage_ms(self._h, stage.encode(), C.byref(ms), C.byref(n)), f"stage_ms({stage})")
        return ms.value, n.value

    # ---- row-sharded index over several GPUs (segvlad_comm_* / segvlad_search_sharded: RCCL bound at run time) ----------
    def comm_unique_id(self) -> bytes:
        """128-byte RCCL id drawn by ONE rank; hand it to every rank's comm_init over any host channel."""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        rc = self.lib.segvlad_comm_unique_id(buf)
        if rc != 0:
            raise SegVLADError(f"comm_unique_id failed ({rc}): RCCL could not be bound (librccl.so; SEGVLAD_RCCL_LIB)", code=int(rc))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int):
        """Collective: bind an RCCL communicator (world ranks, one GPU each) to this context."""
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("uid must be the 128 bytes of comm_unique_id()")
        self._stream()
        self._check(self.lib.segvlad_comm_init(self._h, C.c_char_p(uid), int(rank), int(world)), "comm_init")

    def comm_destroy(self):
        self._check(self.lib.segvlad_comm_destroy(self._h), "comm_destroy")

    def comm_info(self) -> dict:
        r, w = C.c_int(), C.c_int()
        o = C.create_string_buffer(256)
        self._check(self.lib.segvlad_comm_info(self._h, C.byref(r), C.byref(w), o, 256), "comm_info")
        return {"rank": r.value, "world": w.value, "rccl": o.value.decode(errors="replace")}

    def allgather_rows(self, x, world: Optional[int] = None) -> torch.Tensor:
        """[n_local, d] fp32 of every rank -> [world * n_local, d] in rank order (equal slices), one RCCL all-gather.
        ``world``: the communicator's size if the caller knows it (saves a C call per gather)."""
        t = _as(x, np.float32, torch.float32)
        n, d = int(t.shape[0]), int(t.shape[1])
        out = self._empty(((int(world) if world else self.comm_info()["world"]) * n, d), torch.float32)
        self._stream()
        self._check(self.lib.segvlad_allgather_rows(self._h, _ptr(t), n, d, _ptr(out)), "allgather_rows")
        self._keep = [t]
        return out

    def search_sharded(self, Q, k: int, id_base: int):
        """Collective: global exact top-k over all ranks' shards, identical on every rank (d2 [nq,k], GLOBAL ids [nq,k])."""
        q = _as(Q, np.float32, torch.float32)
        nq = int(q.shape[0])
        d2 = self._empty((nq, k), torch.float32)
        idx = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_search_sharded(self._h, _ptr(q), nq, int(k), int(id_base), _ptr(d2), _ptr(idx)), "search_sharded")
        self._keep = [q]
        return d2, idx

    def vote_global(self, idx, sims, qseg_offsets, n_top=5, mode=_lib.VOTE_WT_BORDA_IM, img_of_seg=None, want_scores=True,
                    per_image=None, unique_ref=False):
        """Collective (query-sharded retrieval): vote() over this rank's query images with the min / max of the similarities of
        ALL ranks of the context's communicator (func_vpr.py:211-214).  Every rank calls it, a rank without images included
        (idx / sims [0, k]).  ``per_image``, ``unique_ref``: vote()'s."""
        mode = _lib.vote_mode(mode, per_image, unique_ref)
        i = _as(idx, np.int64, torch.int64)
        s = None if sims is None else _as(sims, np.float32, torch.float32)
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int32)
        n_img = len(qo) - 1
        k = int(i.shape[1])
        im = None if img_of_seg is None else _as(img_of_seg, np.int32, torch.int32)
        n_ref = 0 if im is None else int(im.shape[0])
        pred = self._empty((n_img, n_top), torch.int32)
        sc = self._empty((n_img, n_top), torch.float64) if want_scores else None
        self._stream()
        self._check(self.lib.segvlad_vote_global(self._h, _ptr(i), _ptr(s), _ptr(im), n_ref, _ptr(qo), n_img, k, int(n_top), int(mode),
                                                 _ptr(pred), _ptr(sc)), "vote_global")
        self._keep = [i, s, im]
        return pred, sc

    # ---- vocabulary -------------------------------------------------------------------------------
    def set_vocab(self, c_centers):
        c = _as(c_centers, np.float32, torch.float32)
        K, D = c.shape
        self._stream()
        self._check(self.lib.segvlad_set_vocab(self._h, _ptr(c), K, D), "set_vocab")
        if isinstance(c, torch.Tensor) and c.is_cuda:
            torch.cuda.current_stream(self.device).synchronize()
        self.K, self.D = int(K), int(D)
        self.vocab_generation += 1

    # ---- masks ------------------------------------------------------------------------------------
    def incidence(self, masks, H: int, W: int, patch: int = 14) -> torch.Tensor:
        """masks [S,Hm,Wm] bool/uint8 (tensor or ndarray) -> int64 tensor [S, ceil(N/64)] holding u64 bit rows."""
        m = masks.to(torch.uint8).contiguous() if isinstance(masks, torch.Tensor) else np.ascontiguousarray(masks).astype(np.uint8)
        S, Hm, Wm = m.shape
        N = (H // patch) * (W // patch)
        out = self._empty((S, (N + 63) // 64), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_incidence(self._h, _ptr(m), S, Hm, Wm, H, W, patch, _ptr(out)), "incidence")
        self._keep = [m]
        return out

    def incidence_centroids(self, masks, H: int, W: int, patch: int = 14):
        """One pass over the masks: (incidence bit rows [S, ceil(N/64)] as int64, centroids [S,2] fp64 (x, y))."""
        m = masks.to(torch.uint8).contiguous() if isinstance(masks, torch.Tensor) else np.ascontiguousarray(masks).astype(np.uint8)
        S, Hm, Wm = m.shape
        N = (H // patch) * (W // patch)
        out = self._empty((S, (N + 63) // 64), torch.int64)
        cent = self._empty((S, 2), torch.float64)
        self._stream()
        self._check(self.lib.segvlad_incidence_centroids(self._h, _ptr(m), S, Hm, Wm, H, W, patch, _ptr(out), _ptr(cent)),
                    "incidence_centroids")
        self._keep = [m]
        return out, cent

    def mask_centroids(self, masks) -> torch.Tensor:
        m = masks.to(torch.uint8).contiguous() if isinstance(masks, torch.Tensor) else np.ascontiguousarray(masks).astype(np.uint8)
        S, Hm, Wm = m.shape
        out = self._empty((S, 2), torch.float64)
        self._stream()
        self._check(self.lib.segvlad_mask_centroids(self._h, _ptr(m), S, Hm, Wm, _ptr(out)), "mask_centroids")
        self._keep = [m]
        return out

    # ---- run-length masks (rle.RleMasks: SAM's uncompressed RLE) -----------------------------------------------------------
    def _rle_args(self, rle):
        if not isinstance(rle, RleMasks):
            raise TypeError(f"expected an RleMasks batch, got {type(rle)}")
        n_bad = torch.zeros(1, dtype=torch.int32, device=self.device)   # the kernel adds to it; nothing here reads it back
        self.rle_n_bad = n_bad
        return rle.counts, rle.run_offsets, len(rle), rle.Hm, rle.Wm, n_bad

    def incidence_rle(self, rle, H: int, W: int, patch: int = 14, centroids: bool = True, want_bad: bool = False):
        """incidence_centroids() of a run-length batch without inflating it: ``(bits, cent)`` -- incidence bit rows
        [S, ceil(N/64)] as int64 and centroids [S, 2] fp64 (x, y), ``None`` with ``centroids=False`` -- byte for byte what the
        dense call returns for ``rle.to_dense()``.  The number of malformed masks (runs that do not sum to Hm * Wm) stays on the
        device: ``self.rle_n_bad`` (int32 [1]; also returned third with ``want_bad=True``) -- reading it is the caller's
        synchronisation, not this call's.  Masks whose bitmap exceeds 150 KiB of LDS raise SegVLADError with code
        SEGVLAD_ERR_LIMIT: ``incidence_centroids(rle_decode(rle), ...)`` then."""
        c, o, S, Hm, Wm, n_bad = self._rle_args(rle)
        N = (H // patch) * (W // patch)
        out = self._empty((S, (N + 63) // 64), torch.int64)
        cent = self._empty((S, 2), torch.float64) if centroids else None
        self._stream()
        self._check(self.lib.segvlad_incidence_rle(self._h, _ptr(c), _ptr(o), S, Hm, Wm, H, W, patch, _ptr(out), _ptr(cent), _ptr(n_bad)),
                    "incidence_rle")
        self._keep = [c, o, n_bad]
        return (out, cent, n_bad) if want_bad else (out, cent)

    def rle_decode(self, rle, want_bad: bool = False):
        """A run-length batch inflated on the device: uint8 [S, Hm, Wm] of 0 / 1 (any size).  ``self.rle_n_bad`` /
        ``want_bad`` as for incidence_rle."""
        c, o, S, Hm, Wm, n_bad = self._rle_args(rle)
        out = self._empty((S, Hm, Wm), torch.uint8)
        self._stream()
        self._check(self.lib.segvlad_rle_decode(self._h, _ptr(c), _ptr(o), S, Hm, Wm, _ptr(out), _ptr(n_bad)), "rle_decode")
        self._keep = [c, o, n_bad]
        return (out, n_bad) if want_bad else out

    def rle_encode(self, masks, want_area: bool = False, capacity: Optional[int] = None):
        """segvlad_rle_encode: dense masks -> an ``RleMasks`` batch whose ``counts`` (uint32) and ``run_offsets`` (int64) are
        device tensors, the counts of ``RleMasks.from_dense(masks)`` (mask_to_rle_pytorch); with ``want_area`` also the set
        pixels of every mask, ``(rle, areas)`` with ``areas`` int64 [S] on the device (area_from_rle).  ``masks``: [S, Hm, Wm]
        or one [Hm, Wm], uint8 (non-zero = set) or bool (viewed as bytes, not copied), a torch tensor on the device or the host
        or a NumPy array; made contiguous when it is not.  The first call offers ``capacity`` slots (default
        ``S * (2 * Wm + 2)``: a column-convex blob fits); when the runs do not fit it is repeated once with the total it
        reported (``self.rle_encode_retried``).  Synchronises once: the total has to reach the host to size the result."""
        if isinstance(masks, torch.Tensor):
            m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
            if m.dtype != torch.uint8:
                raise TypeError(f"masks must be uint8 or bool, got {masks.dtype}")
            m = m.contiguous()
        else:
            a = np.asarray(masks)
            a = a.view(np.uint8) if a.dtype == np.bool_ else a
            if a.dtype != np.uint8:
                raise TypeError(f"masks must be uint8 or bool, got {a.dtype}")
            m = np.ascontiguousarray(a)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3:
            raise ValueError(f"masks must be [S, Hm, Wm], got {tuple(m.shape)}")
        S, Hm, Wm = (int(v) for v in m.shape)
        capacity = S * (2 * Wm + 2) if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        offs = self._empty((S + 1,), torch.int64)
        areas = self._empty((S,), torch.int64) if want_area else None
        total = C.c_int64()
        self._stream()
        self.rle_encode_retried = False
        while True:
            counts = self._empty((capacity,), torch.uint32)
            self._check(self.lib.segvlad_rle_encode(self._h, _ptr(m) if S else None, S, Hm, Wm, _ptr(offs), _ptr(counts) if capacity else None,
                                                    capacity, _ptr(areas) if S and want_area else None, C.byref(total)), "rle_encode")
            if total.value <= capacity:
                break
            capacity = int(total.value)
            self.rle_encode_retried = True
        self._keep = [m]
        rle = RleMasks(counts[:total.value], offs, Hm, Wm, validate=False)
        return (rle, areas) if want_area else rle

    MASK_REGIONS_SCRATCH_BYTES = 1 << 30   # mask_regions: the label and size planes of one call, 8 bytes per pixel, stay below this

    def mask_regions(self, masks, min_area: int, want_boxes: bool = True, want_area: bool = True, chunk: Optional[int] = None) -> dict:
        """segvlad_mask_regions: small holes filled and small islands removed from every mask (remove_small_regions, mode
        "holes" then mode "islands", utils/amg.py:267-291; 8-connected, strictly ``< min_area``, keep-largest with the tie to
        the component whose first pixel comes first).  ``masks``: [S, Hm, Wm] or one [Hm, Wm], uint8 (non-zero = set) or bool,
        a torch tensor on the device or the host or a NumPy array; made contiguous when it is not.  Returns device tensors:
        ``masks`` uint8 [S, Hm, Wm] of 0 / 1, ``changed`` int32 [S] (bit 0: the holes pass changed the mask, bit 1: the islands
        pass), and with ``want_boxes`` / ``want_area`` ``boxes`` int32 [S, 4] (tight XYXY, inclusive, zeros for an empty mask:
        ``producers.mask_boxes``) and ``area`` int64 [S].  The batch is processed ``chunk`` masks per call; by default as many as
        keep the call's scratch, 8 bytes per pixel, under ``MASK_REGIONS_SCRATCH_BYTES`` (1 GiB).  Does not synchronise when
        ``masks`` is on the device."""
        if isinstance(masks, torch.Tensor):
            m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
            if m.dtype != torch.uint8:
                raise TypeError(f"masks must be uint8 or bool, got {masks.dtype}")
            m = m.contiguous()
        else:
            a = np.asarray(masks)
            a = a.view(np.uint8) if a.dtype == np.bool_ else a
            if a.dtype != np.uint8:
                raise TypeError(f"masks must be uint8 or bool, got {a.dtype}")
            m = np.ascontiguousarray(a)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3:
            raise ValueError(f"masks must be [S, Hm, Wm], got {tuple(m.shape)}")
        S, Hm, Wm = (int(v) for v in m.shape)
        min_area = int(min_area)
        if chunk is None:
            chunk = max(1, self.MASK_REGIONS_SCRATCH_BYTES // (8 * max(1, Hm * Wm)))
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        out = self._empty((S, Hm, Wm), torch.uint8)
        changed = self._empty((S,), torch.int32)
        boxes = self._empty((S, 4), torch.int32) if want_boxes else None
        area = self._empty((S,), torch.int64) if want_area else None
        self._stream()
        for s0 in range(0, max(S, 1), chunk):   # (S == 0: one call, which checks the arguments and writes nothing)
            n = min(chunk, S - s0)
            self._check(self.lib.segvlad_mask_regions(self._h, _ptr(m[s0:s0 + n]) if n else None, n, Hm, Wm, min_area, _ptr(out[s0:s0 + n]) if n else None,
                                                      _ptr(changed[s0:s0 + n]) if n else None, _ptr(boxes[s0:s0 + n]) if n and want_boxes else None,
                                                      _ptr(area[s0:s0 + n]) if n and want_area else None), "mask_regions")
        self._keep = [m]
        res = {"masks": out, "changed": changed}
        if want_boxes:
            res["boxes"] = boxes
        if want_area:
            res["area"] = area
        return res

    def adjacency(self, centroids, seg_offsets, order: int, check_empty: bool = False) -> torch.Tensor:
        """centroids [S_tot,2] fp64 -> uint8 buffer with the concatenated per-image [S_b,S_b] (A1^order > 0)
        blocks, computed on the device.  check_empty=True synchronises and raises ValueError on an empty mask
        (the reference's behaviour), and SegVLADDegenerateError when an image holds a non-generic centroid
        configuration (duplicate or exactly co-circular points: Qhull's triangulation is then a matter of its own
        tie-breaking; SegVLADPipeline catches this and uses the reference's Qhull path for that batch)."""
        c = _as(centroids, np.float64, torch.float64)
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        B = len(so) - 1
        total = int(((so[1:] - so[:-1]).astype(np.int64) ** 2).sum())
        out = self._empty((total,), torch.uint8)
        n_bad = (C.c_uint32 * 1)(0)
        self._stream()
        self._check(self.lib.segvlad_adjacency(self._h, _ptr(c), _ptr(so), B, int(order), _ptr(out),
                                               C.cast(n_bad, C.c_void_p) if check_empty else None), "adjacency")
        self._keep = [c]
        if check_empty and n_bad[0] & 0xFFFF:
            raise ValueError(f"{n_bad[0] & 0xFFFF} empty mask(s): centroid undefined")
        if check_empty and n_bad[0] >> 16:
            raise SegVLADDegenerateError(f"adjacency: {n_bad[0] >> 16} image(s) with a degenerate centroid configuration "
                                         "(duplicate or co-circular centroids): the Delaunay triangulation is not unique")
        return out

    def adjacency_flagged(self, centroids, seg_offsets, order: int, device_flags: bool = False):
        """adjacency() plus one flag byte per image: bit 0 = empty mask in the image, bit 1 = non-generic centroid
        configuration (segvlad_adjacency_flagged).  Never raises on either.  The flags come back as a NumPy uint8 [B] (ONE
        B-byte read-back, i.e. a host synchronisation) -- or, with ``device_flags``, as a device tensor the caller reads when it
        suits it (e.g. after it has enqueued the kernels that consume the adjacency)."""
        c = _as(centroids, np.float64, torch.float64)
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        B = len(so) - 1
        total = int(((so[1:] - so[:-1]).astype(np.int64) ** 2).sum())
        out = self._empty((total,), torch.uint8)
        flags = self._empty((max(B, 1),), torch.uint8) if device_flags else np.zeros(max(B, 1), np.uint8)
        self._stream()
        self._check(self.lib.segvlad_adjacency_flagged(self._h, _ptr(c), _ptr(so), B, int(order), _ptr(out), _ptr(flags)),
                    "adjacency_flagged")
        self._keep = [c]
        return out, flags[:B]

    # ---- segment VLAD -----------------------------------------------------------------------------
    def seg_vlad(self, tokens, inc_bits, seg_offsets: Sequence[int], adj=None, want_labels=False, want_gap=False,
                 want_block_norms=False, out: Optional[torch.Tensor] = None):
        """tokens [B,D,N] fp32; inc_bits [S_tot,nw] (int64 storage of u64); seg_offsets [B+1];
        adj: None | uint8 buffer with the concatenated per-image [S_b,S_b] matrices.
        Returns dict(out=[S_tot,K*D] fp32 device tensor, labels?, gap?, block_norms?)."""
        if self.K == 0:
            raise SegVLADError("seg_vlad: set_vocab first")
        t = _as(tokens, np.float32, torch.float32)
        if t.ndim == 2:
            t = t[None]
        B, D, N = t.shape
        if D != self.D:
            raise ValueError(f"tokens have D={D}, vocabulary has D={self.D}")
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        assert so.shape == (B + 1,)
        S_tot = int(so[-1])
        ib = inc_bits if isinstance(inc_bits, torch.Tensor) else np.ascontiguousarray(inc_bits)
        a = None
        if adj is not None:
            a = adj.to(torch.uint8).contiguous() if isinstance(adj, torch.Tensor) else np.ascontiguousarray(adj).astype(np.uint8)
        if out is None:
            out = self._empty((S_tot, self.K * self.D), torch.float32)
        res = {"out": out}
        lab = self._empty((B, N), torch.uint8) if want_labels else None
        gap = self._empty((B, N), torch.float32) if want_gap else None
        bn = self._empty((S_tot, self.K), torch.float32) if want_block_norms else None
        self._stream()
        self._check(self.lib.segvlad_images(self._h, _ptr(t), B, N, _ptr(ib), _ptr(so), _ptr(a), _ptr(out), _ptr(lab),
                                            _ptr(gap), _ptr(bn)), "images")
        self._keep = [t, ib, a]
        if want_labels:
            res["labels"] = lab
        if want_gap:
            res["gap"] = gap
        if want_block_norms:
            res["block_norms"] = bn
        return res

    def seg_vlad_pca(self, tokens, inc_bits, seg_offsets: Sequence[int], adj=None, l2norm: bool = True, want_desc=False,
                     want_labels=False, want_gap=False):
        """Fused seg_vlad + pca_apply (segvlad_images_pca): returns dict(out=[S_tot,P] projected (and normalised)
        descriptors, desc?=[S_tot,K*D], labels?, gap?).  Without want_desc the K*D-wide descriptor never reaches HBM."""
        if self.K == 0:
            raise SegVLADError("seg_vlad_pca: set_vocab first")
        if self.P == 0:
            raise SegVLADError("seg_vlad_pca: pca_set first")
        t = _as(tokens, np.float32, torch.float32)
        if t.ndim == 2:
            t = t[None]
        B, D, N = t.shape
        if D != self.D:
            raise ValueError(f"tokens have D={D}, vocabulary has D={self.D}")
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        assert so.shape == (B + 1,)
        S_tot = int(so[-1])
        ib = inc_bits if isinstance(inc_bits, torch.Tensor) else np.ascontiguousarray(inc_bits)
        a = None
        if adj is not None:
            a = adj.to(torch.uint8).contiguous() if isinstance(adj, torch.Tensor) else np.ascontiguousarray(adj).astype(np.uint8)
        y = self._empty((S_tot, self.P), torch.float32)
        desc = self._empty((S_tot, self.K * self.D), torch.float32) if want_desc else None
        lab = self._empty((B, N), torch.uint8) if want_labels else None
        gap = self._empty((B, N), torch.float32) if want_gap else None
        self._stream()
        self._check(self.lib.segvlad_images_pca(self._h, _ptr(t), B, N, _ptr(ib), _ptr(so), _ptr(a), _ptr(y), int(bool(l2norm)),
                                                _ptr(desc), _ptr(lab), _ptr(gap)), "images_pca")
        self._keep = [t, ib, a]
        res = {"out": y}
        if want_desc:
            res["desc"] = desc
        if want_labels:
            res["labels"] = lab
        if want_gap:
            res["gap"] = gap
        return res

    def _describe_operands(self, masks, tokens, seg_offsets, pca: bool) -> dict:
        """The checks of describe / describe_begin, their operands as the C-ABI takes them and the mask branch's outputs (bits, cent,
        adj, flags): the handle of a describe_begin."""
        if self.K == 0:
            raise SegVLADError("describe: set_vocab first")
        if pca and self.P == 0:
            raise SegVLADError("describe: pca_set first")
        m = (masks if masks.dtype == torch.uint8 else masks.to(torch.uint8)).contiguous()
        t = tokens.to(torch.float32).contiguous()
        if t.ndim == 2:
            t = t[None]
        B, D, N = t.shape
        if D != self.D:
            raise ValueError(f"tokens have D={D}, vocabulary has D={self.D}")
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        assert so.shape == (B + 1,) and m.shape[0] == int(so[-1])
        S_tot = int(so[-1])
        sizes = (so[1:] - so[:-1]).astype(np.int64)
        return {"m": m, "t": t, "so": so, "B": B, "N": N, "S_tot": S_tot, "pca": bool(pca),
                "bits": self._empty((S_tot, (N + 63) // 64), torch.int64), "cent": self._empty((S_tot, 2), torch.float64),
                "adj": self._empty((int((sizes * sizes).sum()),), torch.uint8), "flags": self._empty((B,), torch.uint8)}

    def describe(self, masks, tokens, seg_offsets: Sequence[int], H: int, W: int, patch: int = 14, order: int = 3, pca: bool = True,
                 l2norm: bool = True, want_desc: bool = False) -> dict:
        """segvlad_describe: the describe stage of a batch in one call -- incidence + centroids + device adjacency on the
        context's side stream beside the token-assignment pass, then seg-VLAD (+ PCA).  Device tensors only.  Returns
        dict(out=[S_tot,P] or [S_tot,K*D], bits, cent, adj, flags [B] uint8 on the device: bit 0 empty mask, bit 1 non-generic
        centroids -- pipeline.py patches flagged images with Qhull), desc? with pca and want_desc."""
        h = self._describe_operands(masks, tokens, seg_offsets, pca)
        m, t, S_tot = h["m"], h["t"], h["S_tot"]
        bits, cent, adj, flags = h["bits"], h["cent"], h["adj"], h["flags"]
        y = self._empty((S_tot, self.P), torch.float32) if pca else None
        desc = self._empty((S_tot, self.K * self.D), torch.float32) if (want_desc or not pca) else None
        self._stream()
        self._check(self.lib.segvlad_describe(self._h, _ptr(m), int(m.shape[1]), int(m.shape[2]), int(H), int(W), int(patch), _ptr(t), h["B"],
                                              h["N"], _ptr(h["so"]), int(order), _ptr(bits), _ptr(cent), _ptr(adj), _ptr(flags), _ptr(desc),
                                              _ptr(y), int(bool(l2norm))), "describe")
        self._keep = [m, t]
        res = {"out": y if pca else desc, "bits": bits, "cent": cent, "adj": adj, "flags": flags}
        if pca and want_desc:
            res["desc"] = desc
        return res

    # ---- the same stage as begin / flags / end: the caller patches flagged images with Qhull WHILE the assignment pass runs ----
    def describe_begin(self, masks, tokens, seg_offsets: Sequence[int], H: int, W: int, patch: int = 14, order: int = 3,
                       pca: bool = True) -> dict:
        """segvlad_describe_begin: enqueues the mask branch (side stream) and the assignment pass, returns the handle
        describe_flags / describe_end take (it owns the intermediates: bits, cent, adj, flags)."""
        h = self._describe_operands(masks, tokens, seg_offsets, pca)
        h["order"] = int(order)
        m, t = h["m"], h["t"]
        self._stream()
        self._check(self.lib.segvlad_describe_begin(self._h, _ptr(m), int(m.shape[1]), int(m.shape[2]), int(H), int(W), int(patch), _ptr(t),
                                                    h["B"], h["N"], _ptr(h["so"]), int(order), _ptr(h["bits"]), _ptr(h["cent"]), _ptr(h["adj"]),
                                                    _ptr(h["flags"]), int(bool(pca))), "describe_begin")
        return h

    def describe_flags(self, h: dict):
        """segvlad_describe_flags: (flags [B] uint8, centroids [S_tot,2] fp64) on the HOST; waits for the mask branch only."""
        flags = np.empty(h["B"], np.uint8)
        cent = np.empty((h["S_tot"], 2), np.float64)
        self._check(self.lib.segvlad_describe_flags(self._h, flags.ctypes.data_as(C.c_void_p), cent.ctypes.data_as(C.c_void_p)),
                    "describe_flags")
        return flags, cent

    def describe_cancel(self, h: dict):
        """Ends a describe_begin without results (the mask branch is joined, the context is usable again)."""
        self.lib.segvlad_describe_end(self._h, _ptr(h["t"]), h["B"], h["N"], _ptr(h["bits"]), _ptr(h["so"]), _ptr(h["adj"]), 0, None, None,
                                      None, None, 0)

    def describe_end(self, h: dict, patch_images=None, patch_blocks=None, l2norm: bool = True, want_desc: bool = False) -> dict:
        """segvlad_describe_end: patch_images (ascending image indices) / patch_blocks (their [S_b,S_b] uint8 adjacency matrices,
        host arrays) replace the device adjacency of those images; then prep -> aggregation (-> projection)."""
        pca = h["pca"]
        y = self._empty((h["S_tot"], self.P), torch.float32) if pca else None
        desc = self._empty((h["S_tot"], self.K * self.D), torch.float32) if (want_desc or not pca) else None
        n_patch = 0 if patch_images is None else len(patch_images)
        pi = pb = None
        if n_patch:
            pi = np.ascontiguousarray(patch_images, dtype=np.int32)
            pb = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.uint8).reshape(-1) for b in patch_blocks]))
        self._stream()
        self._check(self.lib.segvlad_describe_end(self._h, _ptr(h["t"]), h["B"], h["N"], _ptr(h["bits"]), _ptr(h["so"]), _ptr(h["adj"]),
                                                  n_patch, _ptr(pi), _ptr(pb), _ptr(desc), _ptr(y), int(bool(l2norm))), "describe_end")
        res = {"out": y if pca else desc, "bits": h["bits"], "cent": h["cent"], "adj": h["adj"], "flags": h["flags"]}
        if pca and want_desc:
            res["desc"] = desc
        return res

    def kmeans_step(self, tokens, sums: torch.Tensor, counts: torch.Tensor, want_labels: bool = False):
        """segvlad_kmeans_step: with the current centres in the context (set_vocab), ACCUMULATES the per-cluster sums of the normalised
        tokens into ``sums`` [K, D] fp64 and the assignment counts into ``counts`` [K] int64 (device tensors); tokens [B, D, N]."""
        t = _as(tokens, np.float32, torch.float32)
        if isinstance(t, torch.Tensor):
            t = t.contiguous()
        if t.ndim == 2:
            t = t[None]
        B, D, N = t.shape
        if D != self.D:
            raise ValueError(f"tokens have D={D}, vocabulary has D={self.D}")
        if not (isinstance(sums, torch.Tensor) and sums.is_cuda and sums.dtype == torch.float64 and tuple(sums.shape) == (self.K, self.D)
                and sums.is_contiguous() and isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int64
                and tuple(counts.shape) == (self.K,)):
            raise ValueError("kmeans_step: sums must be a contiguous device fp64 [K, D] tensor, counts a device int64 [K] tensor")
        lab = self._empty((B, N), torch.uint8) if want_labels else None
        self._stream()
        self._check(self.lib.segvlad_kmeans_step(self._h, _ptr(t), B, N, _ptr(sums), _ptr(counts), _ptr(lab)), "kmeans_step")
        self._keep = [t]
        return lab

    def cluster_aggregate(self, num_c: int, res, labels, inc_bits, adj=None) -> torch.Tensor:
        """vlad_matmuls_per_cluster surface: res [N,D] fp32 residuals, labels [N] (< num_c), inc_bits [S,nw]."""
        r = _as(res, np.float32, torch.float32)
        N, D = r.shape
        lab = _as(labels, np.uint8, torch.uint8)
        ib = inc_bits if isinstance(inc_bits, torch.Tensor) else np.ascontiguousarray(inc_bits)
        S = ib.shape[0]
        a = None
        if adj is not None:
            a = adj.to(torch.uint8).contiguous() if isinstance(adj, torch.Tensor) else np.ascontiguousarray(adj).astype(np.uint8)
        out = self._empty((S, num_c * D), torch.float32)
        self._stream()
        self._check(self.lib.segvlad_cluster_aggregate(self._h, num_c, _ptr(r), _ptr(lab), N, D, _ptr(ib), S, _ptr(a), _ptr(out)),
                    "cluster_aggregate")
        self._keep = [r, lab, ib, a]
        return out

    # ---- PCA --------------------------------------------------------------------------------------
    def pca_set(self, mean, components, explained_variance=None, whiten=True):
        comps = _as(components, np.float32, torch.float32)
        P, KD = comps.shape
        mean = None if mean is None else _as(mean, np.float32, torch.float32)
        var = None if explained_variance is None else _as(explained_variance, np.float32, torch.float32)
        self._stream()
        self._check(self.lib.segvlad_pca_set(self._h, _ptr(mean), _ptr(comps), _ptr(var), P, KD, int(bool(whiten))), "pca_set")
        self.P, self.KD = int(P), int(KD)
        self.pca_generation += 1

    def pca_apply(self, X, l2norm=False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _as(X, np.float32, torch.float32)
        n, KD = x.shape
        if KD != self.KD:
            raise ValueError(f"X has {KD} columns, PCA model expects {self.KD}")
        if out is None:
            out = self._empty((n, self.P), torch.float32)
        self._stream()
        self._check(self.lib.segvlad_pca_apply(self._h, _ptr(x), n, _ptr(out), int(l2norm)), "pca_apply")
        self._keep = [x]
        return out

    def normalize_rows(self, X) -> torch.Tensor:
        x = _as(X, np.float32, torch.float32)
        n, d = x.shape
        out = self._empty((n, d), torch.float32)
        self._stream()
        self._check(self.lib.segvlad_normalize_rows(self._h, _ptr(x), n, d, _ptr(out)), "normalize_rows")
        self._keep = [x]
        return out

    # ---- exact kNN --------------------------------------------------------------------------------
    def db_reset(self):
        self._check(self.lib.segvlad_db_reset(self._h), "db_reset")
        self.n_img_ref = 0

    def db_add(self, R, img_of_seg=None):
        r = _as(R, np.float32, torch.float32)
        n, d = r.shape
        im = None if img_of_seg is None else _as(img_of_seg, np.int32, torch.int32)
        self._stream()
        self._check(self.lib.segvlad_db_add(self._h, _ptr(r), n, d, _ptr(im)), "db_add")
        if im is not None and n > 0:
            self.n_img_ref = max(self.n_img_ref, int(im.max()) + 1)
        if isinstance(r, torch.Tensor) and r.is_cuda:
            torch.cuda.current_stream(self.device).synchronize()  # the index copied the rows: r may now be freed

    def db_remove(self, row_ids=None, img_ids=None, want_new_ids: bool = False):
        """segvlad_db_remove (faiss IndexFlat::remove_ids): drops the rows whose id is in ``row_ids`` or whose image id (the
        img_of_seg of db_add) is in ``img_ids``; the survivors keep their order and are renumbered 0 .. n' - 1.  Out-of-range
        and duplicate ids are ignored.  Returns the number removed, and with ``want_new_ids`` also the int64 device tensor [n]
        of every old row's new id (-1: removed).  n_img_ref keeps its meaning (1 + the largest id given to db_add since
        db_reset): a shortlist may still name a removed image, which then contributes no rows."""
        ri = None if row_ids is None else _as(row_ids, np.int64, torch.int64).reshape(-1)
        ii = None if img_ids is None else _as(img_ids, np.int32, torch.int32).reshape(-1)
        n_r = 0 if ri is None else int(ri.shape[0])
        n_i = 0 if ii is None else int(ii.shape[0])
        n, _ = self.db_size()
        new_ids = self._empty((n,), torch.int64) if want_new_ids else None
        removed = C.c_int64(0)
        self._stream()
        self._check(self.lib.segvlad_db_remove(self._h, _ptr(ri) if n_r else None, n_r, _ptr(ii) if n_i else None, n_i,
                                               _ptr(new_ids) if n else None, C.byref(removed)), "db_remove")
        return (int(removed.value), new_ids) if want_new_ids else int(removed.value)

    def db_size(self):
        n, d = C.c_int64(), C.c_int()
        self.lib.segvlad_db_size(self._h, C.byref(n), C.byref(d))
        return n.value, d.value

    def search(self, Q, k: int):
        """segvlad_search: device tensors (d2 [nq][k] fp32 ascending, idx [nq][k] int64; ties to the lower id, (+inf, -1) beyond the
        index).  Non-finite rows (an all-zero descriptor normalises to a NaN row) are ordinary input: a pair whose fp32 distance
        is NaN or +inf is never listed -- an index row holding NaN or +-Inf is in nobody's list, a query row holding one returns
        (+inf, -1) in every slot, a list with fewer than k finite distances is padded with (+inf, -1) -- and every finite query
        row gets, bit for bit, what an index of the finite rows alone returns (ids as db_remove would renumber them), at no extra
        cost.  search_shortlist, search_excluding and search_grouped hold the same rule."""
        q = _as(Q, np.float32, torch.float32)
        nq = q.shape[0]
        d2 = self._empty((nq, k), torch.float32)
        idx = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_search(self._h, _ptr(q), nq, k, _ptr(d2), _ptr(idx)), "search")
        self._keep = [q]
        return d2, idx

    def search_shortlist(self, Q, qseg_offsets, shortlist, k: int):
        """segvlad_search_shortlist: per query row the exact top-k rows of the index whose image is in its query image's
        shortlist.  ``qseg_offsets`` [n_img + 1] (host); ``shortlist``: ``int32 [n_img][M]`` (-1 padded; a host array is
        validated here, ids < -1 or >= n_img_ref raise ValueError) or a ragged list of lists (padded by pad_shortlists).
        Returns device tensors (d2 [nq][k] fp32, idx [nq][k] int64) like search(); (+inf, -1) beyond the allowed rows."""
        q = _as(Q, np.float32, torch.float32)
        nq = q.shape[0]
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int32)
        n_img = len(qo) - 1
        if isinstance(shortlist, torch.Tensor) and shortlist.is_cuda:
            sl = shortlist.to(torch.int32).contiguous()
            if sl.dim() != 2 or sl.shape[0] != n_img:
                raise ValueError(f"shortlist must be [n_img={n_img}][M], got shape {tuple(sl.shape)}")
        else:
            if isinstance(shortlist, torch.Tensor):
                shortlist = shortlist.numpy()
            if isinstance(shortlist, np.ndarray) and shortlist.ndim == 2:
                sl = np.ascontiguousarray(shortlist, dtype=np.int64)
            else:
                sl = pad_shortlists(shortlist).astype(np.int64)
            check_shortlist(sl, n_img, self.n_img_ref)
            sl = np.ascontiguousarray(sl, dtype=np.int32)
        M = int(sl.shape[1])
        d2 = self._empty((nq, k), torch.float32)
        idx = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_search_shortlist(self._h, _ptr(q), nq, _ptr(qo), n_img, _ptr(sl), M, k, _ptr(d2), _ptr(idx)),
                    "search_shortlist")
        self._keep = [q, sl]
        return d2, idx

    def search_excluding(self, Q, qseg_offsets, exclude, k: int):
        """segvlad_search_excluding: per query row the exact top-k rows of the index whose image id lies in none of its query
        image's intervals -- what a fresh index without those images returns.  ``qseg_offsets`` [n_img + 1] (host);
        ``exclude``: host ``int32 [n_img][E][2]`` of inclusive ``[lo, hi]`` reference image ids (lo > hi: empty; E <= 8), or a
        ragged list of ``(lo, hi)`` lists per image (padded by pad_intervals); window_intervals builds the self-query form.
        Malformed input raises ValueError.  Returns device tensors (d2 [nq][k] fp32, idx [nq][k] int64) like search();
        (+inf, -1) beyond the allowed rows.
        Cost: the search runs once at depth ``k_fetch = min(1024, k + rows of the largest window)``, and that depth is what a
        caller pays: a few per cent for a window of a few images, 1.4 - 1.8 x the plain search at depths 600 - 900
        -- and 27 - 37 x once k_fetch reaches the depth at which the search plan leaves its filter levels for the
        distance-matrix path (977 on a 1 M-row index: 19 images of 50 rows at k = 50).  Keep ``k + rows of the window`` below
        that; for a larger window of ONE image, db_remove + search + db_add is cheaper today."""
        q = _as(Q, np.float32, torch.float32)
        nq = q.shape[0]
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int32)
        n_img = len(qo) - 1
        if isinstance(exclude, torch.Tensor):
            exclude = exclude.cpu().numpy()
        if isinstance(exclude, np.ndarray) and exclude.ndim == 3:
            ex = np.ascontiguousarray(exclude, dtype=np.int64)
        else:
            ex = pad_intervals(exclude).astype(np.int64)
        check_intervals(ex, n_img)
        ex = np.ascontiguousarray(ex, dtype=np.int32)
        d2 = self._empty((nq, k), torch.float32)
        idx = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_search_excluding(self._h, _ptr(q), nq, _ptr(qo), n_img, _ptr(ex), int(ex.shape[1]), k,
                                                      _ptr(d2), _ptr(idx)), "search_excluding")
        self._keep = [q]
        return d2, idx

    def search_grouped(self, Q, k: int, per_image: int = 1):
        """segvlad_search_grouped: per query row the nearest index rows such that no reference image (the img_of_seg of db_add)
        appears more than ``per_image`` times (1 .. 16) -- collapse_lists() over the unbounded search() list, bit for bit.  A row
        with a negative image id is a group of its own.  Returns device tensors (d2 [nq][k] fp32, idx [nq][k] int64) like
        search(); (+inf, -1) once the index runs out of admissible rows.  ``per_image=1`` gives k DIFFERENT images per query
        segment: one segment, one vote per image -- and distinct candidates for match_pairs().
        Cost: one search at depth ``min(1024, 4 k)`` plus a collapse kernel; a row whose nearest ``k_fetch`` rows hold fewer
        than k admissible ones is finished by an exact pass over the whole index (group_stats()["tail_rows"])."""
        q = _as(Q, np.float32, torch.float32)
        nq = q.shape[0]
        d2 = self._empty((nq, k), torch.float32)
        idx = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_search_grouped(self._h, _ptr(q), nq, k, int(per_image), _ptr(d2), _ptr(idx)), "search_grouped")
        self._keep = [q]
        return d2, idx

    def group_stats(self) -> dict:
        """Statistics of the last search_grouped(): the depth of the inner search, the query rows the exact tail finished, the
        largest number of list entries a row read before the collapse declared it complete."""
        v = (C.c_int64 * 3)()
        self._check(self.lib.segvlad_group_stats(self._h, v, 3), "group_stats")
        return dict(zip(("k_fetch", "tail_rows", "max_read"), [int(x) for x in v]))

    def match_pairs(self, Q, qseg_offsets, cand, max_d2: float = float("inf"), want_rows: bool = False) -> dict:
        """segvlad_match_pairs: for every query image b and candidate slot j, the mutual nearest pairs between the image's
        query rows and the index rows of reference image ``cand[b][j]`` -- q and r pair up when r is q's nearest row of that
        image, q is r's nearest row of the query image, and ``d2 < max_d2``.  ``qseg_offsets`` [n_img + 1] (host);
        ``cand``: host ``int32 [n_img][C]`` (-1 padded, C <= 64; vote()'s ``pred`` as it is) or a ragged list of lists (padded
        by pad_candidates); malformed input raises ValueError.  Returns device tensors: ``n_mutual`` int32 [n_img][C], ``score``
        fp64 [n_img][C] (the pairs' summed ``2 - d2``), ``order`` int32 [n_img][C] (the slots by (n_mutual desc, score desc,
        slot asc), slots without rows last); with ``want_rows`` also ``fwd_idx`` int64 / ``fwd_d2`` fp32 / ``mutual`` uint8
        [nq][C]: every query row's nearest row of the slot's image, (-1, +inf) where it has none, and whether the pair is mutual."""
        q = _as(Q, np.float32, torch.float32)
        nq = int(q.shape[0])
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int32)
        n_img = len(qo) - 1
        if isinstance(cand, torch.Tensor):
            cand = cand.cpu().numpy()
        if isinstance(cand, np.ndarray) and cand.ndim == 2:
            cd = cand
        else:
            cd = pad_candidates(cand)
        check_candidates(cd, n_img)
        cd = np.ascontiguousarray(cd, dtype=np.int32)
        Cw = int(cd.shape[1])
        out = {"n_mutual": self._empty((n_img, Cw), torch.int32), "score": self._empty((n_img, Cw), torch.float64),
               "order": self._empty((n_img, Cw), torch.int32)}
        if want_rows:
            out["fwd_idx"] = self._empty((nq, Cw), torch.int64)
            out["fwd_d2"] = self._empty((nq, Cw), torch.float32)
            out["mutual"] = self._empty((nq, Cw), torch.uint8)
        self._stream()
        self._check(self.lib.segvlad_match_pairs(self._h, _ptr(q), nq, _ptr(qo), n_img, _ptr(cd), Cw, float(max_d2),
                                                 _ptr(out["n_mutual"]), _ptr(out["score"]), _ptr(out["order"]),
                                                 _ptr(out.get("fwd_idx")), _ptr(out.get("fwd_d2")), _ptr(out.get("mutual"))),
                    "match_pairs")
        self._keep = [q]
        return out

    def verify_pairs(self, q_xy, r_xy, qseg_offsets, fwd_idx, mutual, tol: float, min_scale: float = 0.5, max_scale: float = 2.0,
                     want_rows: bool = False) -> dict:
        """segvlad_verify_pairs: for every query image b and slot j, how many of the slot's correspondences -- the query rows
        with ``mutual[q][j] != 0`` and their ``fwd_idx[q][j]``, match_pairs(want_rows=True)'s outputs -- agree on one 2-D
        similarity transform of their centroids.  ``q_xy`` fp64 [nq][2] and ``r_xy`` fp64 [n_r][2]: the (x, y) centroid of every
        query row and of every index row id; ``qseg_offsets`` [n_img + 1] (host); ``fwd_idx`` [nq][C] int64, ``mutual`` [nq][C]
        uint8, C <= 64.  Every pair of correspondences is a hypothesis (exhaustive, deterministic); a correspondence is an inlier
        when the similarity moves its query centroid to within ``tol`` of its reference centroid; hypotheses whose scale lies
        outside ``min_scale .. max_scale`` are not eligible.  At most 256 rows per query image.  Malformed input raises
        ValueError.  Returns device tensors: ``n_inlier`` int32 [n_img][C], ``pair`` int32 [n_img][C][2] (the winner's two query
        rows, (-1, -1): none), ``model`` fp64 [n_img][C][4] ((a_re, a_im, t_x, t_y), NaN: none), ``order`` int32 [n_img][C] (the
        slots by (n_inlier desc, slot asc)); with ``want_rows`` also ``inlier`` uint8 [nq][C]."""
        qx = _as(q_xy, np.float64, torch.float64)
        rx = _as(r_xy, np.float64, torch.float64)
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int64).reshape(-1)
        if qx.ndim != 2 or qx.shape[1] != 2:
            raise ValueError(f"q_xy must be [nq][2], got shape {tuple(qx.shape)}")
        if rx.ndim != 2 or rx.shape[1] != 2:
            raise ValueError(f"r_xy must be [n_r][2], got shape {tuple(rx.shape)}")
        nq, n_r = int(qx.shape[0]), int(rx.shape[0])
        if len(qo) < 1 or qo[0] != 0 or qo[-1] != nq or (np.diff(qo) < 0).any():
            raise ValueError(f"qseg_offsets must run from 0 to nq={nq} and never decrease")
        if (np.diff(qo) > MAX_VERIFY_ROWS).any():
            raise ValueError(f"a query image owns {int(np.diff(qo).max())} rows, more than {MAX_VERIFY_ROWS}")
        for name, x in (("fwd_idx", fwd_idx), ("mutual", mutual)):
            if not _is_integral(x):
                raise ValueError(f"{name} must be integers")
        fi = _as(fwd_idx, np.int64, torch.int64)
        mu = _as(mutual, np.uint8, torch.uint8)
        if fi.ndim != 2 or fi.shape[0] != nq or not 1 <= fi.shape[1] <= MAX_CANDIDATES:
            raise ValueError(f"fwd_idx must be [nq={nq}][C] with 1 <= C <= {MAX_CANDIDATES}, got shape {tuple(fi.shape)}")
        if tuple(mu.shape) != tuple(fi.shape):
            raise ValueError(f"mutual must have fwd_idx's shape {tuple(fi.shape)}, got {tuple(mu.shape)}")
        tol, min_scale, max_scale = float(tol), float(min_scale), float(max_scale)
        if not (np.isfinite(tol) and tol > 0):
            raise ValueError(f"tol={tol} must be finite and > 0")
        if not (0 < min_scale <= max_scale < float("inf")):
            raise ValueError(f"need 0 < min_scale <= max_scale < inf, got {min_scale}, {max_scale}")
        qo = np.ascontiguousarray(qo, dtype=np.int32)
        n_img, Cw = len(qo) - 1, int(fi.shape[1])
        out = {"n_inlier": self._empty((n_img, Cw), torch.int32), "pair": self._empty((n_img, Cw, 2), torch.int32),
               "model": self._empty((n_img, Cw, 4), torch.float64), "order": self._empty((n_img, Cw), torch.int32)}
        if want_rows:
            out["inlier"] = self._empty((nq, Cw), torch.uint8)
        self._stream()
        self._check(self.lib.segvlad_verify_pairs(self._h, _ptr(qx), nq, _ptr(rx), n_r, _ptr(qo), n_img, Cw, _ptr(fi), _ptr(mu), tol,
                                                  min_scale, max_scale, _ptr(out["n_inlier"]), _ptr(out["pair"]), _ptr(out["model"]),
                                                  _ptr(out["order"]), _ptr(out.get("inlier"))), "verify_pairs")
        self._keep = [qx, rx, fi, mu]
        return out

    def sequence_rerank(self, cand, score, seq_offsets=None, back: int = 5, fwd: int = 5, velocities=None, tol: int = 1,
                        want_all: bool = True) -> dict:
        """segvlad_sequence_rerank: every candidate of every query frame scored by the support it finds in the frames around it.
        ``cand`` int32 [T][C] (vote()'s ``pred`` as it is; -1: empty) and ``score`` fp64 [T][C] (its scores, or ``n_mutual`` /
        ``n_inlier``; converted to fp64), device or host, C <= 64; the frames are in time order and the image ids are frame
        numbers along the map.  ``seq_offsets`` [n_seq + 1] (host; None: one sequence) splits the frames into sequences no
        window crosses; a candidate r of frame t collects, for each of the ``velocities`` (map frames per query frame; None:
        velocity_grid()), the best score within ``tol`` map frames of r + rint(v tau) in every frame t + tau, -back <= tau <=
        fwd, and keeps the best velocity.  Malformed arguments raise ValueError.  Returns device tensors: ``seq_score`` fp64
        [T][C] and ``order`` int32 [T][C] (the slots by (seq_score desc, slot asc), empty slots last); with ``want_all`` also
        ``n_hit`` int32 [T][C] (the frames that supported the winner) and ``vel`` int32 [T][C] (its index; -1: empty slot)."""
        if not _is_integral(cand):
            raise ValueError("cand must be integers")
        c = _as(cand, np.int32, torch.int32)
        s = _as(score, np.float64, torch.float64)
        if c.ndim != 2 or tuple(s.shape) != tuple(c.shape):
            raise ValueError(f"cand and score must both be [T][C], got shapes {tuple(c.shape)} and {tuple(s.shape)}")
        T, Cw = int(c.shape[0]), int(c.shape[1])
        so, vel = check_sequence_args(T, Cw, seq_offsets, back, fwd, velocities, tol)
        out = {"seq_score": self._empty((T, Cw), torch.float64), "order": self._empty((T, Cw), torch.int32)}
        if want_all:
            out["n_hit"] = self._empty((T, Cw), torch.int32)
            out["vel"] = self._empty((T, Cw), torch.int32)
        self._stream()
        self._check(self.lib.segvlad_sequence_rerank(self._h, _ptr(c), _ptr(s), T, Cw, _ptr(so), len(so) - 1, int(back), int(fwd),
                                                     _ptr(vel), len(vel), int(tol), _ptr(out["seq_score"]), _ptr(out.get("n_hit")),
                                                     _ptr(out.get("vel")), _ptr(out["order"])), "sequence_rerank")
        self._keep = [c, s]
        return out

    def exclude_stats(self) -> dict:
        """Statistics of the last search_excluding(): the depth of the inner search, the largest number of index rows a query
        image excluded, the query rows the exact tail finished, the query images that excluded any row.  Synchronises."""
        v = (C.c_int64 * 4)()
        self._check(self.lib.segvlad_exclude_stats(self._h, v, 4), "exclude_stats")
        return dict(zip(("k_fetch", "x_max", "tail_rows", "n_img_excluding"), [int(x) for x in v]))

    def range_search(self, Q, radius2, qseg_offsets=None, capacity: Optional[int] = None):
        """segvlad_range_search: every index row with ``d2 < radius2`` of each query row (strictly; faiss range_search), the
        distances bit for bit search()'s.  ``radius2``: SQUARED radii -- a scalar, ``[nq]`` (host, or a device tensor used
        as it is), or with ``qseg_offsets`` one per query image (radius2_from_sim gives the radius of a similarity floor).
        Returns device tensors ``(lims [nq + 1] int64, d2 [total] fp32, idx [total] int64)``: row q's hits, ascending
        (d2, lower id), are ``lims[q] .. lims[q + 1] - 1``.  The first call offers ``capacity`` slots (default: the previous
        call's total, else 4 nq); when the hits do not fit it is repeated once with the total it reported."""
        q = _as(Q, np.float32, torch.float32)
        nq = int(q.shape[0])
        if isinstance(radius2, torch.Tensor) and radius2.is_cuda and radius2.dim() == 1 and qseg_offsets is None:
            if tuple(radius2.shape) != (nq,):
                raise ValueError(f"radius2 must be a scalar or [nq={nq}], got shape {tuple(radius2.shape)}")
            r = radius2.to(torch.float32).contiguous()
        else:
            r = expand_radius2(radius2, nq, qseg_offsets)
        if capacity is None:
            capacity = getattr(self, "_range_total", 0) or 4 * nq
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        lims = self._empty((nq + 1,), torch.int64)
        total = C.c_int64()
        self._stream()
        self.range_retried = False
        while True:
            d2 = self._empty((capacity,), torch.float32)
            idx = self._empty((capacity,), torch.int64)
            self._check(self.lib.segvlad_range_search(self._h, _ptr(q), nq, _ptr(r), _ptr(lims), _ptr(d2) if capacity else None,
                                                      _ptr(idx) if capacity else None, capacity, C.byref(total)), "range_search")
            if total.value <= capacity:
                break
            capacity = int(total.value)
            self.range_retried = True
        self._range_total = int(total.value)
        self._keep = [q, r]
        return lims, d2[:total.value], idx[:total.value]

    def range_stats(self) -> dict:
        """Statistics of the last range_search(): total hits, query rows finished by the long-row path, the longest and the
        sum of the candidate lists the filter produced, the path taken ("exact" distance blocks or the "f16" filter)."""
        v = (C.c_int64 * 5)()
        self._check(self.lib.segvlad_range_stats(self._h, v, 5), "range_stats")
        d = dict(zip(("total", "long_rows", "cand_max", "cand_sum", "path"), [int(x) for x in v]))
        d["path"] = {0: "exact", 1: "f16"}[d["path"]]
        return d

    def merge_topk(self, d2_parts, idx_parts, parts: int, k: int):
        d = _as(d2_parts, np.float32, torch.float32)
        i = _as(idx_parts, np.int64, torch.int64)
        nq = d.shape[0]
        assert d.shape[1] == parts * k and i.shape == d.shape
        od = self._empty((nq, k), torch.float32)
        oi = self._empty((nq, k), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_merge_topk(self._h, _ptr(d), _ptr(i), nq, parts, k, _ptr(od), _ptr(oi)), "merge_topk")
        self._keep = [d, i]
        return od, oi

    def sims_from_d2(self, d2, idx, k_keep: int):
        d = _as(d2, np.float32, torch.float32)
        i = _as(idx, np.int64, torch.int64)
        nq, k_in = d.shape
        s = self._empty((nq, k_keep), torch.float32)
        oi = self._empty((nq, k_keep), torch.int64)
        self._stream()
        self._check(self.lib.segvlad_sims_from_d2(self._h, _ptr(d), _ptr(i), nq, k_in, k_keep, _ptr(s), _ptr(oi)), "sims_from_d2")
        self._keep = [d, i]
        return s, oi

    def minmax(self, sims) -> torch.Tensor:
        s = _as(sims, np.float32, torch.float32)
        out = self._empty((2,), torch.float32)
        self._stream()
        self._check(self.lib.segvlad_minmax(self._h, _ptr(s), s.numel() if isinstance(s, torch.Tensor) else s.size, _ptr(out)), "minmax")
        self._keep = [s]
        return out

    def vote(self, idx, sims, qseg_offsets, n_top=5, mode=_lib.VOTE_WT_BORDA_IM, img_of_seg=None, smin=float("nan"),
             smax=float("nan"), want_scores=True, per_image=None, unique_ref=False):
        """segvlad_vote.  ``per_image`` (1 .. 255): every query segment gives a reference image at most that many hits -- the
        vote over blank_capped(idx, img_of_seg, per_image), bit for bit (SEGVLAD_VOTE_PER_IMAGE; an int ``mode`` that already
        carries the bits is accepted as it is).  ``unique_ref``: a reference segment votes once per query image -- the vote over
        blank_unique(idx, sims, qseg_offsets, n_ref_seg), bit for bit (SEGVLAD_VOTE_UNIQUE_REF); the most similar of an image's
        claims on a segment wins wherever ``sims`` is given, COUNT included, the first visited without.  With both, the cap is
        applied to the one-to-one lists."""
        mode = _lib.vote_mode(mode, per_image, unique_ref)
        i = _as(idx, np.int64, torch.int64)
        s = None if sims is None else _as(sims, np.float32, torch.float32)
        qo = np.ascontiguousarray(qseg_offsets, dtype=np.int32)
        n_img = len(qo) - 1
        k = i.shape[1]
        im = None if img_of_seg is None else _as(img_of_seg, np.int32, torch.int32)
        n_ref = 0 if im is None else int(im.shape[0])
        pred = self._empty((n_img, n_top), torch.int32)
        sc = self._empty((n_img, n_top), torch.float64) if want_scores else None
        self._stream()
        self._check(self.lib.segvlad_vote(self._h, _ptr(i), _ptr(s), _ptr(im), n_ref, _ptr(qo), n_img, k, smin, smax, n_top,
                                          int(mode), _ptr(pred), _ptr(sc)), "vote")
        self._keep = [i, s, im]
        return pred, sc
