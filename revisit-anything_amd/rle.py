"""Run-length masks as SAM emits them: the uncompressed RLE of ``mask_to_rle_pytorch`` / ``rle_to_mask``
(sam/segment_anything/utils/amg.py:107-149) for a whole batch, in the layout segvlad_incidence_rle and segvlad_rle_decode take.

One record of SAM is ``{"size": [h, w], "counts": [...]}``: the mask flattened column-major (pixel ``p = col * h + row``),
alternating runs of zeros and ones that start with zeros (the first count is 0 for a mask whose first pixel is set).  A batch
here is the records of S masks of ONE size, concatenated:

    counts       uint32 [n_runs]   the runs of all masks one after the other
    run_offsets  int64  [S + 1]    mask s owns counts[run_offsets[s] : run_offsets[s + 1]]
    Hm, Wm                         the masks' size

Dense masks become a batch in two places: ``RleMasks.from_dense`` on the host (NumPy; a device tensor is copied to the host
first and the result is host arrays), and ``SegVLADEngine.rle_encode`` on the device (segvlad_rle_encode,
csrc/rle_encode_kernels.hip: device tensors in, device tensors out, the same counts).  ``areas()`` is ``area_from_rle``.

Out of scope: COCO's compressed string form of the counts (``coco_rle``)."""
from __future__ import annotations

from typing import Mapping, Optional, Sequence

import numpy as np
import torch

RLE_CHUNK_RUNS = 512   # runs per step of the kernels' run walk (csrc/rle_kernels.hip: RLE_CHUNK)
RLE_ENCODE_ROWS = 256  # rows of one unit of the device encoder (csrc/rle_encode_kernels.hip: RLE_ENCODE_ROWS)


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


class RleMasks:
    """S run-length masks of one size.  ``counts`` / ``run_offsets`` are NumPy arrays (host) or torch tensors (host or device,
    see ``to``).  The constructor checks the batch on the host -- offsets from 0 to len(counts), non-decreasing, every mask's
    counts summing to Hm * Wm -- and raises ValueError otherwise (``validate=False``: the caller vouches for it)."""

    __hash__ = None

    def __init__(self, counts, run_offsets, Hm: int, Wm: int, validate: bool = True):
        self.Hm, self.Wm = int(Hm), int(Wm)
        if self.Hm <= 0 or self.Wm <= 0:
            raise ValueError(f"mask size must be positive, got {Hm} x {Wm}")
        if self.Hm * self.Wm > np.iinfo(np.uint32).max:
            raise ValueError(f"{Hm} x {Wm} pixels do not fit a 32-bit count")
        if isinstance(counts, torch.Tensor) or isinstance(run_offsets, torch.Tensor):
            self.counts = torch.as_tensor(counts).to(torch.uint32).contiguous() if not (
                isinstance(counts, torch.Tensor) and counts.dtype == torch.uint32) else counts.contiguous()
            self.run_offsets = torch.as_tensor(run_offsets).to(device=self.counts.device, dtype=torch.int64).contiguous()
        else:
            c = np.asarray(counts)
            if c.size and (c.dtype.kind not in "iu" or int(c.min()) < 0 or int(c.max()) > np.iinfo(np.uint32).max):
                raise ValueError("counts must be integers in 0 .. 2^32 - 1")
            self.counts = np.ascontiguousarray(c, dtype=np.uint32).reshape(-1)
            self.run_offsets = np.ascontiguousarray(run_offsets, dtype=np.int64)
        if validate:
            self._validate()

    def _validate(self) -> None:
        c, o = _host(self.counts, np.uint32), _host(self.run_offsets, np.int64)
        if c.ndim != 1 or o.ndim != 1 or len(o) < 1:
            raise ValueError("counts must be [n_runs] and run_offsets [S + 1]")
        if o[0] != 0 or o[-1] != len(c) or (np.diff(o) < 0).any():
            raise ValueError("run_offsets must run from 0 to len(counts) without decreasing")
        cs = np.concatenate([[0], np.cumsum(c, dtype=np.int64)])
        sums = cs[o[1:]] - cs[o[:-1]]
        bad = np.nonzero(sums != self.Hm * self.Wm)[0]
        if len(bad):
            raise ValueError(f"mask {int(bad[0])}: counts sum to {int(sums[bad[0]])}, not Hm * Wm = {self.Hm * self.Wm}"
                             f" ({len(bad)} such mask(s))")

    # ---- constructors --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, masks) -> "RleMasks":
        """``masks`` [S, Hm, Wm] (or one [Hm, Wm]) of any dtype, non-zero = true -> the counts mask_to_rle_pytorch emits."""
        m = masks.detach().cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3:
            raise ValueError(f"masks must be [S, Hm, Wm], got {m.shape}")
        S, Hm, Wm = m.shape
        P = Hm * Wm
        if Hm <= 0 or Wm <= 0 or P > np.iinfo(np.uint32).max:
            raise ValueError(f"unsupported mask size {Hm} x {Wm}")
        f = np.ascontiguousarray((m != 0).transpose(0, 2, 1)).reshape(S, P)          # column-major pixels
        si, pi = np.nonzero(f[:, 1:] != f[:, :-1])                                    # value changes, by mask, then by pixel
        n_ch = np.bincount(si, minlength=S).astype(np.int64)
        first = f[:, 0].astype(np.int64)                                              # a set first pixel: a leading run of 0 zeros
        # every mask's edges 0, change + 1 ..., P in one array; the run lengths are the differences inside a mask
        eoff = np.concatenate([[0], np.cumsum(n_ch + 2)])
        edges = np.empty(int(eoff[-1]), np.int64)
        edges[eoff[:-1]] = 0
        edges[eoff[1:] - 1] = P
        rank = np.arange(len(si), dtype=np.int64) - (np.cumsum(n_ch) - n_ch)[si]
        edges[eoff[si] + 1 + rank] = pi + 1
        lengths = np.diff(edges)
        keep = np.ones(len(lengths), bool)
        keep[eoff[1:-1] - 1] = False                                                  # (the step from one mask's P to the next one's 0)
        lengths = lengths[keep]
        run_offsets = np.concatenate([[0], np.cumsum(n_ch + 1 + first)]).astype(np.int64)
        counts = np.zeros(int(run_offsets[-1]), np.uint32)
        loff = np.cumsum(n_ch + 1) - (n_ch + 1)
        counts[np.arange(len(lengths), dtype=np.int64) + np.repeat(run_offsets[:-1] + first - loff, n_ch + 1)] = lengths
        return cls(counts, run_offsets, Hm, Wm, validate=False)

    @classmethod
    def from_sam(cls, records: Sequence, size: Optional[Sequence[int]] = None) -> "RleMasks":
        """SAM's ``{"size": [h, w], "counts": [...]}`` dicts, or records whose ``"segmentation"`` is such a dict
        (``output_mode="uncompressed_rle"``).  ``size``: the batch's (h, w), needed only for an empty list."""
        rles = []
        for r in records:
            r = r["segmentation"] if isinstance(r, Mapping) and "segmentation" in r else r
            if not isinstance(r, Mapping) or "size" not in r or "counts" not in r:
                raise ValueError("a record must be {'size': [h, w], 'counts': [...]} or hold one under 'segmentation'")
            if isinstance(r["counts"], (str, bytes)):
                raise ValueError("compressed (coco_rle) counts are not supported: pass the uncompressed_rle form")
            rles.append(r)
        sizes = {tuple(int(v) for v in r["size"]) for r in rles} | ({tuple(int(v) for v in size)} if size is not None else set())
        if len(sizes) != 1:
            raise ValueError(f"one size per batch, got {sorted(sizes)}" if sizes else "no records and no size")
        (Hm, Wm), = sizes
        per = [np.asarray(r["counts"], dtype=np.int64).reshape(-1) for r in rles]
        counts = np.concatenate(per) if per else np.zeros(0, np.int64)
        run_offsets = np.concatenate([[0], np.cumsum([len(p) for p in per], dtype=np.int64)]).astype(np.int64)
        return cls(counts, run_offsets, Hm, Wm)

    @classmethod
    def concat(cls, parts: Sequence["RleMasks"]) -> "RleMasks":
        parts = list(parts)
        if not parts:
            raise ValueError("concat needs at least one batch")
        if len({(p.Hm, p.Wm) for p in parts}) != 1:
            raise ValueError(f"one size per batch, got {sorted({(p.Hm, p.Wm) for p in parts})}")
        counts = np.concatenate([_host(p.counts, np.uint32) for p in parts])
        offs, base = [np.zeros(1, np.int64)], 0
        for p in parts:
            o = _host(p.run_offsets, np.int64)
            offs.append(o[1:] + base)
            base += int(o[-1])
        return cls(counts, np.concatenate(offs), parts[0].Hm, parts[0].Wm, validate=False)

    # ---- views ---------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self.run_offsets.shape[0]) - 1

    @property
    def size(self):
        return [self.Hm, self.Wm]

    @property
    def nbytes(self) -> int:
        """bytes of counts + run_offsets (what a caller stores or moves instead of S * Hm * Wm mask bytes)"""
        return int(self.counts.shape[0]) * 4 + int(self.run_offsets.shape[0]) * 8

    @property
    def device(self):
        return self.counts.device if isinstance(self.counts, torch.Tensor) else torch.device("cpu")

    def to(self, device) -> "RleMasks":
        """The batch as torch tensors on ``device`` (uint32 counts, int64 run_offsets); not validated again."""
        c = self.counts if isinstance(self.counts, torch.Tensor) else torch.from_numpy(self.counts)
        o = self.run_offsets if isinstance(self.run_offsets, torch.Tensor) else torch.from_numpy(self.run_offsets)
        return RleMasks(c.to(device), o.to(device), self.Hm, self.Wm, validate=False)

    def to_dense(self) -> np.ndarray:
        """bool [S, Hm, Wm] on the host (rle_to_mask per mask)"""
        c, o = _host(self.counts, np.uint32), _host(self.run_offsets, np.int64)
        n = np.diff(o)
        parity = ((np.arange(len(c), dtype=np.int64) - np.repeat(o[:-1], n)) & 1).astype(bool)
        flat = np.repeat(parity, c)
        if flat.size != len(self) * self.Hm * self.Wm:
            raise ValueError("the counts do not cover the masks")
        return flat.reshape(len(self), self.Wm, self.Hm).transpose(0, 2, 1)

    def arrays(self):
        """(counts uint32, run_offsets int64) as host NumPy arrays"""
        return _host(self.counts, np.uint32), _host(self.run_offsets, np.int64)

    def mask(self, j: int) -> np.ndarray:
        """Mask j alone: bool [Hm, Wm] (rle_to_mask)"""
        c, o = self.arrays()
        runs = c[o[j]:o[j + 1]]
        flat = np.repeat((np.arange(len(runs)) & 1).astype(bool), runs)
        if flat.size != self.Hm * self.Wm:
            raise ValueError(f"mask {j}: the counts do not cover the mask")
        return flat.reshape(self.Wm, self.Hm).transpose()

    def areas(self) -> np.ndarray:
        """Set pixels of every mask, int64 [S] on the host: the sum of its odd-indexed runs (area_from_rle, utils/amg.py)"""
        c, o = _host(self.counts, np.uint32), _host(self.run_offsets, np.int64)
        odd = ((np.arange(len(c), dtype=np.int64) - np.repeat(o[:-1], np.diff(o))) & 1).astype(bool)
        cs = np.concatenate([[0], np.cumsum(np.where(odd, c, 0), dtype=np.int64)])
        return (cs[o[1:]] - cs[o[:-1]]).astype(np.int64)

    def to_sam(self) -> list:
        """One ``{"size": [Hm, Wm], "counts": [...]}`` per mask"""
        c, o = _host(self.counts, np.uint32), _host(self.run_offsets, np.int64)
        return [{"size": [self.Hm, self.Wm], "counts": c[o[s]:o[s + 1]].tolist()} for s in range(len(self))]

    def __eq__(self, other) -> bool:
        if not isinstance(other, RleMasks):
            return NotImplemented
        return ((self.Hm, self.Wm) == (other.Hm, other.Wm)
                and np.array_equal(_host(self.counts, np.uint32), _host(other.counts, np.uint32))
                and np.array_equal(_host(self.run_offsets, np.int64), _host(other.run_offsets, np.int64)))

    def __repr__(self) -> str:
        return f"RleMasks(S={len(self)}, {self.Hm}x{self.Wm}, runs={int(self.counts.shape[0])}, device={self.device})"
