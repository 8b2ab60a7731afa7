"""Row-sharded exact segment index over the GPUs of one node (one process per GPU).

The reference is single-process; sharding is the build's own layer:

* the reference-segment rows are split into contiguous blocks, rank r keeps rows
  [row_start[r], row_start[r+1]) and answers queries against its block only;
* every rank sees the full query batch, computes its local top-k (distance, GLOBAL segment id),
  then ONE all_gather (RCCL over xGMI when the backend is "nccl") exchanges the per-shard lists as
  packed 12-byte records {fp32 distance bits, int64 id}: nq * k * 12 B per rank;
* every rank merges the world*k candidates per query segment to the global top-k -- by distance,
  ties by lower global id, i.e. exactly what a single index over all rows returns -- and votes.

The compute is delegated to a backend object with the SegVLADEngine interface (db_reset, db_add,
db_remove, search, merge_topk, sims_from_d2, vote); the distributed plumbing below is backend-agnostic so
that it can be exercised with gloo on CPU (tests/test_sharded_gloo.py) with a checker backend.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from ._lib import vote_mode


def shard_bounds(n_rows: int, world: int) -> np.ndarray:
    """Contiguous, balanced row blocks: row_start[r] = floor(r * n / world)."""
    return np.array([(r * n_rows) // world for r in range(world + 1)], dtype=np.int64)


def shard_images(n_images: int, world: int) -> np.ndarray:
    """Contiguous image blocks (a reference image's segments never straddle two ranks)."""
    return np.array([(r * n_images) // world for r in range(world + 1)], dtype=np.int64)


def removal_keep_mask(img_of_seg: torch.Tensor, row_ids=None, img_ids=None) -> torch.Tensor:
    """The keep flag [n] of every row of an index whose segment -> image map is ``img_of_seg`` [n] after removing the rows listed
    in ``row_ids`` and the rows of the images listed in ``img_ids`` (segvlad_db_remove's rule: out-of-range ids, negative image ids
    and duplicates are ignored).  On img_of_seg's device."""
    n = int(img_of_seg.shape[0])
    dev = img_of_seg.device
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    if row_ids is not None:
        r = torch.as_tensor(np.asarray(row_ids) if not isinstance(row_ids, torch.Tensor) else row_ids).reshape(-1).to(dev, torch.int64)
        keep[r[(r >= 0) & (r < n)]] = False
    if img_ids is not None and n:
        g = torch.as_tensor(np.asarray(img_ids) if not isinstance(img_ids, torch.Tensor) else img_ids).reshape(-1).to(dev, torch.int64)
        top = int(img_of_seg.max()) if n else -1
        g = g[(g >= 0) & (g <= top)]
        if g.numel():
            gone = torch.zeros(top + 1, dtype=torch.bool, device=dev)
            gone[g] = True
            im = img_of_seg.to(torch.int64)
            keep &= ~torch.where(im >= 0, gone[im.clamp(min=0)], torch.zeros_like(keep))
    return keep


class ShardedSegmentIndex:
    """A reference index split by rows over the ranks.  Excluding image-id windows per query image (engine.search_excluding)
    is a single-index feature for now: the row-sharded search has no such form."""

    def __init__(self, backend, rank: Optional[int] = None, world: Optional[int] = None, group=None,
                 device: Optional[torch.device] = None, native_comm: bool = False):
        """native_comm: exchange through the C-ABI's own RCCL communicator (segvlad_comm_init / segvlad_search_sharded /
        segvlad_allgather_rows: pack, all-gather, unpack and merge on the context's stream, no torch collective on the data
        path) instead of torch.distributed; the 128-byte communicator id still travels over torch.distributed's host
        channel.  What a C caller of include/segvlad.h gets."""
        self.be = backend
        self.native = bool(native_comm)
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = rank if rank is not None else (dist.get_rank(group) if self.distributed else 0)
        self.world = world if world is not None else (dist.get_world_size(group) if self.distributed else 1)
        self.device = device if device is not None else getattr(backend, "device", torch.device("cpu"))
        self.row_start = np.zeros(self.world + 1, dtype=np.int64)
        self.n_local = 0
        self.img_of_seg_global: Optional[torch.Tensor] = None
        # profile_collectives(True): every collective on the data path is bracketed by a pair of events on the current stream;
        # collective_ms() sums them per name (the N > 1 bench line carries them per rank, with the bytes of collective_bytes())
        self._coll_events = None

    # ---- what travels, and how long it takes --------------------------------------------------------------------------
    def profile_collectives(self, on: bool = True):
        self._coll_events = [] if on else None

    def _timed(self, name: str, fn):
        if self._coll_events is None or self.device.type != "cuda":
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self._coll_events.append((name, e0, e1))
        return out

    def collective_ms(self) -> dict:
        """{collective name: summed milliseconds since profile_collectives(True)} (synchronises on the recorded events)."""
        out: dict = {}
        for name, e0, e1 in self._coll_events or []:
            e1.synchronize()
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        if self._coll_events is not None:
            self._coll_events = []
        return out

    @staticmethod
    def collective_bytes(world: int, nq: int, k: int, d: int, rows_per_rank: Sequence[int]) -> dict:
        """Bytes every rank SENDS / RECEIVES per retrieve(): the all-gather of the query descriptors (fp32 rows; ragged slices are
        padded to the longest) and the all-gather of the per-shard top-k as packed 12-byte records."""
        mx = max(int(r) for r in rows_per_rank) if len(rows_per_rank) else 0
        return {"query_rows_allgather_send": mx * d * 4, "query_rows_allgather_recv": world * mx * d * 4,
                "topk_records_allgather_send": nq * k * 12, "topk_records_allgather_recv": world * nq * k * 12}

    # ---- build --------------------------------------------------------------------------------------
    def build(self, local_rows, local_img_of_seg):
        """local_rows [n_local, d] (this rank's block, in global row order), local_img_of_seg [n_local]
        with GLOBAL reference-image ids.  Exchanges the block sizes and the (small) segment->image map."""
        self.be.db_reset()
        n_local = int(local_rows.shape[0])
        counts = [n_local]
        if self.world > 1:
            t = torch.tensor([n_local], dtype=torch.int64, device=self.device)
            allc = [torch.zeros_like(t) for _ in range(self.world)]
            dist.all_gather(allc, t, group=self.group)
            counts = [int(c.item()) for c in allc]
        self.row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_local = n_local
        img = torch.as_tensor(np.asarray(local_img_of_seg) if not isinstance(local_img_of_seg, torch.Tensor) else local_img_of_seg)
        img = img.to(torch.int32).to(self.device)
        if self.world > 1:
            mx = max(counts)
            pad = torch.full((mx,), -1, dtype=torch.int32, device=self.device)
            pad[:n_local] = img
            parts = [torch.empty_like(pad) for _ in range(self.world)]
            dist.all_gather(parts, pad, group=self.group)
            img = torch.cat([p[:c] for p, c in zip(parts, counts)])
        self.img_of_seg_global = img.contiguous()
        if n_local:
            self.be.db_add(local_rows, None)
        if self.native:
            uid = [self.be.comm_unique_id() if self.rank == 0 else None]
            if self.world > 1:
                dist.broadcast_object_list(uid, src=0, group=self.group)
            self.be.comm_init(uid[0], self.rank, self.world)

    @property
    def n_total(self) -> int:
        return int(self.row_start[-1])

    # ---- removal ------------------------------------------------------------------------------------
    def remove(self, row_ids=None, img_ids=None) -> int:
        """Removes rows by GLOBAL row id and / or by reference image id; the survivors keep their order and their global ids
        move down, exactly as one index over all rows (segvlad_db_remove).  Collective: every rank passes the same lists.  Each
        rank derives the global keep mask from img_of_seg_global (the rank engines hold no image map: image removal becomes row
        removal), removes its own rows, and takes the new row_start and the compacted map.  One all-gather of every rank's view
        -- the kept rows per shard and a checksum of the removed ids -- comes first: if any rank was given other lists, every
        rank raises before any shard changes.  Shards may become uneven (no rebalancing).  Returns the number of rows removed."""
        keep = removal_keep_mask(self.img_of_seg_global, row_ids, img_ids)
        bounds = [int(b) for b in self.row_start]
        kept = [int(keep[bounds[r]:bounds[r + 1]].sum()) for r in range(self.world)]
        gone = torch.nonzero(~keep).reshape(-1).to(torch.int64)
        view = torch.tensor(kept + [int(gone.sum()), int((gone * gone % 1000000007).sum())], dtype=torch.int64, device=self.device)
        if self.world > 1:
            views = [torch.zeros_like(view) for _ in range(self.world)]
            dist.all_gather(views, view, group=self.group)
            if any(not torch.equal(v, views[0]) for v in views):
                from ._lib import SegVLADError

                raise SegVLADError("ShardedSegmentIndex.remove: the ranks were given different removal lists (no shard changed)")
        lo, hi = bounds[self.rank], bounds[self.rank + 1]
        local = gone[(gone >= lo) & (gone < hi)] - lo
        if local.numel():
            self.be.db_remove(row_ids=local)
        self.row_start = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
        self.n_local = kept[self.rank]
        self.img_of_seg_global = self.img_of_seg_global[keep].contiguous()
        return int(gone.numel())

    # ---- query descriptors: every rank describes a slice of the query images, all ranks need all rows -----------
    def gather_rows(self, local_rows: torch.Tensor, rows_per_rank: Sequence[int]) -> torch.Tensor:
        """Concatenation, in rank order, of every rank's ``local_rows`` ([rows_per_rank[r], d]) -- one all_gather
        (RCCL over xGMI with the nccl backend).  Slices may be ragged: short ones are padded to the longest for the
        collective and trimmed afterwards."""
        rows_per_rank = [int(r) for r in rows_per_rank]
        if len(rows_per_rank) != self.world:
            raise ValueError("rows_per_rank must have one entry per rank")
        if int(local_rows.shape[0]) != rows_per_rank[self.rank]:
            raise ValueError(f"rank {self.rank} holds {int(local_rows.shape[0])} rows, rows_per_rank says {rows_per_rank[self.rank]}")
        if self.world == 1:
            return local_rows
        mx = max(rows_per_rank)
        x = local_rows.contiguous()
        if self.native and min(rows_per_rank) == mx and x.dim() == 2 and x.dtype == torch.float32:
            # (the C-ABI gathers fp32 rows; any other type keeps torch.distributed's collective and its dtype)
            return self._timed("query_rows_allgather", lambda: self.be.allgather_rows(x, world=self.world))
        if min(rows_per_rank) == mx:   # equal slices (the usual case): ONE all_gather_into_tensor, no padding, no trimming
            out = torch.empty((self.world * mx,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            self._timed("query_rows_allgather", lambda: dist.all_gather_into_tensor(out, x, group=self.group))
            return out
        if x.shape[0] < mx:
            x = torch.cat([x, x.new_zeros((mx - x.shape[0],) + tuple(x.shape[1:]))])
        parts = [torch.empty_like(x) for _ in range(self.world)]
        self._timed("query_rows_allgather", lambda: dist.all_gather(parts, x, group=self.group))
        return torch.cat([p[:n] for p, n in zip(parts, rows_per_rank)])

    # ---- query --------------------------------------------------------------------------------------
    def search(self, Q, k: int, k_local: Optional[int] = None):
        """Global top-k over all shards: (d2 [nq,k] ascending, idx [nq,k] GLOBAL ids), identical on every rank.
        k_local >= k: search depth used on each shard before the exchange (only the first k columns travel:
        the global top-k is contained in the union of the per-shard top-k lists)."""
        nq = int(Q.shape[0])
        if self.native:   # local search, packed all-gather, merge: one C-ABI call on the context's stream
            # (its all-gather sits inside the C-ABI call: the event pair brackets local search + exchange + merge)
            return self._timed("native_search_sharded", lambda: self.be.search_sharded(Q, k, int(self.row_start[self.rank])))
        if self.world == 1 and self.n_local and (k_local is None or k_local <= k):
            # a single index: the engine's result as it is (no id offset, no slice: four small torch kernels and their launch
            # gaps per call otherwise -- 0.1 ms of a 26-ms step)
            d2, idx = self.be.search(Q, k)
            return torch.as_tensor(d2).to(self.device), torch.as_tensor(idx).to(self.device)
        if self.n_local:
            d2, idx = self.be.search(Q, max(k, k_local or k))
            d2 = torch.as_tensor(d2).to(self.device)[:, :k].contiguous()
            idx = torch.as_tensor(idx).to(self.device)[:, :k].contiguous()
            idx = torch.where(idx >= 0, idx + int(self.row_start[self.rank]), idx)
        else:
            d2 = torch.full((nq, k), float("inf"), dtype=torch.float32, device=self.device)
            idx = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        if self.world == 1:
            return d2, idx
        d2c, idc = self.exchange_topk(d2, idx)
        md, mi = self.be.merge_topk(d2c, idc, self.world, k)
        return torch.as_tensor(md), torch.as_tensor(mi)

    def exchange_topk(self, d2: torch.Tensor, idx: torch.Tensor):
        """ONE collective for the per-shard lists: (d2 fp32, global id int64) travel as a packed 12-byte record
        {fp32 bits, id low, id high}; returns ([nq, world*k] d2, [nq, world*k] ids), shard-major within a row.
        (Also valid at world size 1, which is how the RCCL path is smoke-tested on a 1-GPU box.)"""
        nq, k = int(d2.shape[0]), int(d2.shape[1])
        rec = self.pack_topk_records(d2, idx)
        allrec = torch.empty((self.world * nq, k, 3), dtype=torch.int32, device=self.device)   # rank-major concatenation
        self._timed("topk_records_allgather", lambda: dist.all_gather_into_tensor(allrec, rec, group=self.group))
        return self.unpack_topk_records(allrec, self.world)

    @staticmethod
    def pack_topk_records(d2: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """[nq, k] (fp32 d2, int64 global id) -> [nq, k, 3] int32 records {fp32 bits, id low, id high}, contiguous: what a rank
        hands to the all-gather."""
        if d2.dtype != torch.float32 or idx.dtype != torch.int64 or d2.shape != idx.shape or d2.dim() != 2:
            raise ValueError(f"pack_topk_records: want fp32 / int64 [nq, k] pairs, got {d2.dtype}{tuple(d2.shape)} / {idx.dtype}{tuple(idx.shape)}")
        nq, k = int(d2.shape[0]), int(d2.shape[1])
        rec = torch.empty((nq, k, 3), dtype=torch.int32, device=d2.device)
        rec[:, :, 0] = d2.contiguous().view(torch.int32)
        rec[:, :, 1:] = idx.contiguous().view(torch.int32).view(nq, k, 2)
        return rec

    @staticmethod
    def unpack_topk_records(allrec: torch.Tensor, world: int):
        """The all-gather's output -- the ranks' record blocks concatenated in rank order, [world * nq, k, 3] int32 -- as
        ([nq, world * k] fp32 d2, [nq, world * k] int64 ids), shard-major within a row (what merge_topk takes)."""
        if allrec.dtype != torch.int32 or allrec.dim() != 3 or allrec.shape[2] != 3 or allrec.shape[0] % world or not allrec.is_contiguous():
            raise ValueError(f"unpack_topk_records: want a contiguous int32 [world * nq, k, 3] block, got {allrec.dtype}{tuple(allrec.shape)}")
        nq, k = int(allrec.shape[0]) // world, int(allrec.shape[1])
        r = allrec.view(world, nq, k, 3).permute(1, 0, 2, 3)                                    # [nq, world, k, 3]
        d2c = r[..., 0].contiguous().view(torch.float32).view(nq, world * k)
        idc = r[..., 1:].contiguous().view(torch.int64).view(nq, world * k)
        return d2c, idc

    def retrieve(self, Q, qseg_offsets: Sequence[int], k_search: int = 200, k_vote: int = 50, n_top: int = 5, mode: int = 0,
                 want_scores: bool = False, vote_depth_only: bool = False, votes_per_image=None, vote_unique_ref=False):
        """search -> keep k_vote, 2-d^2 -> vote with the global segment->image map.  The global min/max of the
        vote (func_vpr.py:212-213) is taken over the merged (global) similarities, so it needs no extra collective.
        vote_depth_only: a caller that does not keep the k_search-wide lists (place_rec_main.py:61-75 pickles them only under
        save_results) may have a single index search k_vote deep as well -- same first k_vote columns, same votes.
        votes_per_image (1 .. 255): at most that many hits per reference image from each query segment, capped in the vote
        (the backend's vote takes it in ``mode``, _lib.vote_mode): the lists are the merged global ones, so the result is the
        single index's.  vote_unique_ref: a reference segment votes once per query image (SEGVLAD_VOTE_UNIQUE_REF, in ``mode``
        as well); the ids of the merged lists are global rows, so the result is again the single index's."""
        mode = vote_mode(mode, votes_per_image, vote_unique_ref)
        if hasattr(self.be, "hint_query_groups"):   # an image's rows as one group of the exact refinement (same results)
            self.be.hint_query_groups(qseg_offsets)
        if self.world > 1 or vote_depth_only:
            # The reference searches 200 and keeps 50 (place_rec_main.py:56,78).  The global top-50 is contained in the union
            # of the per-shard top-50 lists, and an exact search returns the same first 50 rows whatever depth it is asked
            # for (ascending by (distance, id)): every shard searches -- and refines -- k_vote deep, not k_search, and only
            # those columns travel.  (k_search only matters to a single index, which mirrors the reference's call.)
            d2, idx = self.search(Q, k_vote)
        else:
            d2, idx = self.search(Q, k_search)
        sims, m = self.be.sims_from_d2(d2, idx, k_vote)
        pred, sc = self.be.vote(m, sims, np.asarray(qseg_offsets, dtype=np.int32), n_top=n_top, mode=mode,
                                img_of_seg=self.img_of_seg_global, want_scores=want_scores)
        return pred, sc, m, sims


def _f32_key(u: np.ndarray) -> np.ndarray:
    """fp32 bits -> the order-preserving unsigned key of the device min / max reduction (select_kernels.hip)."""
    u = np.asarray(u, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _key_f32(k: int) -> float:
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


class QueryShardedRetrieval:
    """Query-sharded retrieval over a REPLICATED index (SURVEY 8e's second form), one process per GPU.

    * every rank adds the whole reference matrix (no row exchange); the query images are split into contiguous blocks,
      ``shard_images(n_query_images, world)``, so an image's segments never straddle ranks (a rank may hold none);
    * every rank searches, keeps k_vote and votes on its own images only.  The vote normalises by the GLOBAL min / max of
      all kept similarities (func_vpr.py:211-214), and that changes the ORDER of the predictions, not only the scale, so the
      ranks exchange one 16-byte record {min bits, max bits, status, query segments} before the vote -- min / max are exact:
      the same bits as one process over all similarities;
    * the predictions (and fp64 scores) are gathered in global image order, padded to equal slices: the same on every rank.

    Two transports, as ShardedSegmentIndex: a torch.distributed group (gloo / nccl), or ``native_comm=True`` -- the context's
    own RCCL communicator (segvlad_vote_global + segvlad_allgather_rows), the id travelling over torch.distributed's host
    channel.  The compute is delegated to a backend with the SegVLADEngine interface (db_reset, db_add, search, sims_from_d2,
    minmax, vote; vote_global / allgather_rows / comm_* for native_comm).  Excluding image-id windows per query image
    (engine.search_excluding) is a single-index feature for now: this class has no ``exclude`` option."""

    def __init__(self, backend, rank: Optional[int] = None, world: Optional[int] = None, group=None,
                 device: Optional[torch.device] = None, native_comm: bool = False):
        self.be = backend
        self.native = bool(native_comm)
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = rank if rank is not None else (dist.get_rank(group) if self.distributed else 0)
        self.world = world if world is not None else (dist.get_world_size(group) if self.distributed else 1)
        self.device = device if device is not None else getattr(backend, "device", torch.device("cpu"))
        self.img_of_seg: Optional[torch.Tensor] = None
        self.img_bounds: Optional[np.ndarray] = None

    @staticmethod
    def collective_bytes(world: int, n_img: int, n_top: int) -> dict:
        """Bytes every rank SENDS / RECEIVES per retrieve(): the 16-byte extrema record, and the prediction rows -- one row of
        3 * n_top 32-bit words {pred, fp64 score bits} per image of the largest slice (equal slices).  (The row-sharded form
        moves the query descriptors and nq * k * 12 B of top-k records instead.)"""
        rows = (n_img + world - 1) // world if world else 0
        row_b = 3 * n_top * 4
        return {"extrema_allgather_send": 16, "extrema_allgather_recv": world * 16,
                "pred_allgather_send": rows * row_b, "pred_allgather_recv": world * rows * row_b}

    # ---- build --------------------------------------------------------------------------------------
    def build(self, all_rows, img_of_seg):
        """Every rank adds the WHOLE reference matrix [n, d] and keeps the segment -> image map [n] (no exchange)."""
        self.be.db_reset()
        img = torch.as_tensor(np.asarray(img_of_seg) if not isinstance(img_of_seg, torch.Tensor) else img_of_seg)
        self.img_of_seg = img.to(torch.int32).to(self.device).contiguous()
        if int(all_rows.shape[0]):
            self.be.db_add(all_rows, None)
        if self.native and not (hasattr(self.be, "comm_info") and self.be.comm_info()["world"] == self.world):
            # (a communicator of this size that the caller bound to the context already is used as it is)
            uid = [self.be.comm_unique_id() if self.rank == 0 else None]
            if self.world > 1:
                dist.broadcast_object_list(uid, src=0, group=self.group)
            self.be.comm_init(uid[0], self.rank, self.world)

    def remove(self, row_ids=None, img_ids=None) -> int:
        """Removes rows by row id and / or by reference image id from the replicated index (segvlad_db_remove: survivors keep
        their order, ids move down).  Every rank removes the same rows -- the engine holds no image map, so image ids become row
        ids through the Python-side map, which is compacted with them.  Returns the number of rows removed."""
        keep = removal_keep_mask(self.img_of_seg, row_ids, img_ids)
        gone = torch.nonzero(~keep).reshape(-1).to(torch.int64)
        if gone.numel():
            self.be.db_remove(row_ids=gone)
        self.img_of_seg = self.img_of_seg[keep].contiguous()
        return int(gone.numel())

    def split(self, n_query_images: int) -> np.ndarray:
        """The query split (contiguous image blocks): rank r describes and retrieves images [b[r], b[r + 1])."""
        self.img_bounds = shard_images(int(n_query_images), self.world)
        return self.img_bounds

    # ---- query --------------------------------------------------------------------------------------
    def retrieve(self, Q_local, qseg_offsets_local: Sequence[int], k_search: int = 200, k_vote: int = 50, n_top: int = 5,
                 mode: int = 0, want_scores: bool = False, vote_depth_only: bool = False, n_query_images: Optional[int] = None,
                 votes_per_image=None, vote_unique_ref=False) -> dict:
        """This rank's images: Q_local [nq_local, d] (their segment rows), qseg_offsets_local [n_img_local + 1] (from 0).
        Collective: every rank calls it, with the split of split(n_query_images) (or n_query_images given here).
        Returns {"pred", "score"}: the GATHERED [n_query_images, n_top] predictions / fp64 scores in global image order,
        identical on every rank (score None unless want_scores), and {"pred_local", "score_local", "m", "sims"}: this rank's.
        votes_per_image (1 .. 255): at most that many hits per reference image from each query segment, capped in the vote
        (in ``mode``, _lib.vote_mode); the global extrema stay those of all kept similarities.  vote_unique_ref: a reference
        segment votes once per query image (SEGVLAD_VOTE_UNIQUE_REF, in ``mode`` as well); an image's rows live on one rank."""
        mode = vote_mode(mode, votes_per_image, vote_unique_ref)
        if n_query_images is not None:
            self.split(n_query_images)
        if self.img_bounds is None:
            raise ValueError("QueryShardedRetrieval.retrieve: call split(n_query_images) first (or pass n_query_images)")
        off = np.asarray(qseg_offsets_local, dtype=np.int32)
        n_img = len(off) - 1
        per_rank = [int(self.img_bounds[r + 1] - self.img_bounds[r]) for r in range(self.world)]
        if n_img != per_rank[self.rank]:
            raise ValueError(f"rank {self.rank} holds {n_img} query images, the split gives it {per_rank[self.rank]}")
        nq = int(off[-1]) if n_img else 0
        local_err = None
        m = torch.empty((0, k_vote), dtype=torch.int64, device=self.device)
        sims = torch.empty((0, k_vote), dtype=torch.float32, device=self.device)
        try:
            if nq:
                if hasattr(self.be, "hint_query_groups"):
                    self.be.hint_query_groups(off)
                d2, idx = self.be.search(Q_local, k_vote if vote_depth_only else k_search)
                sims, m = (torch.as_tensor(t).to(self.device) for t in self.be.sims_from_d2(d2, idx, k_vote))
        except Exception as e:   # noqa: BLE001 -- reported on every rank after the exchange (nobody is left waiting)
            if self.world == 1 and not self.native:
                raise
            local_err = e
        if self.native:
            # the exchange and the vote in ONE collective C-ABI call; a failed local step still enters it (with no images)
            if local_err is not None:
                # n_top = 0 is refused by the local checks: this rank joins the exchange with a failed status, so every rank
                # raises and none goes on to the prediction gather without it
                try:
                    self.be.vote_global(m[:0], sims[:0], np.zeros(1, np.int32), n_top=0, mode=mode, img_of_seg=self.img_of_seg,
                                        want_scores=False)
                except Exception:   # noqa: BLE001
                    pass
                raise local_err
            pred, sc = self.be.vote_global(m, sims, off, n_top=n_top, mode=mode, img_of_seg=self.img_of_seg, want_scores=want_scores)
        else:
            smin, smax = self._global_extrema(sims, nq, local_err, mode)
            pred, sc = self._vote_local(m, sims, off, n_img, n_top, mode, want_scores, smin, smax)
        pred_all, sc_all = self.gather_predictions(pred, sc, per_rank, n_top, want_scores)
        return {"pred": pred_all, "score": sc_all, "pred_local": pred, "score_local": sc, "m": m, "sims": sims}

    def _global_extrema(self, sims, nq: int, local_err, mode: int):
        """torch.distributed transport: this rank's record -> all_gather -> the exact global (min, max) on the host."""
        rec = torch.tensor([0x7F800000, -0x00800000, 1 if local_err is not None else 0, 0], dtype=torch.int32, device=self.device)
        if local_err is None and nq and (mode & 0x7F) == 0:
            mm = torch.as_tensor(self.be.minmax(sims)).to(self.device).to(torch.float32).contiguous()
            rec = torch.cat([mm.view(torch.int32), torch.tensor([0, nq], dtype=torch.int32, device=self.device)])
        if self.world > 1:
            allrec = torch.empty((self.world, 4), dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(allrec.view(-1), rec, group=self.group)
        else:
            allrec = rec.view(1, 4)
        r = allrec.cpu().numpy().view(np.uint32)
        if local_err is not None:
            raise local_err
        bad = [i for i in range(self.world) if r[i, 2]]
        if bad:
            from ._lib import SEGVLAD_ERR_COMM, SegVLADError

            raise SegVLADError(f"query-sharded retrieve: rank {bad[0]} failed its local step (every rank raises)", code=SEGVLAD_ERR_COMM)
        has = r[:, 3] != 0
        if not has.any():
            return float("nan"), float("nan")
        return _key_f32(int(_f32_key(r[has, 0]).min())), _key_f32(int(_f32_key(r[has, 1]).max()))

    def _vote_local(self, m, sims, off, n_img, n_top, mode, want_scores, smin, smax):
        if n_img == 0:
            return (torch.empty((0, n_top), dtype=torch.int32, device=self.device),
                    torch.empty((0, n_top), dtype=torch.float64, device=self.device) if want_scores else None)
        pred, sc = self.be.vote(m, sims, off, n_top=n_top, mode=mode, img_of_seg=self.img_of_seg, smin=smin, smax=smax,
                                want_scores=want_scores)
        pred = torch.as_tensor(pred).to(self.device)
        if want_scores:
            sc = torch.as_tensor(np.asarray(sc, dtype=np.float64) if not isinstance(sc, torch.Tensor) else sc).to(self.device)
        return pred, sc

    def gather_predictions(self, pred, sc, per_rank: Sequence[int], n_top: int, want_scores: bool):
        """Every rank's [n_img_r, n_top] predictions (and fp64 scores) -> [sum n_img_r, n_top] in rank = image order.  One
        all-gather of int32 rows {pred [n_top], score bits [2 * n_top]}, padded to the largest slice (a byte-exact copy)."""
        n = int(pred.shape[0])
        mx = max(per_rank)
        rows = torch.zeros((mx, 3 * n_top), dtype=torch.int32, device=self.device)
        rows[:n, :n_top] = pred.to(torch.int32)
        if want_scores:
            rows[:n, n_top:] = sc.to(torch.float64).contiguous().view(torch.int32).view(n, 2 * n_top)
        if self.world == 1:
            allrows = rows
        elif self.native:
            allrows = self.be.allgather_rows(rows.view(torch.float32), world=self.world).view(torch.int32)
        else:
            allrows = torch.empty((self.world * mx, 3 * n_top), dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(allrows, rows, group=self.group)
        allrows = allrows.view(self.world, mx, 3 * n_top)
        take = torch.cat([allrows[r, :per_rank[r]] for r in range(self.world)])
        pred_all = take[:, :n_top].clone()
        sc_all = None
        if want_scores:   # (a fresh dense copy: a one-row slice keeps its odd offset and stride, which a fp64 view refuses)
            sc_all = torch.empty((take.shape[0], 2 * n_top), dtype=torch.int32, device=take.device)
            sc_all.copy_(take[:, n_top:])
            sc_all = sc_all.view(torch.float64)
        return pred_all, sc_all


def dry_run_collectives(backend, device, worlds: Sequence[int] = (2, 3, 4, 8), nq: int = 96, k: int = 50, d: int = 64, seed: int = 0) -> dict:
    """Everything of the multi-GPU exchange that can be checked WITHOUT the other ranks (VERDICT r05 next #5b): the first real
    N > 1 run must not be the first time these shapes exist.

    For every world size W in `worlds`: a planted index is cut into W image-aligned shards, every shard is searched on `backend`
    (one after the other, on this one device), each rank's operands of the two collectives are built exactly as the ranks would
    build them -- `pack_topk_records`, the (padded) query-row slices -- and CHECKED against what `all_gather_into_tensor` demands
    (dtype, contiguity, output numel == W x input numel); the collective itself is replaced by the concatenation in rank order
    that it is defined to produce; `unpack_topk_records` + `merge_topk` must then return the single index's (d2, ids) bit for bit.
    At W = 1 the real collectives run when a process group is initialised (the nccl = RCCL backend on a GPU box).
    Returns a report; raises AssertionError / ValueError on the first violation."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    n_img, S = 64, 23
    R = torch.nn.functional.normalize(torch.randn(n_img * S, d, generator=g), dim=1).to(device)
    Q = torch.nn.functional.normalize(R[torch.randint(0, n_img * S, (nq,), generator=g).to(device)] + 0.05 * torch.randn(nq, d, generator=g).to(device), dim=1)
    backend.db_reset()
    backend.db_add(R, None)
    d2_ref, idx_ref = (torch.as_tensor(t).to(device) for t in backend.search(Q, k))
    report = {"worlds": {}, "nq": nq, "k": k, "d": d, "rows": n_img * S}
    for W in worlds:
        ib = shard_images(n_img, W)
        recs, row_slices = [], []
        qb = shard_images(nq, W)                                      # the ranks' slices of the query rows (ragged unless W | nq)
        rows_per_rank = [int(qb[r + 1] - qb[r]) for r in range(W)]
        mx = max(rows_per_rank)
        for r in range(W):
            lo, hi = int(ib[r]) * S, int(ib[r + 1]) * S
            backend.db_reset()
            if hi > lo:
                backend.db_add(R[lo:hi].contiguous(), None)
                dd, ii = (torch.as_tensor(t).to(device) for t in backend.search(Q, k))
                ii = torch.where(ii >= 0, ii + lo, ii)
            else:
                dd = torch.full((nq, k), float("inf"), dtype=torch.float32, device=device)
                ii = torch.full((nq, k), -1, dtype=torch.int64, device=device)
            rec = ShardedSegmentIndex.pack_topk_records(dd, ii)
            assert rec.dtype == torch.int32 and rec.is_contiguous() and tuple(rec.shape) == (nq, k, 3), (W, r, rec.shape)
            recs.append(rec)
            x = Q[int(qb[r]):int(qb[r + 1])].contiguous()
            if x.shape[0] < mx:
                x = torch.cat([x, x.new_zeros((mx - x.shape[0], d))])
            assert x.is_contiguous() and x.dtype == torch.float32 and tuple(x.shape) == (mx, d)
            row_slices.append(x)
        allrec = torch.cat(recs)                                      # = all_gather_into_tensor's output: rank-major concatenation
        assert allrec.numel() == W * recs[0].numel() and allrec.is_contiguous()
        d2c, idc = ShardedSegmentIndex.unpack_topk_records(allrec, W)
        assert tuple(d2c.shape) == (nq, W * k) and d2c.dtype == torch.float32 and idc.dtype == torch.int64 and d2c.is_contiguous() and idc.is_contiguous()
        md, mi = (torch.as_tensor(t).to(device) for t in backend.merge_topk(d2c, idc, W, k))
        assert torch.equal(mi, idx_ref) and torch.equal(md, d2_ref), f"world {W}: the merged shards differ from the single index"
        gathered = torch.cat([p[:n] for p, n in zip(row_slices, rows_per_rank)])
        assert torch.equal(gathered, Q), f"world {W}: the padded row gather does not reproduce the query rows"
        report["worlds"][str(W)] = {"ok": True, "rows_per_rank": rows_per_rank,
                                    "bytes": ShardedSegmentIndex.collective_bytes(W, nq, k, d, rows_per_rank)}
    backend.db_reset()
    # world 1 through the REAL collectives (whatever backend the process group has: nccl on the GPU box)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() == 1:
        index = ShardedSegmentIndex(backend, rank=0, world=1, device=device)
        index.build(R, torch.arange(n_img, dtype=torch.int32).repeat_interleave(S))
        d2c, idc = index.exchange_topk(d2_ref, idx_ref)
        assert torch.equal(d2c, d2_ref) and torch.equal(idc, idx_ref)
        out = torch.empty_like(Q)
        dist.all_gather_into_tensor(out, Q.contiguous())
        assert torch.equal(out, Q)
        t = torch.tensor([1.0], device=device)
        dist.all_reduce(t)
        report["world_1_process_group"] = {"backend": dist.get_backend(), "ok": True}
        backend.db_reset()
    return report
