"""Batched SegVLAD pipeline on one GPU: the reference's per-image driver loop
(place_rec_main.py:244-276 / 309-341: masks -> imInds -> adjacency -> seg-VLAD -> [PCA per batch] -> concat)
restated as batch calls over device-resident inputs, followed by the ``recall_segloc`` chain
(place_rec_main.py:44-96).  Host work is limited to what the reference also does on the host
(Qhull Delaunay via scipy) plus launch bookkeeping."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import SEGVLAD_ERR_LIMIT, SegVLADDegenerateError, SegVLADError
from .engine import SegVLADEngine
from .func_vpr import adjacency_from_centroids
from .rle import RleMasks

_POOL: Optional[ThreadPoolExecutor] = None


def _pool(workers: int) -> ThreadPoolExecutor:
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=workers)
    return _POOL


def adjacency_batch(centroids: np.ndarray, seg_offsets: Sequence[int], order: int, workers: int = 8) -> np.ndarray:
    """Concatenated per-image [S_b,S_b] uint8 adjacency blocks from the centroids [S_tot,2]
    (func_vpr.py:1315-1345 per image; Qhull releases the GIL, so images run on a thread pool)."""
    B = len(seg_offsets) - 1

    def one(b):
        c = centroids[seg_offsets[b]:seg_offsets[b + 1]]
        return adjacency_from_centroids(c, order).numpy().astype(np.uint8).reshape(-1)

    if B == 0:
        return np.zeros(0, np.uint8)
    parts = list(_pool(workers).map(one, range(B))) if B > 1 else [one(0)]
    return np.concatenate(parts)


class SegVLADPipeline:
    def __init__(self, engine: SegVLADEngine, H: int, W: int, patch: int = 14, order: int = 3, use_pca: bool = True,
                 adj_workers: int = 8, host_adjacency: bool = False, fuse_pca: bool = True, check_empty: bool = True,
                 vlad_mode: str = None, soft_temp: float = None, vlad_burst=None, vlad_burst_scope: str = None):
        self.eng = engine
        # vlad_burst_scope 'image' | 'segment': the engine's option vlad_burst_scope; None leaves the engine as it is
        if vlad_burst_scope is not None:
            engine.set_vlad_burst_scope(vlad_burst_scope)
        # vlad_burst (a, b, p): the engine's option vlad_burst, set here like vlad_mode; None leaves the engine as it is
        if vlad_burst is not None:
            engine.set_vlad_burst(tuple(vlad_burst))
        # vlad_mode 'hard' | 'soft' | 'soft_pooled' (+ soft_temp): the engine's option vlad_assign, set here for every describe of
        # this context (soft_pooled is the reference's VLAD(vlad_mode='soft', soft_temp=...)); None leaves the engine as it is
        if vlad_mode is not None:
            engine.set_vlad_assign(vlad_mode, soft_temp if vlad_mode != "hard" else None)
        elif soft_temp is not None:
            raise ValueError("SegVLADPipeline: soft_temp needs vlad_mode='soft'")
        self.H, self.W, self.patch = H, W, patch
        self.order = order
        self.use_pca = use_pca
        self.adj_workers = adj_workers
        self.host_adjacency = host_adjacency
        self.fuse_pca = fuse_pca
        # an empty mask has no centroid: the reference fails there (func_vpr.py:1314 -> Delaunay on NaN); with
        # check_empty the device adjacency reports it (one 4-byte read-back per batch) and describe() raises ValueError
        self.check_empty = check_empty
        self.N = (H // patch) * (W // patch)
        self._index_xy = None                # fp64 [rows][2] on the device: the index rows' centroids (index_add(..., xy=...))
        self._index_rows_without_xy = False  # rows were added without them since the last index_reset
        self._eager_flags = 0   # > 0: read the adjacency flags BEFORE describing (set after a batch that needed a Qhull patch)

    # ---- a2..a9: images -> (normalised) segment descriptors ------------------------------------------
    def describe(self, tokens: torch.Tensor, masks: torch.Tensor, seg_offsets: np.ndarray, adj=None,
                 l2norm: bool = True) -> torch.Tensor:
        """tokens [B,D,N] fp32 (device), masks [S_tot,Hm,Wm] uint8 (device) or an ``RleMasks`` batch of S_tot run-length masks
        (SAM's uncompressed RLE; same results, the masks are never inflated), seg_offsets [B+1] (host).
        adj: precomputed concatenated adjacency (uint8) or None to derive it (order>0) from the masks.
        Returns [S_tot, P] (PCA'd, row-normalised when l2norm) or [S_tot, K*D]."""
        eng = self.eng
        lazy = None   # (device flags, centroids) of a device adjacency whose per-image flags have not been looked at yet
        rle = masks if isinstance(masks, RleMasks) else None   # run-length masks: the separate entry points below, never inflated
        if (rle is None and self.order and adj is None and not self.host_adjacency and hasattr(eng, "describe_begin")
                and isinstance(tokens, torch.Tensor) and tokens.is_cuda and isinstance(masks, torch.Tensor) and masks.is_cuda
                and (self.fuse_pca or not self.use_pca)):
            # THREE calls (segvlad_describe_begin / _flags / _end): the mask branch (incidence + centroids -> adjacency) runs on the
            # context's side stream beside the assignment pass; its per-image flags and centroids reach the host while that pass
            # keeps the device busy, so an empty mask is reported, and the images with a non-generic centroid configuration get
            # Qhull's adjacency (the reference's own library, ~0.2 ms of host work per image), WITHOUT an idle device -- rounds 3-4
            # read the flags between two launches (a synchronisation in the middle of the stage) or described the batch twice.
            try:
                h = eng.describe_begin(masks, tokens, seg_offsets, self.H, self.W, self.patch, self.order, pca=self.use_pca)
            except SegVLADError as e:
                # SEGVLAD_ERR_LIMIT = "the split call cannot, the separate entry points can": more segments in an image than the
                # in-LDS Delaunay holds, an empty batch, a PCA model without the fp16x3 form (pca_arith=fp32 / K*D % 32 != 0:
                # images_pca then projects the stored descriptor with the plain GEMM) -> the paths below
                if e.code != SEGVLAD_ERR_LIMIT:
                    raise
                h = None
            if h is not None:
                imgs, blocks = None, None
                if self.check_empty:
                    flags, cent = eng.describe_flags(h)
                    if (flags & 1).any():
                        eng.describe_cancel(h)
                        raise ValueError(f"{int((flags & 1).sum())} image(s) with an empty mask: centroid undefined")
                    imgs = np.nonzero(flags & 2)[0]
                    self.n_flag_checks = getattr(self, "n_flag_checks", 0) + 1
                    self.n_flagged_images = getattr(self, "n_flagged_images", 0) + int(len(imgs))
                    so = np.asarray(seg_offsets)
                    try:
                        blocks = [adjacency_from_centroids(cent[so[b]:so[b + 1]], self.order).numpy().astype(np.uint8) for b in imgs]
                    except Exception:
                        eng.describe_cancel(h)
                        raise
                return eng.describe_end(h, imgs, blocks, l2norm=l2norm)["out"]
        if self.order and adj is None:
            bits, cent = self._incidence(masks, rle, True)   # one pass over the mask bytes (or over the runs)
            if self.host_adjacency:   # scipy/Qhull on the host, exactly the reference's library (slow: ~0.4 ms/image)
                adj = adjacency_batch(cent.cpu().numpy(), seg_offsets, self.order, self.adj_workers)
            else:                     # device kernel: no host round trip (check_empty: one flag byte per image comes back)
                try:
                    if self.check_empty and hasattr(eng, "adjacency_flagged"):
                        # The flags are READ after the kernels that consume the adjacency have been enqueued (below): reading
                        # them here is a host synchronisation in the middle of the describe stage, with an idle device behind
                        # it.  A flagged image is patched afterwards and the batch described AGAIN -- twice the work, so a
                        # batch that needed it switches the next 16 batches back to reading the flags first (data whose
                        # centroids are non-generic again and again: axis-aligned synthetic masks; real SAM masks are not).
                        adj, flags_dev = eng.adjacency_flagged(cent, seg_offsets, self.order, device_flags=True)
                        if self._eager_flags > 0:
                            self._eager_flags -= 1
                            adj = self._check_flags(flags_dev, adj, cent, seg_offsets)
                        else:
                            lazy = (flags_dev, cent)
                    else:
                        adj = eng.adjacency(cent, seg_offsets, self.order, check_empty=self.check_empty)
                except SegVLADError as e:
                    # typed, not message-matched: a documented implementation limit (SEGVLAD_ERR_LIMIT) or the
                    # degenerate-configuration report are recoverable; anything else is not
                    if not isinstance(e, SegVLADDegenerateError) and e.code != SEGVLAD_ERR_LIMIT:
                        raise
                    # an image with more segments (> 639) than the in-LDS Delaunay holds (or a report from an engine
                    # without per-image flags): the reference's own Qhull path for this batch
                    adj = adjacency_batch(cent.cpu().numpy(), seg_offsets, self.order, self.adj_workers)
        else:
            bits = self._incidence(masks, rle, False)[0]
            if not self.order:
                adj = None
        out = self._describe_with(tokens, bits, seg_offsets, adj, l2norm)
        if lazy is not None:
            patched = self._check_flags(lazy[0], adj, lazy[1], seg_offsets)
            if patched is not adj:
                self._eager_flags = 16
                out = self._describe_with(tokens, bits, seg_offsets, patched, l2norm)
        return out

    def _incidence(self, masks, rle, want_centroids):
        """(incidence bit rows, centroids or None) of dense masks or of a run-length batch.  Masks whose bitmap the run-length
        kernel cannot hold (SEGVLAD_ERR_LIMIT) are inflated on the device and take the dense entry: the same bytes."""
        eng = self.eng
        if rle is not None:
            try:
                return eng.incidence_rle(rle, self.H, self.W, self.patch, centroids=want_centroids)
            except SegVLADError as e:
                if e.code != SEGVLAD_ERR_LIMIT:
                    raise
                masks = eng.rle_decode(rle)
        if want_centroids:
            return eng.incidence_centroids(masks, self.H, self.W, self.patch)
        return eng.incidence(masks, self.H, self.W, self.patch), None

    def _check_flags(self, flags_dev, adj, cent, seg_offsets):
        """Reads the per-image flags of a device adjacency (a host synchronisation): raises on an empty mask; images with a
        non-generic centroid configuration (duplicate / co-circular centroids: the triangulation is Qhull's tie-breaking) get
        the reference's own Qhull path.  Returns ``adj`` itself when nothing was flagged, else the patched adjacency."""
        flags = flags_dev.cpu().numpy()
        if (flags & 1).any():
            raise ValueError(f"{int((flags & 1).sum())} image(s) with an empty mask: centroid undefined")
        bad = np.nonzero(flags & 2)[0]
        self.n_flag_checks = getattr(self, "n_flag_checks", 0) + 1
        self.n_flagged_images = getattr(self, "n_flagged_images", 0) + int(len(bad))
        if len(bad):
            return self._patch_with_qhull(adj.clone(), cent, np.asarray(seg_offsets), bad)
        return adj

    def _describe_with(self, tokens, bits, seg_offsets, adj, l2norm):
        eng = self.eng
        if self.use_pca and self.fuse_pca:   # aggregation feeds the projection GEMM directly (segvlad_images_pca)
            return eng.seg_vlad_pca(tokens, bits, seg_offsets, adj, l2norm=l2norm)["out"]
        desc = eng.seg_vlad(tokens, bits, seg_offsets, adj)["out"]
        if self.use_pca:
            desc = eng.pca_apply(desc, l2norm=l2norm)
        return desc

    def _patch_with_qhull(self, adj: torch.Tensor, cent: torch.Tensor, so: np.ndarray, images) -> torch.Tensor:
        """Overwrite the [S_b, S_b] blocks of the listed images in the concatenated device adjacency with Qhull's."""
        sizes = (so[1:] - so[:-1]).astype(np.int64)
        adj_off = np.concatenate([[0], np.cumsum(sizes * sizes)])
        lo, hi = int(so[min(images)]), int(so[max(images) + 1])
        ch = cent[lo:hi].cpu().numpy()
        for b in images:
            blk = adjacency_from_centroids(ch[so[b] - lo:so[b + 1] - lo], self.order).numpy().astype(np.uint8).reshape(-1)
            adj[int(adj_off[b]):int(adj_off[b + 1])] = torch.from_numpy(blk).to(adj.device)
        return adj

    # ---- a10: index ------------------------------------------------------------------------------------
    def index_reset(self):
        self.eng.db_reset()
        self._index_xy = None
        self._index_rows_without_xy = False

    def index_add(self, desc: torch.Tensor, img_of_seg, xy=None):
        """Adds rows to the index.  ``xy`` (optional, fp64 [rows][2]): the rows' segment centroids (x, y), kept in a device tensor
        beside the index -- row id for row id -- for verify()."""
        n = int(desc.shape[0])
        if xy is not None:
            xy = torch.as_tensor(xy, dtype=torch.float64, device=self.eng.device)
            if tuple(xy.shape) != (n, 2):
                raise ValueError(f"xy must be [rows={n}][2], got shape {tuple(xy.shape)}")
        self.eng.db_add(desc, img_of_seg)
        if n == 0:
            return
        if xy is None or self._index_rows_without_xy:
            self._index_rows_without_xy = True   # (until index_reset: the table would no longer be one row per row id)
            self._index_xy = None
            return
        self._index_xy = xy.clone() if self._index_xy is None else torch.cat([self._index_xy, xy])

    def index_remove_images(self, img_ids) -> int:
        """Drops every segment row of the listed reference images (stale, mis-registered or withdrawn) from the index on the
        device; later rows move down (engine.db_remove), and so do their centroids when index_add received them.  Returns the
        number of rows removed."""
        xy = self._index_xy
        if xy is None:
            return self.eng.db_remove(img_ids=img_ids)
        removed, new_id = self.eng.db_remove(img_ids=img_ids, want_new_ids=True)
        self._index_xy = xy[new_id >= 0].contiguous()   # (the survivors keep their order)
        return removed

    # ---- a10..a12: descriptors -> ranked reference images ----------------------------------------------
    def retrieve(self, qdesc: torch.Tensor, qseg_offsets: np.ndarray, k_search: int = 200, k_vote: int = 50, n_top: int = 5,
                 mode: int = _lib.VOTE_WT_BORDA_IM, want_scores: bool = False, vote_depth_only: bool = False, shortlist=None,
                 exclude=None, per_image=None, votes_per_image=None, vote_unique_ref=False):
        """search k_search (place_rec_main.py:56) -> keep k_vote and 2-d^2 (:78-81) -> vote (:84).  vote_depth_only: search
        only as deep as the vote reads (the 200-wide lists are only pickled under save_results, :61-75): the same k_vote columns
        -- an exact search's first columns do not depend on its depth -- for a quarter of the refinement.
        shortlist: per query image the reference image ids its segments may match (engine.search_shortlist: an
        ``int32 [n_img][M]`` array, -1 padded, or a ragged list of lists): the search runs over those images' rows only, and
        the vote's global extrema (func_vpr.py:212-213) are taken over the filled slots -- a (+inf, -1) pad is a -inf
        similarity, which the vote skips and which must not become the minimum.
        exclude: per query image the intervals of reference image ids its segments must NOT match (engine.search_excluding:
        ``int32 [n_img][E][2]`` or a ragged list; engine.window_intervals for a map queried with its own frames); the extrema
        as for a shortlist.  Not together with ``shortlist`` (ValueError).
        per_image: the search step is engine.search_grouped at the same depth: every query segment's list holds at most
        ``per_image`` rows of one reference image (1: one segment, one vote per image; the predictions are then distinct
        candidates for rerank()).  A list may end in (+inf, -1) pads: the extrema as for a shortlist.  Not together with
        ``shortlist`` or ``exclude`` (ValueError).
        votes_per_image (1 .. 255): the cap is applied in the VOTE instead (engine.vote's ``per_image``): of every query
        segment's k_vote entries at most that many count for one reference image, the others are skipped and nothing moves up
        behind them.  No second search, and it combines with ``shortlist``, ``exclude`` and ``per_image``; the extrema passed
        for the derived searches stay those of the filled slots.
        vote_unique_ref: a reference segment votes once per query image (engine.vote's ``unique_ref``): of the entries of one
        query image that name the same index row only the most similar one counts.  In front of ``votes_per_image``; combines
        with everything above."""
        mode = _lib.vote_mode(mode, votes_per_image, vote_unique_ref)
        if shortlist is not None and exclude is not None:
            raise ValueError("retrieve: give shortlist or exclude, not both")
        if per_image is not None and (shortlist is not None or exclude is not None):
            raise ValueError("retrieve: per_image does not combine with shortlist or exclude")
        depth = k_vote if vote_depth_only else k_search
        if per_image is not None:
            self.eng.hint_query_groups(qseg_offsets)
            d2, idx = self.eng.search_grouped(qdesc, depth, per_image)
        elif exclude is not None:
            self.eng.hint_query_groups(qseg_offsets)
            d2, idx = self.eng.search_excluding(qdesc, qseg_offsets, exclude, depth)
        elif shortlist is None:
            self.eng.hint_query_groups(qseg_offsets)
            d2, idx = self.eng.search(qdesc, depth)
        else:
            d2, idx = self.eng.search_shortlist(qdesc, qseg_offsets, shortlist, depth)
        self.last_search = (d2, idx)   # the full-depth lists: what `save_results` pickles (place_rec_main.py:61-75)
        sims, m = self.eng.sims_from_d2(d2, idx, k_vote)
        smin = smax = float("nan")
        if (shortlist is not None or exclude is not None or per_image is not None) and (mode & 0x7F) == _lib.VOTE_WT_BORDA_IM:
            kept = sims[m >= 0]
            if kept.numel():
                smin, smax = float(kept.min()), float(kept.max())
        pred, sc = self.eng.vote(m, sims, qseg_offsets, n_top=n_top, mode=mode, want_scores=want_scores, smin=smin, smax=smax)
        return pred, sc, m, sims

    # ---- behind the vote: candidate images re-ranked by one-to-one segment matching ------------------------------------------
    def rerank(self, qdesc: torch.Tensor, qseg_offsets: np.ndarray, pred, max_d2: float = float("inf")):
        """Re-ranks every query image's candidate reference images -- ``pred`` [n_img][C]: retrieve()'s predictions, -1 padded
        -- by the mutual nearest segments between the query image and each candidate (engine.match_pairs; the use case of
        get_matches_for_single_image_pair, func_vpr.py:247-270): more mutual pairs first, then the larger summed similarity,
        then the vote's own order; candidates without rows last.  Returns ``(pred_reranked, n_mutual, score)``, each
        [n_img][C] in the NEW order: ``pred_reranked[b] = pred[b][order[b]]``."""
        cand = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)   # (the call takes its candidates on the host)
        out = self.eng.match_pairs(qdesc, qseg_offsets, cand, max_d2=max_d2)
        order = out["order"].to(torch.int64)
        if not (isinstance(pred, torch.Tensor) and pred.device == order.device):
            pred = torch.as_tensor(np.ascontiguousarray(cand), device=order.device)
        return torch.gather(pred, 1, order), torch.gather(out["n_mutual"], 1, order), torch.gather(out["score"], 1, order)

    # ---- behind the re-ranking: do the matched segments lie the same way in both images? ------------------------------------
    def verify(self, qdesc: torch.Tensor, qseg_offsets: np.ndarray, pred, q_xy, tol: float, max_d2: float = float("inf"),
               min_scale: float = 0.5, max_scale: float = 2.0):
        """Spatial verification of every query image's candidate reference images -- ``pred`` [n_img][C] as for rerank() --:
        the mutual nearest segments of each candidate (engine.match_pairs), then the largest set of them whose centroids one
        2-D similarity transform maps onto each other within ``tol`` (engine.verify_pairs; ``q_xy`` fp64 [nq][2]: the query
        rows' centroids, the index rows' are those given to index_add).  The candidates are ordered by (inliers desc, then
        rerank()'s order: mutual pairs, summed similarity, the vote).  Returns ``(pred_verified, n_inlier, n_mutual)``, each
        [n_img][C] in the NEW order.  ValueError when rows were added to the index without ``xy``."""
        if self._index_rows_without_xy:
            raise ValueError("verify: rows were added to the index without their centroids (index_add(..., xy=...))")
        r_xy = self._index_xy
        if r_xy is None:
            r_xy = torch.zeros((0, 2), dtype=torch.float64, device=self.eng.device)
        cand = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
        mp = self.eng.match_pairs(qdesc, qseg_offsets, cand, max_d2=max_d2, want_rows=True)
        o1 = mp["order"].to(torch.int64)                       # [n_img][C]: rerank()'s order of the slots
        per_img = torch.as_tensor(np.diff(np.asarray(qseg_offsets, dtype=np.int64)), device=o1.device)
        row_o1 = torch.repeat_interleave(o1, per_img, dim=0, output_size=int(mp["mutual"].shape[0]))  # [nq][C]: every query row's slot columns in that order
        vp = self.eng.verify_pairs(q_xy, r_xy, qseg_offsets, torch.gather(mp["fwd_idx"], 1, row_o1).contiguous(),
                                   torch.gather(mp["mutual"], 1, row_o1).contiguous(), tol, min_scale=min_scale, max_scale=max_scale)
        order = torch.gather(o1, 1, vp["order"].to(torch.int64))   # slots of `pred`, best verified first
        if not (isinstance(pred, torch.Tensor) and pred.device == order.device):
            pred = torch.as_tensor(np.ascontiguousarray(cand), device=order.device)
        self.last_verify = {"match": mp, "verify": vp, "order": order}
        return torch.gather(pred, 1, order), torch.gather(vp["n_inlier"], 1, vp["order"].to(torch.int64)), torch.gather(mp["n_mutual"], 1, order)

    # ---- behind any of them: candidates believed when the frames around them agree on one line through the map ---------------
    def sequence(self, pred, score, seq_offsets=None, back: int = 5, fwd: int = 5, velocities=None, tol: int = 1):
        """Temporal re-ranking of a traversal's candidates (engine.sequence_rerank): ``pred`` [T][C] holds the candidate
        reference images of T query frames in time order, image ids being frame numbers along the map, and ``score`` [T][C]
        one evidence value >= 0 per slot, in ``pred``'s slot order.  Accepted scores: retrieve()'s ``sc``
        (``want_scores=True``; with ``pred`` as returned), rerank()'s ``n_mutual`` or ``score`` and verify()'s ``n_inlier``
        or ``n_mutual`` (with the re-ranked / verified predictions those calls return, which are in the same order); integer
        counts are converted to fp64.  A slot with ``pred < 0`` or a non-finite score is empty.  ``seq_offsets`` [n_seq + 1]
        splits the frames into sequences (None: one).  Returns ``(pred_seq, seq_score, n_hit)``, each [T][C] in the NEW
        order: ``pred_seq[t] = pred[t][order[t]]``, best supported first, empty slots last."""
        out = self.eng.sequence_rerank(pred, score, seq_offsets=seq_offsets, back=back, fwd=fwd, velocities=velocities, tol=tol)
        order = out["order"].to(torch.int64)
        if not (isinstance(pred, torch.Tensor) and pred.device == order.device):
            pred = torch.as_tensor(np.ascontiguousarray(pred.cpu().numpy() if isinstance(pred, torch.Tensor) else pred), device=order.device)
        self.last_sequence = out
        return torch.gather(pred, 1, order), torch.gather(out["seq_score"], 1, order), torch.gather(out["n_hit"], 1, order)


def recall_at(preds: np.ndarray, gt: List[Sequence[int]], n: int) -> List[float]:
    """calc_recall (func_vpr.py:396-422) without the print: first correct rank, queries with empty GT skipped."""
    rec = np.zeros(n)
    num = 0
    for i, g in enumerate(gt):
        if len(g) == 0:
            continue
        num += 1
        for j in range(min(n, preds.shape[1])):
            if preds[i, j] in g:
                rec[j] += 1
                break
    return (np.cumsum(rec) / max(num, 1)).tolist()
