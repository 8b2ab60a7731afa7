/*
 * segvlad.h -- C-ABI of the MI355X-native SegVLAD hot path (libsegvlad_hip.so, gfx950).
 *
 * The reference (AnyLoc/Revisit-Anything, all Python) exposes no FFI; the boundary it offers is
 * the function surface of func_vpr.py / place_rec_main.py.  Each of the 58 entry points below replaces the
 * cited reference function(s); the Python module revisit_anything_amd.func_vpr maps the reference's
 * names/arguments onto these calls (INTEGRATION.md shows the ctypes stub a maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  Bulk data pointers may be DEVICE or HOST pointers
 *     (hipPointerGetAttributes decides; host data is staged through a context-owned buffer).
 *     Pointers documented "host" must be host memory (small launch-geometry metadata).
 *   - every function returns 0 (SEGVLAD_OK) or a negative error code; the message is available from
 *     segvlad_last_error(ctx).  No exception crosses the ABI.
 *   - one context per (device, stream).  A context is not re-entrant; distinct contexts may be
 *     driven from distinct host threads.  Work is enqueued on the context's HIP stream
 *     (segvlad_set_stream) and is asynchronous unless an output pointer is host memory.
 *   - results are freshly written into caller-owned buffers; inputs are never modified.
 *   - arithmetic: fp32 on device (the reference's fp64 aggregation is matched to <=1e-6 cosine);
 *     integer/bit outputs (incidence, labels away from audited ties, kNN ids away from ties,
 *     vote order) are exact.
 */
#ifndef SEGVLAD_H
#define SEGVLAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct segvlad_ctx segvlad_ctx;

enum {
  SEGVLAD_OK = 0,
  SEGVLAD_ERR_ARG = -1,    /* bad argument (null pointer, negative size, unsupported shape)   */
  SEGVLAD_ERR_HIP = -2,    /* a HIP runtime call failed                                        */
  SEGVLAD_ERR_STATE = -3,  /* call order (e.g. segvlad_images before segvlad_set_vocab)        */
  SEGVLAD_ERR_LIMIT = -4,  /* documented implementation limit exceeded                        */
  SEGVLAD_ERR_NOMEM = -5,
  SEGVLAD_ERR_COMM = -6    /* RCCL: library not found, or a collective / communicator call failed */
};

#define SEGVLAD_VOTE_WT_BORDA_IM 0 /* get_matches(method="max_seg_topk_wt_borda_Im"), func_vpr.py:207-224 */
#define SEGVLAD_VOTE_COUNT 1       /* get_matches(method="max_seg_topk"),            func_vpr.py:118-125 */

/* ---- lifetime ------------------------------------------------------------------------------ */
int segvlad_version(void);
int segvlad_create(segvlad_ctx** out, int device_id);
int segvlad_destroy(segvlad_ctx* ctx);
const char* segvlad_last_error(const segvlad_ctx* ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream.  The context's scratch and
 * barrier words assume its work is stream-ordered: before switching to another stream, order the old stream's work before the
 * new stream's -- synchronise the old stream, or make the new one wait on an event recorded on the old one behind the context's
 * last call (hipStreamWaitEvent; torch's wait_stream).  Inputs follow the same order: a call reads its device inputs in the
 * order of the context's stream (work the library runs on streams of its own is joined to it by events), and has taken what it
 * needs of its HOST inputs when it returns -- the caller may overwrite a device input behind the call on that stream, and a host
 * input at once (segvlad_describe_begin .. _end keep some buffers longer: see there).  tests/test_gpu_async_order.py holds every
 * entry to this. */
int segvlad_set_stream(segvlad_ctx* ctx, void* hip_stream);
int segvlad_synchronize(segvlad_ctx* ctx);

/* ---- vocabulary: torch.load(c_centers.pt) + F.normalize(c_centers)   place_rec_main.py:149-154,
 *      func_vpr.py:1145.  C is [K][D] fp32; both C and its row-normalised copy stay on device.   */
int segvlad_set_vocab(segvlad_ctx* ctx, const float* C, int K, int D);

/* ---- mask -> token incidence: nearest-upsample + argwhere + scatter  func_vpr.py:1088-1092 with
 *      the pixel->token map of place_rec_main.py:187-194 folded in.
 *      masks [S][Hm][Wm] bytes (non-zero = true); inc_bits [S][ceil(N/64)] u64, bit (t%64) of word
 *      (t/64) = token t covered; N = (H/patch)*(W/patch).  S may span a whole batch of images.   */
int segvlad_incidence(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch,
                      uint64_t* inc_bits);

/*      Fused variant: one pass over the mask bytes yields the incidence rows AND the centroids of
 *      func_vpr.py:1314 (see segvlad_mask_centroids) -- what the batched pipeline calls.            */
int segvlad_incidence_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch,
                                uint64_t* inc_bits, double* centroids);

/* ---- mask centroids: np.nonzero(mask).mean(1)[::-1]                  func_vpr.py:1314
 *      centroids [S][2] fp64 (x, y); an empty mask yields NaN (the reference raises ValueError).  */
int segvlad_mask_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, double* centroids);

/* ---- run-length masks: SAM's uncompressed RLE, mask_to_rle_pytorch / rle_to_mask        sam/segment_anything/utils/amg.py:107-149
 *      A batch of S masks of one size Hm x Wm:  counts [n_runs] uint32, the runs of all masks one after the other;
 *      run_offsets [S+1] int64, mask s owns counts[run_offsets[s] .. run_offsets[s+1]).  A mask is column-major (pixel
 *      p = col * Hm + row) and its runs alternate zeros / ones, starting with zeros: the first count may be 0, and zero-length
 *      runs are tolerated anywhere.  Both arrays device or host (host run_offsets are checked: non-negative, non-decreasing;
 *      host counts under device run_offsets cost one synchronising read of run_offsets[S]).
 *      segvlad_incidence_rle writes exactly what segvlad_incidence_centroids writes for the decoded masks, byte for byte:
 *      inc_bits [S][ceil(N/64)] with zero pad bits and centroids [S][2] fp64 (x, y), NaN for an empty mask; centroids may be
 *      NULL.  No Wm % 16 or alignment condition.  The mask lives as a bitmap in LDS: Wm * ceil(Hm/32) * 4 bytes above
 *      150 KiB return SEGVLAD_ERR_LIMIT -- inflate such a batch with segvlad_rle_decode and call segvlad_incidence_centroids.
 *      A mask whose runs do not sum to exactly Hm * Wm (a mask without runs included) is MALFORMED: it is clipped at Hm * Wm,
 *      the pixels its runs do not reach are zero, and it adds 1 to *n_bad_out (DEVICE memory or NULL; the caller zeroes it: the
 *      call never reads it back, so it does not synchronise when the outputs are device memory).  The other masks of the batch
 *      are unaffected, and no count ever becomes a global address.  S == 0: OK, nothing is written.  SEGVLAD_ERR_STATE while a
 *      segvlad_describe_begin is open; SEGVLAD_ERR_ARG on bad geometry, null pointers or a host n_bad_out.                     */
int segvlad_incidence_rle(segvlad_ctx* ctx, const uint32_t* counts, const int64_t* run_offsets, int S, int Hm, int Wm, int H, int W,
                          int patch, uint64_t* inc_bits, double* centroids, uint32_t* n_bad_out);

/*      rle_to_mask for the batch (amg.py:107-149 again: the inverse of mask_to_rle_pytorch): masks_out [S][Hm][Wm] bytes 0 / 1,
 *      row-major, device or host.  Malformed masks and n_bad_out as above.  Any size: masks whose bitmap exceeds the LDS are
 *      decoded in windows of columns (up to 65535 windows per mask) -- the way in for callers of the one-call segvlad_describe
 *      and for masks above segvlad_incidence_rle's bound.                                                                  */
int segvlad_rle_decode(segvlad_ctx* ctx, const uint32_t* counts, const int64_t* run_offsets, int S, int Hm, int Wm, uint8_t* masks_out,
                       uint32_t* n_bad_out);

/*      mask_to_rle_pytorch for the batch (amg.py:107-135), with area_from_rle's areas: dense masks -> the layout above, on the device.
 *      masks [S][Hm][Wm] uint8, row-major, device or host; a NON-ZERO byte is a set pixel (as in segvlad_incidence); any alignment,
 *      any Wm.  The runs are exactly the reference's counts: the mask is read column-major (pixel p = col * Hm + row), the runs
 *      alternate zeros / ones and start with zeros; the first count is 0 exactly when pixel 0 is set and no other count is 0; a mask
 *      with n value changes has n + 1 runs, plus one more if pixel 0 is set; an all-zero mask is [P], an all-ones mask [0, P]
 *      (P = Hm * Wm).
 *      run_offsets_out [S + 1] int64, device or host, required: always written, always the true counts; run_offsets[0] = 0 and
 *      mask s owns counts[run_offsets[s] .. run_offsets[s + 1]).  n_runs_out (HOST, may be NULL) = run_offsets[S].
 *      counts_out holds `capacity` uint32 slots, device or host (may be NULL when capacity == 0: a count-only call).  When
 *      run_offsets[S] <= capacity it receives the runs.  When run_offsets[S] > capacity it is NOT WRITTEN AT ALL, the call still
 *      returns SEGVLAD_OK, and the caller allocates run_offsets[S] slots and calls again (the protocol of segvlad_range_search).
 *      Slots at and beyond run_offsets[S] are never written.
 *      area_out [S] int64, device or host, may be NULL: the set pixels of each mask = the sum of its odd-indexed runs
 *      (area_from_rle).
 *      Synchronisation: none when every output is device memory and n_runs_out is NULL -- the emitting kernel reads the total from
 *      device memory and leaves, every thread alike, when it exceeds `capacity`.  Otherwise once; a host counts_out is filled by
 *      a blocking copy behind that wait, and only when the total fits (the total is read first: a host array that is too small
 *      stays untouched).
 *      S == 0: OK; run_offsets_out[0] = 0 and *n_runs_out = 0 are written, nothing else.  SEGVLAD_ERR_ARG: S < 0, Hm <= 0, Wm <= 0,
 *      capacity < 0, a NULL run_offsets_out, a NULL masks with S > 0, a NULL counts_out with capacity > 0.  SEGVLAD_ERR_LIMIT:
 *      Hm * Wm > 2^32 - 1 (a run is a 32-bit count), decided before any pointer is looked at.  SEGVLAD_ERR_STATE while a
 *      segvlad_describe_begin is open.  No mask is held in LDS: no other size bound (segvlad_incidence_rle's 150 KiB does not
 *      apply).  Deterministic: two calls return the same bytes.  Stage timer "rle_encode".
 *      How: a unit is one (mask, column, block of 256 rows); pass 1 counts every unit's value changes, a scan per mask ranks them
 *      and carries the last change along the column-major order, pass 2 reads the bytes again and stores each change's distance
 *      to the one before it (csrc/rle_encode_kernels.hip).                                                                     */
int segvlad_rle_encode(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int64_t* run_offsets_out, uint32_t* counts_out,
                       int64_t capacity, int64_t* area_out, int64_t* n_runs_out);

/*      remove_small_regions for the batch, mode "holes" and then mode "islands" (amg.py:267-291): the cleaning step of
 *      SamAutomaticMaskGenerator.postprocess_small_regions (automatic_mask_generator.py:325-376; its scoring and second box NMS stay
 *      with the caller).  The reference labels every mask twice with OpenCV on the host; this labels the whole batch on the device.
 *      masks, masks_out [S][Hm][Wm] uint8, row-major, device or host, any alignment; a NON-ZERO byte is a set pixel and the bytes
 *      written are 0 / 1.  For every mask, in this order:
 *        1. holes: the 8-connected components of the COMPLEMENT are labelled; every component with fewer than min_area pixels
 *           becomes set -- the outer background too when it is that small (the reference does not treat it specially).  The pass
 *           CHANGED the mask iff such a component exists.
 *        2. islands, on the result of 1: the 8-connected components of the mask are labelled; if none has fewer than min_area
 *           pixels the mask is unchanged; otherwise exactly the components with area >= min_area are kept, or, when there are
 *           none of those, the single largest one -- and the pass CHANGED the mask in either case: a mask whose only island is
 *           small comes back identical and flagged changed, as from the reference, whose caller turns the flag into the NMS score.
 *      The comparison is strictly <.  A complement without pixels (1.) and a mask without pixels (2.) have no components and are
 *      unchanged.  Tie for "largest": the reference takes argmax over OpenCV's label order; here the tie goes to THE COMPONENT WHOSE
 *      FIRST PIXEL IN ROW-MAJOR ORDER COMES FIRST, which is scipy.ndimage.label's numbering.  OpenCV's numbering under such a tie
 *      has not been checked (a known possible divergence).
 *      changed_out [S] int32: bit 0 = the holes pass changed the mask, bit 1 = the islands pass did.  boxes_out [S][4] int32: the
 *      tight XYXY box of the result in inclusive pixel coordinates, [0, 0, 0, 0] for an empty result (batched_mask_to_box).
 *      area_out [S] int64: the set pixels of the result.  Each device or host; each may be NULL.
 *      masks_out == masks is allowed (in place); any other overlap of the two is SEGVLAD_ERR_ARG.
 *      S == 0: OK, nothing is written.  min_area <= 1 changes nothing: the masks are copied (as 0 / 1), boxes and areas are
 *      computed, the flags are 0.  SEGVLAD_ERR_ARG: S < 0, Hm <= 0, Wm <= 0, min_area < 0, a NULL masks or masks_out with S > 0.
 *      SEGVLAD_ERR_LIMIT: Hm * Wm > 2^31 - 1 (a label is a 32-bit pixel index), decided before any pointer is looked at.
 *      SEGVLAD_ERR_STATE while a segvlad_describe_begin is open.  No mask is held whole in LDS: no other size bound.  Scratch: 8
 *      bytes per pixel of the batch (callers with many masks call in pieces; SegVLADEngine.mask_regions does).
 *      Synchronisation: none when every pointer is device memory; otherwise once.  Deterministic: all sums are integers and all
 *      roots are minima, two calls write the same bytes.  Stage timer "mask_regions".
 *      How: per pass a label plane int32 [S][Hm * Wm] (a pixel index inside the mask; union-find, the root is the component's
 *      first pixel): a union-find per 32 x 32 tile in LDS, the tile edges (both diagonals at every corner) united with agent-scope
 *      atomicMin, labels flattened and sizes summed with one atomic per (tile, tile-local component), one packed 64-bit maximum of
 *      (area, ~root) per mask, one rewrite of the pixels (csrc/regions_kernels.hip).                                            */
int segvlad_mask_regions(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int min_area, uint8_t* masks_out,
                         int32_t* changed_out, int32_t* boxes_out, int64_t* area_out);

/* ---- neighbourhood adjacency for a batch: getNbrsDelaunay + nbrMasksAGGFastSingle
 *      func_vpr.py:1241-1245, 1315-1345.  centroids [S_tot][2] fp64 (x, y) from segvlad_mask_centroids,
 *      seg_offsets [B+1] int32 HOST, order >= 1.  adj_out: concatenated per-image [S_b][S_b] byte
 *      matrices = (A1^order > 0), A1 = Delaunay neighbours + self loop; images with S_b <= 3 get the
 *      reference's special rows e0(+e1).  Computed on the device (empty-circle test per point pair;
 *      identical to Qhull for points in general position).  n_empty_out (HOST, may be NULL; passing it
 *      synchronises): low 16 bits = number of NaN centroids (= empty masks, for which the reference raises
 *      ValueError); bits 16.. = number of images holding a NON-GENERIC configuration (a duplicate centroid, or
 *      four centroids co-circular -- exactly or to within rounding -- with an empty circle), where the Delaunay triangulation is not unique
 *      and Qhull's choice cannot be reproduced: callers that need the reference's result bit for bit recompute
 *      such batches with Qhull (pipeline.py does). */
int segvlad_adjacency(segvlad_ctx* ctx, const double* centroids, const int32_t* seg_offsets, int B, int order,
                      uint8_t* adj_out, uint32_t* n_empty_out);

/*      The same, with one flag byte per image instead of the two counts: img_flags_out [B] (HOST or device; a host
 *      pointer synchronises): bit 0 = the image holds an empty mask (NaN centroid), bit 1 = it holds a non-generic
 *      centroid configuration (duplicate centroids, or four centroids co-circular exactly or to within rounding).
 *      A caller that needs the reference's result bit for bit recomputes exactly the flagged images with Qhull
 *      (pipeline.py does: ~0.2 ms of host work per flagged image instead of the whole batch). */
int segvlad_adjacency_flagged(segvlad_ctx* ctx, const double* centroids, const int32_t* seg_offsets, int B, int order,
                              uint8_t* adj_out, uint8_t* img_flags_out);

/* ---- segment VLAD for a batch of B images of identical token geometry
 *      seg_vlad_gpu_single(_img) -> vlad_single -> vlad_matmuls_per_cluster   func_vpr.py:1065-1210
 *      tokens      [B][D][N] fp32, as stored by the reference (D-major, N contiguous)
 *      inc_bits    [S_tot][ceil(N/64)] u64 from segvlad_incidence
 *      seg_offsets [B+1] int32 HOST: segments of image b are rows seg_offsets[b]..seg_offsets[b+1]
 *      adj         concatenated per-image [S_b][S_b] byte matrices (row-major, non-zero = 1), or
 *                  NULL for order 0 (identity)                                func_vpr.py:1192-1193
 *      out         [S_tot][K*D] fp32, cluster-major, intra-normalised then L2-normalised
 *      labels_out  [B][N] u8 or NULL      (argmax_k <x^, c^_k>, first max)    func_vpr.py:1146
 *      gap_out     [B][N] fp32 or NULL    (top-1 minus top-2 cosine: the tie audit)
 *      block_norms_out [S_tot][K] fp32 or NULL (||V[s,k,:]|| before intra-normalisation)          */
int segvlad_images(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits,
                   const int32_t* seg_offsets, const uint8_t* adj, float* out, uint8_t* labels_out,
                   float* gap_out, float* block_norms_out);

/* ---- fused segvlad_images + segvlad_pca_apply: the per-batch pair of place_rec_main.py:259-270
 *      (seg_vlad_gpu_single per image, then apply_pca_transform_from_pkl on the batch) in one call.  The
 *      aggregation kernel emits the projection GEMM's input planes directly, so the K*D-wide fp32 descriptor is
 *      neither measured (max |x|), nor re-read, nor -- when desc_out is NULL -- written to HBM at all; with
 *      desc_out == NULL the call may not even form it (option "pca_path": the tokens' residuals are projected with
 *      their cluster's slice of the components and the segments aggregated in the P-dimensional space -- the same
 *      linear map in another order, fp32-class like the other form).
 *      y [S_tot][P] fp32 (l2norm != 0: rows normalised as normalizeFeat); desc_out [S_tot][K*D] fp32 or NULL;
 *      other arguments as segvlad_images.  Requires segvlad_set_vocab and segvlad_pca_set (KD == K*D).      */
int segvlad_images_pca(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits,
                       const int32_t* seg_offsets, const uint8_t* adj, float* y, int l2norm, float* desc_out,
                       uint8_t* labels_out, float* gap_out);

/* ---- the describe stage of a batch in ONE call: the per-image chain of place_rec_main.py:244-263 (preload_masks -> masks ->
 *      nbrMasksAGGFastSingle -> seg_vlad_gpu_single) plus, with y != NULL, the per-batch apply_pca_transform_from_pkl (:269).
 *      = segvlad_incidence_centroids + segvlad_adjacency_flagged + segvlad_images / segvlad_images_pca with the same arguments
 *      and the same results; the mask branch runs on a second stream of the context beside the token-assignment pass.
 *      All bulk pointers are DEVICE memory, seg_offsets [B+1] HOST.  The intermediates come back in caller-owned buffers
 *      (inc_bits_out [S_tot][ceil(N/64)], centroids_out [S_tot][2] fp64, adj_out concatenated [S_b][S_b] bytes, img_flags_out [B]:
 *      bit 0 empty mask, bit 1 non-generic centroids -- see segvlad_adjacency_flagged: a caller that needs the reference's result
 *      bit for bit patches the flagged images' adjacency with Qhull and describes again through segvlad_images[_pca]).
 *      desc_out [S_tot][K*D] and / or y [S_tot][P] (one of them may be NULL).                                            */
int segvlad_describe(segvlad_ctx* ctx, const uint8_t* masks, int Hm, int Wm, int H, int W, int patch, const float* tokens, int B, int N,
                     const int32_t* seg_offsets, int order, uint64_t* inc_bits_out, double* centroids_out, uint8_t* adj_out,
                     uint8_t* img_flags_out, float* desc_out, float* y, int l2norm);
/*      The same stage as THREE calls, for a caller that patches flagged images with Qhull WHILE the device works:
 *      segvlad_describe_begin   enqueues the mask branch (side stream; its flags and centroids are also copied to pinned host
 *                               memory behind it) and the assignment pass (the context's stream), and returns.  pca != 0: the
 *                               projected form will be asked of segvlad_describe_end (checked here).
 *      segvlad_describe_flags   waits for the MASK BRANCH only -- the assignment pass keeps the device busy -- and hands the
 *                               per-image flags [B] (and, if asked for, the centroids [S_tot][2]) to HOST buffers.
 *      segvlad_describe_end     n_patch adjacency blocks recomputed by the caller (patch_images [n_patch] HOST, ascending image
 *                               indices; patch_blocks HOST: their [S_b][S_b] byte matrices, concatenated) are written over the
 *                               device's, then prep -> aggregation (-> projection) run: the result is that of segvlad_images[_pca]
 *                               with the patched adjacency.  Same tokens / inc_bits / seg_offsets / adj buffers as in begin:
 *                               from begin to end they (and the other outputs of begin) are the library's, unchanged.  The masks
 *                               are read by the mask branch only, on the context's second stream: the caller may overwrite them
 *                               once segvlad_describe_flags has returned (it waits for that branch), without it once
 *                               segvlad_describe_end has.  patch_images / patch_blocks may be overwritten when end returns.
 *      A begin must be followed by an end (flags is optional) before any other describe / incidence / adjacency / images /
 *      cluster_aggregate call on the context: those return SEGVLAD_ERR_STATE while a begin is open (round 6; the rule used to
 *      be documented only).  segvlad_describe_begin and segvlad_describe return SEGVLAD_ERR_LIMIT -- "this entry point cannot,
 *      the separate ones can" -- for an empty batch (B == 0 or no segments), for a PCA model without the fp16x3 form
 *      (option pca_arith=fp32, or K*D not a multiple of 32) and for an image with more segments than the in-LDS Delaunay holds.   */
int segvlad_describe_begin(segvlad_ctx* ctx, const uint8_t* masks, int Hm, int Wm, int H, int W, int patch, const float* tokens, int B,
                           int N, const int32_t* seg_offsets, int order, uint64_t* inc_bits_out, double* centroids_out, uint8_t* adj_out,
                           uint8_t* img_flags_out, int pca);
int segvlad_describe_flags(segvlad_ctx* ctx, uint8_t* flags_host, double* centroids_host);
int segvlad_describe_end(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits, const int32_t* seg_offsets,
                         uint8_t* adj, int n_patch, const int32_t* patch_images, const uint8_t* patch_blocks, float* desc_out, float* y,
                         int l2norm);

/* ---- vocabulary k-means, one Lloyd half-step over a batch of images: the fit that writes c_centers.pt
 *      (vlad_c_centers_pt_gen.py:86-158 -> utilities.py:749-791 VLAD.fit -> fast_pytorch_kmeans.KMeans(mode='cosine').fit).
 *      With the CURRENT centres in the context (segvlad_set_vocab): every token is assigned to the centre of largest cosine
 *      (normalised token against normalised centre, first maximum -- the assignment kernel of segvlad_images), and
 *        sums [K][D]  fp64 += sum of the NORMALISED tokens assigned to each centre      (DEVICE memory, accumulated into)
 *        counts [K]   int64 += number of tokens assigned to each centre                 (DEVICE memory, accumulated into)
 *      so that a caller walks its token set in batches, then sets centre k to sums[k] / counts[k] (centres that lost all their
 *      tokens keep their value; the means are NOT re-normalised, utilities.py:749-791).  tokens [B][D][N] fp32 as
 *      segvlad_images takes them; labels_out [B][N] bytes or NULL.  Deterministic (fixed summation order, no atomics on the
 *      sums).  Round 6: replaces the round-3 recovery of the sums from normalised VLAD descriptors.                              */
int segvlad_kmeans_step(segvlad_ctx* ctx, const float* tokens, int B, int N, double* sums, int64_t* counts, uint8_t* labels_out);

/* ---- the K-parametric entry: vlad_matmuls_per_cluster(num_c, masks, res, clus_labels, adjMat)
 *      func_vpr.py:1181-1210.  res [N][D] fp32 residuals (token-major, as the reference passes them),
 *      labels [N] u8 (< num_c <= 256), inc_bits [S][ceil(N/64)], adj [S][S] bytes or NULL,
 *      out [S][num_c*D] fp32.  Independent of the vocabulary held by the context.                  */
int segvlad_cluster_aggregate(segvlad_ctx* ctx, int num_c, const float* res, const uint8_t* labels, int N, int D,
                              const uint64_t* inc_bits, int S, const uint8_t* adj, float* out);

/* ---- PCA apply: pickle.load + PCA.transform                          func_vpr.py:1419-1443
 *      Y = ((X - mean) @ comps^T) / sqrt(expl_var) when whiten!=0.  comps [P][KD] fp32.          */
int segvlad_pca_set(segvlad_ctx* ctx, const float* mean, const float* comps, const float* expl_var, int P, int KD,
                    int whiten);
/*      X [n][KD] -> Y [n][P]; l2norm!=0 additionally applies normalizeFeat (func_vpr.py:1673-1676).
 *      Accuracy.  With KD % 32 == 0 (and option pca_arith != fp32) the product runs as a two-term fp16 split on the 16-bit
 *      matrix pipe, with ONE power-of-two scale per batch (from max|X| + max|mean| over the finite entries) and ONE per model
 *      (from max|comps|).  A row of X - mean (a row of comps) whose largest element is at least 2^-12 of that maximum comes
 *      out fp32-class relative to ITS OWN magnitude, like an fp32 product.  Below that the second fp16 terms are sub-normal:
 *      the absolute error per element is bounded by 2^-25 of the scaled unit (2^-38 of the batch / model maximum), so the
 *      row's relative error grows as the row shrinks -- about 1e-5 at 2^-20 and 2e-4 at 2^-24 of the maximum (K = 2048)
 *      against 1e-6 for fp32.  With a mean, X - mean keeps the rows of a descriptor batch at one scale; a caller whose rows
 *      (or whose components: the PCA fit's X^T operand) span more than 2^12 and who needs the small ones to full relative
 *      accuracy sets pca_arith=fp32.  A NaN / Inf row of X gives a non-finite row of Y and leaves the other rows alone.
 *      (tests/test_gpu_projection.py holds every output entry to this.)  On that path a device pointer X must be 16-byte
 *      aligned (SEGVLAD_ERR_ARG otherwise; nothing is staged: X may be far larger than any scratch buffer).        */
int segvlad_pca_apply(segvlad_ctx* ctx, const float* X, int n, float* Y, int l2norm);

/* ---- row L2 normalisation: normalizeFeat                             func_vpr.py:1673-1676
 *      (no epsilon: an all-zero row becomes NaN exactly like the reference).  X may equal Y.      */
int segvlad_normalize_rows(segvlad_ctx* ctx, const float* X, int n, int d, float* Y);

/* ---- exact kNN: faiss.IndexFlatL2(d).add / .search                   place_rec_main.py:53-60
 *      The index keeps a device copy of the rows.  img_of_seg (imIndsRef / imInds1,
 *      place_rec_main.py:252) may be NULL if segvlad_vote is given the map explicitly.            */
int segvlad_db_reset(segvlad_ctx* ctx);
/*      Rows holding NaN / +-Inf are stored like any other and are never listed: "Non-finite rows" at segvlad_search.    */
int segvlad_db_add(segvlad_ctx* ctx, const float* R, int n, int d, const int32_t* img_of_seg);
int segvlad_db_size(segvlad_ctx* ctx, int64_t* n_rows, int* d);

/* ---- removal from the index: faiss IndexFlat::remove_ids (no reference counterpart: the reference builds its index once,
 *      place_rec_main.py:53-60; this is the upkeep of a deployed map).
 *      A row is removed when its id is listed in row_ids [n_row_ids] int64, or when its image id (img_of_seg of
 *      segvlad_db_add) is listed in img_ids [n_img_ids] int32.  Either list may be NULL / empty.  Ids outside 0 .. n-1,
 *      negative image ids, image ids no row carries and duplicates are ignored.  img_ids on an index without an img_of_seg
 *      map: SEGVLAD_ERR_STATE.
 *      The surviving rows keep their order and are renumbered 0 .. n'-1 (faiss's semantics: every id above a removed one
 *      moves down).  new_id_out [n] int64 or NULL: the new id of every OLD row, -1 if it was removed.  n_removed_out: HOST,
 *      may be NULL.
 *      Afterwards every segvlad_search / _search_shortlist / _vote (img_of_seg NULL) / _search_sharded returns, bit for
 *      bit, what a fresh context returns that holds the surviving rows (and their image ids) from one segvlad_db_add.
 *      Removing every row leaves an empty index that keeps its dimension and its img_of_seg rule: a search then returns
 *      (+inf, -1) in every slot.  Synchronises.  Peak device memory during the call: the old AND the new buffers.   */
int segvlad_db_remove(segvlad_ctx* ctx, const int64_t* row_ids, int64_t n_row_ids, const int32_t* img_ids, int n_img_ids,
                      int64_t* new_id_out, int64_t* n_removed_out);
/*      d2_out [nq][k] fp32 ascending squared L2; idx_out [nq][k] int64 (ties -> lower id; slots
 *      beyond the database size hold (+inf, -1) like faiss).  1 <= k <= 1024.
 *      Non-finite rows.  NaN and +-Inf are ordinary input of segvlad_db_add and segvlad_search (segvlad_normalize_rows turns an
 *      all-zero row into a NaN row on purpose), in any number, whether they arrive with the first segvlad_db_add or a later one:
 *      - never listed: a pair whose fp32 distance is NaN or +inf is never listed (the hit rule of segvlad_range_search, and of
 *        faiss, whose heap admits neither).  An index row holding NaN or +-Inf is in nobody's list; a query row holding one
 *        returns (+inf, -1) in every slot; a list with fewer than k finite distances is padded with (+inf, -1).  No slot holds a
 *        NaN distance, or a valid id beside a non-finite distance.
 *      - isolation: a query row whose values are all finite gets, ids and distance bits, what segvlad_search returns on an index
 *        holding only the finite rows (ids as segvlad_db_remove would renumber them) -- on every plan and under every option.
 *        A row is never listed exactly when its fp32 squared norm is not finite: it holds NaN / +-Inf, or it is all finite and
 *        its norm overflows.  The fp16 scales of the index and of the queries, max |r|^2 of the filters' margins and min |q|^2
 *        are all taken over the other rows alone, whatever finite entries a never-listed row holds.
 *      - no collateral cost: the bad rows send no other row to the redo or the matrix fallback (a bad query row itself may go).  */
int segvlad_search(segvlad_ctx* ctx, const float* Q, int nq, int k, float* d2_out, int64_t* idx_out);

/* ---- shortlist-restricted exact search (no reference counterpart: the reference searches the whole index,
 *      place_rec_main.py:53-60; this is the re-ranking of a global shortlist / a location prior of deployed place recognition).
 *      Q [nq][d] query segment rows (device or host), qseg_offsets [n_img+1] int32 HOST as in segvlad_vote: query image b owns
 *      the rows qseg_offsets[b] .. qseg_offsets[b+1]-1 (0 rows allowed).  shortlist [n_img][M] int32: the reference image ids
 *      (the img_of_seg values given to segvlad_db_add) that image b's segments may match; -1 is padding, a duplicate counts
 *      once, an id no row carries contributes no rows.  1 <= M <= 4096, 1 <= k <= 1024.
 *      d2_out [nq][k] / idx_out [nq][k]: per query row the top-k rows of the index whose image is in its image's shortlist,
 *      ordered by (squared L2, lower id) as segvlad_search; (+inf, -1) beyond the number of allowed rows.  Every distance is
 *      the exact fp32 chain of segvlad_search (sequential fma dot product in k order, the stored row norms, negatives set to
 *      0): a pair's value is bit for bit segvlad_search's, and a shortlist of every image returns segvlad_search(Q, k).
 *      Non-finite rows: the rule of segvlad_search (never listed, isolation).
 *      SEGVLAD_ERR_STATE without an img_of_seg map; SEGVLAD_ERR_LIMIT when d % 32 != 0.  The image -> row map is built on
 *      the device by the first call after segvlad_db_add / segvlad_db_reset.                                          */
int segvlad_search_shortlist(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img,
                             const int32_t* shortlist, int M, int k, float* d2_out, int64_t* idx_out);

/* ---- search excluding image-id windows per query image (no reference counterpart: the reference searches the whole index,
 *      place_rec_main.py:53-60; this is the self-query of a live map -- loop closure, the leave-one-out check of a map -- where
 *      the query image's own rows and its neighbours in time are in the index).
 *      Q [nq][d] device or host; qseg_offsets [n_img+1] int32 HOST as in segvlad_search_shortlist (0 rows allowed).
 *      excl [n_img][E][2] int32 HOST: per query image E inclusive intervals [lo, hi] of reference image ids (the img_of_seg
 *      values of segvlad_db_add) its rows must not match.  lo > hi is an empty interval (padding); intervals may overlap, reach
 *      below 0 or above the largest id, cover ids no row carries.  1 <= E <= 8, 1 <= k <= 1024.  A row whose image id is
 *      negative is never excluded.
 *      d2_out / idx_out [nq][k]: per query row the top-k rows of the index whose image id lies in none of its image's intervals,
 *      ordered by (squared L2, lower id); (+inf, -1) beyond the number of allowed rows -- bit for bit what segvlad_search
 *      returns on an index without those images (ids aside).  All intervals empty: exactly segvlad_search(Q, k).
 *      Non-finite rows: the rule of segvlad_search (never listed, isolation).
 *      The search runs once at depth k_fetch = min(1024, k + the largest number of rows any query image excludes) and keeps
 *      each row's first k allowed entries; rows of an image whose window holds more than 1024 - k rows AND fills the row's
 *      nearest 1024 are finished by an exact fp32 pass over the allowed rows (needs every row's image id >= 0: a call whose
 *      largest window holds more than 1024 - k rows on an index with a negative image id returns SEGVLAD_ERR_LIMIT).  SEGVLAD_ERR_STATE without an img_of_seg map; SEGVLAD_ERR_LIMIT when d % 32 != 0; SEGVLAD_ERR_ARG
 *      on bad shapes, offsets or E.  Stage timer "knn_exclude": the kernels this call adds to the inner search's own stages.
 *      segvlad_exclude_stats: HOST array, up to 4 values, of the last segvlad_search_excluding -- [0] the depth the inner
 *      search ran at (k_fetch), [1] the largest number of excluded index rows of any query image that owns rows, [2] query
 *      rows finished by the exact pass, [3] query images (that own rows) with at least one excluded row.  Synchronises. */
int segvlad_search_excluding(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img,
                             const int32_t* excl, int E, int k, float* d2_out, int64_t* idx_out);
int segvlad_exclude_stats(segvlad_ctx* ctx, int64_t* stats_out, int n);

/* ---- grouped search: top-k with at most per_image rows per reference image (no reference counterpart: the reference's vote
 *      adds one similarity per HIT, get_matches / max_seg_topk_wt_borda_Im, func_vpr.py:207-224, so on a map with revisited
 *      places one query segment gives one image dozens of votes; retrieval engines call this a grouped or collapsed search).
 *      Q [nq][d] device or host.  1 <= k <= 1024, 1 <= per_image <= 16.  d2_out / idx_out [nq][k], device or host.
 *      Let L(q) be the unbounded segvlad_search list of row q: every index row in ascending (squared L2, lower id) order, the
 *      distances the search's exact fp32 chain (sequential fma dot product in k order, the stored row norms,
 *      fmaf(-2, dot, |q|^2 + |r|^2), negatives set to 0).  An entry of L(q) is KEPT when fewer than per_image EARLIER entries
 *      of L(q) carry its image id (the img_of_seg value given to segvlad_db_add); a row whose image id is negative is a group
 *      of its own and is always kept.  The output is the first k kept entries, in their order; slots behind them hold
 *      (+inf, -1).  Hence: with per_image at least every image's row count, and on an index whose image ids are all distinct,
 *      the call returns segvlad_search(Q, k) bit for bit; with per_image = 1 the ids of a row name k different images.
 *      How: the search runs once at depth k_fetch = min(1024, 4 k) and each row's list is collapsed on the device; a row that
 *      neither kept k entries nor reached the index's end within k_fetch is finished by an exact pass -- the exact distance
 *      blocks of segvlad_range_search over the whole index, ordered, collapsed by the same rule (in batches whose scratch --
 *      two word buffers of 8 bytes per index row, and one byte per image id up to the largest, per query row -- stays within
 *      1 GiB, at least one row).  Non-finite rows: the rule of segvlad_search (never listed, isolation), in the fetched lists
 *      and in the exact pass alike -- that pass takes a hit as the range search does, d2 < +inf, and the fetched list ends at its
 *      first (+inf, -1) slot.  A query row holding a non-finite value is never sent to the exact pass: its fetched list is
 *      empty, it returns (+inf, -1) in every slot.
 *      Cost: what a caller pays is the depth of the inner search, 4 k: any k >= 245 fetches >= 977 entries, where on a
 *      1 M-row index the search plan leaves its filter levels for the distance-matrix path (tens of times slower; see
 *      segvlad_search_excluding); and every open row streams the whole index once more.  Keep k below that where it matters.
 *      SEGVLAD_ERR_STATE without an img_of_seg map or with no dimension yet; SEGVLAD_ERR_ARG on null pointers, negative nq, k
 *      or per_image out of range; more than 2^32 - 1 index rows: SEGVLAD_ERR_LIMIT, as in the range search.  nq == 0: OK.  An
 *      index that removal has emptied: (+inf, -1) everywhere.  Works after any sequence of segvlad_db_add / segvlad_db_remove.
 *      Deterministic: two calls return the same bits.  Synchronises once (the number of rows the collapse left open has to
 *      reach the host; the exact pass synchronises again).  Stage timer "knn_group": the kernels this call adds to the inner
 *      search's own stages.  One index, one context: the row-sharded and query-sharded classes have no counterpart yet.
 *      Where only the vote's weight of one image per segment matters, SEGVLAD_VOTE_PER_IMAGE (segvlad_vote) caps the hits in
 *      the vote instead: it costs no second search and does not back-fill the lists.
 *      segvlad_group_stats: HOST array, up to 3 values, of the last segvlad_search_grouped -- [0] the depth the inner search
 *      ran at (k_fetch), [1] query rows finished by the exact pass, [2] the largest number of list entries any row read
 *      before the collapse declared it complete (rows the exact pass finished do not count).                              */
int segvlad_search_grouped(segvlad_ctx* ctx, const float* Q, int nq, int k, int per_image, float* d2_out, int64_t* idx_out);
int segvlad_group_stats(segvlad_ctx* ctx, int64_t* stats_out, int n);

/* ---- exact range search: faiss IndexFlat::range_search (no reference counterpart: the reference only searches top-k,
 *      place_rec_main.py:53-60, and turns distances into similarities with 2 - d^2, place_rec_main.py:78-81 -- a similarity
 *      floor s on unit rows is the squared radius 2 - s).  Loop closure and map upkeep ask "which rows are closer than this?".
 *      Q [nq][d] device or host.  radius2 [nq] fp32, device or host: one SQUARED radius per query row.
 *      A pair (q, r) is a hit when d2(q, r) < radius2[q], strictly, as faiss.  d2 is exactly the value segvlad_search reports
 *      for that pair (sequential fma dot product in k order, the stored row norms, fmaf(-2, dot, |q|^2 + |r|^2), negatives
 *      set to 0): a hit list is, bit for bit, the entries of an unbounded segvlad_search list that lie below the radius.
 *      A radius that is NaN, zero or negative yields no hit; +inf yields every row whose distance is neither NaN nor +inf; a
 *      query row holding NaN yields no hit.
 *      lims_out [nq + 1] int64, device or host: lims[0] = 0, row q's hits occupy slots lims[q] .. lims[q+1]-1.  Always
 *      written, always the true counts.  n_total_out (HOST, may be NULL) = lims[nq].
 *      d2_out / idx_out hold `capacity` slots each (device or host; both may be NULL when capacity == 0: a count-only call).
 *      When lims[nq] <= capacity they receive the hits, each row's in ascending (d2, lower id) order, the order of
 *      segvlad_search.  When lims[nq] > capacity they are NOT WRITTEN AT ALL, the call still returns SEGVLAD_OK, and the
 *      caller allocates lims[nq] slots and calls again.  Slots beyond lims[nq] are never written.
 *      An index that removal has emptied: all-zero lims.  No dimension yet: SEGVLAD_ERR_STATE.  nq == 0: OK.  Bad pointers /
 *      negative sizes: SEGVLAD_ERR_ARG.  More than 2^32 - 1 index rows: SEGVLAD_ERR_LIMIT (candidate ids are 32-bit, as in
 *      the search).  Works after any sequence of segvlad_db_add / segvlad_db_remove, like segvlad_search.  Deterministic: two
 *      calls return the same bits.  Synchronises (the total has to reach the host).
 *      How: d % 64 == 0 (d <= 8192) on more than 32 768 rows -- ONE pass of the search's fp16 filter over every row under
 *      thr = radius2 with its rigorous margin, then the exact chain on every candidate; a row with more than 8192 candidates
 *      (or a +inf radius), and every row of the other shapes or under option knn_filter = fp32, goes through exact fp32
 *      distance blocks against slabs of the index, counted in one sweep and emitted in a second.  Stage timer "knn_range".
 *      segvlad_range_stats: HOST array, up to 5 values, of the last segvlad_range_search -- [0] total hits, [1] query rows
 *      finished by the long-row path, [2] max and [3] sum of the candidate-list lengths the filter produced, [4] the path
 *      taken (0 exact blocks, 1 fp16 filter).                                                                            */
int segvlad_range_search(segvlad_ctx* ctx, const float* Q, int nq, const float* radius2, int64_t* lims_out, float* d2_out,
                         int64_t* idx_out, int64_t capacity, int64_t* n_total_out);
int segvlad_range_stats(segvlad_ctx* ctx, int64_t* stats_out, int n);

/* ---- mutual nearest segments between query images and candidate reference images (no reference counterpart as a batched
 *      call: get_matches_for_single_image_pair, func_vpr.py:247-270, studies ONE query / reference pair on the host; this is
 *      the verification step behind the vote -- does query image b really show candidate image c? -- whose counts and summed
 *      similarities re-rank the vote's top-n).
 *      Q [nq][d] device or host; qseg_offsets [n_img+1] int32 HOST as in segvlad_search_shortlist (0 rows allowed).
 *      cand [n_img][C] int32 HOST: reference image ids (the img_of_seg values of segvlad_db_add), 1 <= C <= 64.  -1 is
 *      padding -- segvlad_vote's pred_out can be passed as it is --, an id no row carries behaves like -1, and every slot is
 *      evaluated on its own: a duplicate id gets the same answer twice.
 *      For slot (b, j): A = the query rows of image b, B = the index rows whose image id is cand[b][j].  d2(q, r) is exactly
 *      the value segvlad_search reports for the pair (sequential fma dot product in k order, the stored row norms,
 *      fmaf(-2, dot, |q|^2 + |r|^2), negatives set to 0).  fwd(q) = the row of B with the smallest (d2, row id) -- what
 *      segvlad_search_shortlist returns for the shortlist {cand[b][j]} at k = 1 --, bwd(r) = the row of A with the smallest
 *      (d2, query row index); a NaN distance is never anyone's nearest.  The pair (q, fwd(q)) is MUTUAL when
 *      bwd(fwd(q)) == q and d2 < max_d2, strictly: max_d2 = +inf admits every finite distance; NaN, zero or a negative value
 *      admit none (the rule of segvlad_range_search's radii).
 *      Outputs, device or host; all but n_mutual_out and score_out may be NULL:
 *        n_mutual_out [n_img][C] int32   the number of mutual pairs (0 when A or B is empty)
 *        score_out    [n_img][C] fp64    the sum over the mutual pairs, in ascending query-row order, of (double)(2.0f - d2):
 *                                        the subtraction in fp32 as in segvlad_sims_from_d2, the additions in fp64 in that
 *                                        fixed order -- a host loop reproduces it bit for bit
 *        order_out    [n_img][C] int32   image b's slots sorted by (n_mutual desc, score desc, slot asc); slots that are -1
 *                                        or carry no rows come last, in slot order: cand[b][order[b][j]] is the re-ranked list
 *        fwd_idx_out  [nq][C] int64, fwd_d2_out [nq][C] fp32   fwd(q) and its distance; (-1, +inf) where B is empty
 *        mutual_out   [nq][C] uint8      1 where (q, fwd(q)) is mutual, else 0
 *      SEGVLAD_ERR_STATE without an img_of_seg map or with no dimension yet; SEGVLAD_ERR_LIMIT when d % 32 != 0 (the shortlist
 *      search's limit); SEGVLAD_ERR_ARG on bad pointers, offsets, C, or nq != qseg_offsets[n_img].  nq == 0: OK; with n_img > 0 the per-image outputs are
 *      still written (zero counts and scores, the slots that carry rows first).  Deterministic: two calls return the same bits.  Works after any sequence of segvlad_db_add /
 *      segvlad_db_remove: it uses the image -> row map of segvlad_search_shortlist, whose offsets are mirrored on the host --
 *      the FIRST call after the index changed synchronises once for that copy; otherwise the call does not synchronise when
 *      every output is device memory (the grid and the scratch are sized on the host from cand; host outputs are copied back
 *      behind one synchronisation).  Stage timer "match_pairs".  One index, one context: the row-sharded and query-sharded
 *      classes have no counterpart yet.                                                                                  */
int segvlad_match_pairs(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img, const int32_t* cand, int C,
                        float max_d2, int32_t* n_mutual_out, double* score_out, int32_t* order_out, int64_t* fwd_idx_out,
                        float* fwd_d2_out, uint8_t* mutual_out);

/* ---- spatial verification of matched segments: how many correspondences of a query image / candidate pair agree on one 2-D
 *      similarity transform of their centroids (no reference counterpart: the reference stops at the vote, func_vpr.py:207-224, and
 *      looks at the matches of ONE image pair by eye, func_vpr.py:247-270).  The step behind segvlad_match_pairs: a count of mutual
 *      pairs says two images hold similar-looking segments, this call says whether they are laid out the same way.  It does not
 *      touch the index and works on any correspondences.
 *      q_xy [nq][2] fp64 (x, y) centroid of every query row, r_xy [n_r][2] fp64 centroid of every index row id (the caller's
 *      table -- segvlad_mask_centroids / segvlad_incidence_centroids produce such centroids --, compacted with new_id_out after
 *      segvlad_db_remove); both device or host.  qseg_offsets [n_img+1] int32 HOST as in segvlad_match_pairs (0 rows allowed).
 *      fwd_idx [nq][C] int64 and mutual [nq][C] uint8, device or host: segvlad_match_pairs' fwd_idx_out / mutual_out, 1 <= C <= 64.
 *      Correspondences of slot (b, j): the query rows q of image b, in ascending q, with mutual[q][j] != 0 and
 *      0 <= fwd_idx[q][j] < n_r and all four coordinates (q_xy[q], r_xy[fwd_idx[q][j]]) finite.  Any other row is dropped: not a
 *      correspondence, not an inlier, inlier_out 0.  M = their number, (p_m, s_m) the m-th: p the query point, s the reference point.
 *      Hypotheses: every pair i < j of the M correspondences, numbered h = 0, 1, ... in lexicographic (i, j) order.  The search is
 *      exhaustive: no sampling, no seed.
 *      Arithmetic, fp64, every operation separately rounded (no fused multiply-add) and in exactly this order.  Hypothesis (i, j):
 *        dx = p_j.x - p_i.x, dy = p_j.y - p_i.y;  ex = s_j.x - s_i.x, ey = s_j.y - s_i.y
 *        n = dx*dx + dy*dy, m = ex*ex + ey*ey;  ar = ex*dx + ey*dy, ai = ey*dx - ex*dy
 *      It is ELIGIBLE when n > 0 && (min_scale*min_scale)*n <= m && m <= (max_scale*max_scale)*n.  Correspondence t is an INLIER when, with
 *        px = p_t.x - p_i.x, py = p_t.y - p_i.y;  sx = s_t.x - s_i.x, sy = s_t.y - s_i.y
 *        ux = (ar*px - ai*py) - n*sx, uy = (ar*py + ai*px) - n*sy
 *      ux*ux + uy*uy < ((tol*tol)*n)*n, strictly: |a (p_t - p_i) - (s_t - s_i)| < tol for the similarity a = ds conj(dp) / |dp|^2,
 *      multiplied through by n -- no division and no square root on the decision path, so a host loop in fp64 reproduces every
 *      decision bit for bit.
 *      Winner: the eligible hypothesis with the most inliers, ties to the lowest h.  Outputs, device or host; all but
 *      n_inlier_out may be NULL:
 *        n_inlier_out [n_img][C] int32     the winner's inlier count; 0 when M < 2 or no hypothesis is eligible
 *        pair_out     [n_img][C][2] int32  the query rows (q_i, q_j) of the winner's sample; (-1, -1) when there is none
 *        model_out    [n_img][C][4] fp64   (a_re, a_im, t_x, t_y): a = (ar/n, ai/n), t = s_i - a p_i; NaN when there is none.
 *                                          Informative only: it plays no part in any decision
 *        order_out    [n_img][C] int32     image b's slots sorted by (n_inlier desc, slot asc)
 *        inlier_out   [nq][C] uint8        1 where the row is an inlier of its slot's winner, else 0
 *      SEGVLAD_ERR_ARG on null required pointers, negative sizes, C outside 1 .. 64, bad offsets or nq != qseg_offsets[n_img],
 *      qseg_offsets in device memory, tol not finite or <= 0, or unless 0 < min_scale <= max_scale < inf.  SEGVLAD_ERR_LIMIT when
 *      a query image owns more than 256 rows: the exhaustive search is cubic in M (about 14 M * M (M - 1) / 2 fp64 operations
 *      per slot).  n_img == 0: OK.  nq == 0 with n_img > 0: the per-image outputs are still written (zeros, (-1, -1), NaN, the
 *      identity order).  Deterministic: two calls return the same bits.  The call does not synchronise when every output is
 *      device memory (the grid is sized on the host from qseg_offsets alone; host outputs are copied back behind one
 *      synchronisation).  Stage timer "verify_pairs".                                                                       */
int segvlad_verify_pairs(segvlad_ctx* ctx, const double* q_xy, int nq, const double* r_xy, int64_t n_r, const int32_t* qseg_offsets,
                         int n_img, int C, const int64_t* fwd_idx, const uint8_t* mutual, double tol, double min_scale,
                         double max_scale, int32_t* n_inlier_out, int32_t* pair_out, double* model_out, int32_t* order_out,
                         uint8_t* inlier_out);

/* ---- re-ranking by consistency along the query sequence: a candidate of query frame t is believed when the frames around t hold
 *      candidates that lie on one line through the map (no reference counterpart: the reference judges every query image alone,
 *      func_vpr.py:207-224).  SeqSLAM's trajectory search, restricted to the candidate lists: the last stage behind segvlad_vote,
 *      segvlad_match_pairs and segvlad_verify_pairs, all of which look at one query image.  It never reads the d-wide rows and
 *      does not touch the index or the vocabulary.
 *      Image ids MUST be frame numbers along the map -- consecutive ids are consecutive places, the assumption of
 *      engine.window_intervals and segvlad_search_excluding --, and the query frames of a sequence are in time order.
 *      The lists' truncation to C candidates is the approximation: a frame's vote is zero outside the images it voted for, so a
 *      frame supports a line only through the C images it lists (the dense frame x map score matrix is not built).
 *      cand [T][C] int32, device or host: the candidate reference image ids of query frame t -- segvlad_vote's pred_out as it
 *      is --, 1 <= C <= 64.  score [T][C] fp64, device or host: one evidence value per slot, meant to be >= 0 -- the vote's
 *      score_out, or n_mutual / n_inlier as doubles.  A slot is EMPTY when cand < 0 or its score is not finite; every other slot
 *      is evaluated on its own (a duplicate id in a frame gets the same answer twice).
 *      seq_offsets [n_seq+1] int32 HOST, ascending, seq_offsets[0] == 0, seq_offsets[n_seq] == T: sequence s owns the frames
 *      seq_offsets[s] .. seq_offsets[s+1]-1 in time order (empty sequences allowed); a window never crosses a sequence boundary.
 *      0 <= back, fwd <= 32: the frames before and after t that are asked.  vel [n_vel] fp64 HOST: map frames per query frame,
 *      1 <= n_vel <= 16, every value finite with |v| <= 2^20; a negative value describes a reverse traversal.  0 <= tol <= 2^30:
 *      how far, in map frames, a neighbour's candidate may lie from the line.
 *      Arithmetic: fp64 and int64, every operation separately rounded and in exactly this order, so a host loop reproduces every
 *      bit.  For a non-empty slot (t, c) with r = cand[t][c] and velocity index u:
 *        acc = 0.0, hits = 0; for tau = -back .. fwd, ascending:
 *          tau == 0:  acc = acc + score[t][c]
 *          tau != 0 and frame t' = t + tau lies in t's sequence:
 *            p = (int64)r + (int64)rint(vel[u] * (double)tau)       -- one multiplication, rounded half to even
 *            sup = the LARGEST score among the non-empty slots j of frame t' with |(int64)cand[t'][j] - p| <= tol
 *            if there is such a slot: acc = acc + sup, hits += 1; otherwise nothing is added
 *      Winner: the u with the largest acc, ties to the lowest u.  Outputs, device or host; all but seq_score_out may be NULL:
 *        seq_score_out [T][C] fp64   the winner's acc; 0.0 for an empty slot
 *        n_hit_out     [T][C] int32  the winner's hits; 0 for an empty slot
 *        vel_out       [T][C] int32  the winner's u; -1 for an empty slot
 *        order_out     [T][C] int32  the frame's slots sorted by (seq_score descending, slot ascending), empty slots last in
 *                                    slot order: cand[t][order[t][j]] is the re-ranked list.  (A NaN sum -- infinite sums of
 *                                    both signs, which scores >= 0 never produce -- sorts behind every number.)
 *      SEGVLAD_ERR_ARG on null required pointers, negative sizes, C outside 1 .. 64, back or fwd outside 0 .. 32, n_vel outside
 *      1 .. 16, tol outside 0 .. 2^30, a velocity that is not finite or beyond 2^20 in magnitude, bad offsets or
 *      T != seq_offsets[n_seq], seq_offsets or vel in device memory.  T == 0: OK.  Deterministic: two calls return the same
 *      bits.  The call does not synchronise when every output is device memory (host outputs are copied back behind one
 *      synchronisation).  Stage timer "sequence_rerank".                                                                    */
int segvlad_sequence_rerank(segvlad_ctx* ctx, const int32_t* cand, const double* score, int T, int C, const int32_t* seq_offsets,
                            int n_seq, int back, int fwd, const double* vel, int n_vel, int tol, double* seq_score_out,
                            int32_t* n_hit_out, int32_t* vel_out, int32_t* order_out);

/* ---- merge of per-shard top-k lists (no reference counterpart: the reference is single-process).
 *      d2_parts/idx_parts [nq][parts*k] (shard-major within a row, global ids); output top-k by
 *      (distance, lower id).  An entry with id < 0 is an empty slot whatever its distance: it comes
 *      last and is returned as (+inf, -1).  The parts need not be sorted: sorted parts (the per-shard
 *      lists) are rank-merged, anything else -- an empty slot inside a part included -- is sorted, with
 *      the same result.  Limit: parts * k <= 8192 candidates per row (the LDS sort; 9 x 1024 returns
 *      SEGVLAD_ERR_LIMIT and leaves the context usable).                                              */
int segvlad_merge_topk(segvlad_ctx* ctx, const float* d2_parts, const int64_t* idx_parts, int nq, int parts, int k,
                       float* d2_out, int64_t* idx_out);

/* ---- top-50 slice + "2 - d^2":  sims_50 = 2 - sims[:, :50]           place_rec_main.py:78-81     */
int segvlad_sims_from_d2(segvlad_ctx* ctx, const float* d2, const int64_t* idx, int nq, int k_in, int k_keep,
                         float* sims_out, int64_t* idx_out);

/* ---- global min / max of the kept similarities                        func_vpr.py:212-213
 *      minmax_out [2] fp32 = {min, max}; +-inf take part like any value.  The empty list
 *      (count == 0) gives (NaN, NaN).                                                             */
int segvlad_minmax(segvlad_ctx* ctx, const float* sims, int64_t count, float* minmax_out);

/* ---- image vote: get_matches + weighted_borda_count                   func_vpr.py:61-77, 207-224
 *      idx [nq][k] int64 reference-segment ids, sims [nq][k] fp32, img_of_seg [n_ref_seg] int32
 *      (NULL = the map given to segvlad_db_add; n_ref_seg is then ignored), qseg_offsets [n_img+1]
 *      int32 HOST.
 *      smin/smax: the GLOBAL extrema (func_vpr.py:212-213); pass NaN to have them computed from
 *      `sims`.  pred_out [n_img][n_top] int32 (-1 padded), score_out [n_img][n_top] fp64 or NULL
 *      (mode COUNT: the integer vote count as a double).  Ties: first appearance (rank-major, then
 *      segment) for WT_BORDA_IM; (count desc, image id asc) for COUNT.
 *      An entry whose id lies outside [0, n_ref_seg) -- the -1 of an empty slot of a derived search --
 *      is skipped: it votes for nothing in either mode.  Its `sims` value still enters the extrema
 *      that the call computes itself (NaN smin/smax), so a caller whose lists carry empty slots passes
 *      the extrema of the kept entries (pipeline.py does).  A weight below 0 or above 1 (explicit
 *      extrema inside the data's range) is added like any other.  A query image's row of pred_out /
 *      score_out depends on that image's entries and the extrema alone, bit for bit: not on the other
 *      images of the call, whose sizes only choose the kernel's code path.
 *      Per-image cap: at most m hits per reference image from each query segment.
 *        #define SEGVLAD_VOTE_PER_IMAGE(m) ((m) << 8)      1 <= m <= 255; 0 = no cap
 *      mode = base | SEGVLAD_VOTE_PER_IMAGE(m): base = mode & 0x7f is SEGVLAD_VOTE_WT_BORDA_IM or SEGVLAD_VOTE_COUNT,
 *      m = (mode >> 8) & 0xff; any bit above bit 15, or an unknown base, returns SEGVLAD_ERR_ARG.  m == 0 is the call without
 *      a cap, launch for launch.  For m >= 1 take row q of idx and rank r: the entry is VALID when 0 <= idx[q][r] < n_ref_seg
 *      (the rule above), its image is g = img_of_seg[idx[q][r]] (images compare as 32-bit values, negative ones included), and
 *      it VOTES when it is valid and fewer than m valid entries at ranks r' < r of the same row carry the same g.  The call
 *      returns, bit for bit in pred_out and score_out, what the same call with mode = base returns on the same arguments with
 *      every non-voting entry's id replaced by -1.  Hence: the sums run in visiting order over the voting entries; ties go
 *      by the first appearance, which always votes; a COUNT score is the sum over the segments of min(m, hits) -- at m = 1 the
 *      number of query segments that see the image; with NaN smin / smax the extrema are still taken over ALL sims of the
 *      call (a caller that wants others passes them); m >= k blanks nothing; sims may be NULL in COUNT; and a query image's
 *      row still depends on that image's entries and the extrema alone.  How: one more launch in front of the vote (one wave
 *      per row marks the voting entries into a blanked copy of idx; stage "vote"), no further synchronisation.  The cap
 *      works behind every search variant and on lists a caller already holds; it does not back-fill a list with the entries
 *      behind the blanked ones (segvlad_search_grouped does).
 *      One-to-one vote: a reference segment votes once per query image.
 *        #define SEGVLAD_VOTE_UNIQUE_REF 0x80
 *      mode = base | SEGVLAD_VOTE_UNIQUE_REF | SEGVLAD_VOTE_PER_IMAGE(m), base = mode & 0x7f; the refusals above stand (0x82 has
 *      an unknown base).  Take query image b with S_b rows off[b] .. off[b+1]-1: entry (q, r) is VALID as above and its visiting
 *      position is p = r * S_b + (q - off[b]) (rank-major, then segment: the vote's order).  Among the valid entries of image b
 *      that carry the same id exactly one WINS: the one with the largest sims value, where a NaN loses to every number and
 *      +0.0 == -0.0; on a tie (equal values, or all NaN) the smallest p wins; with sims == NULL (COUNT only) the smallest p wins.
 *      Whenever sims is non-NULL it decides, in both bases.  Ids compare on all 64 bits; entries of different query images never
 *      interact.  The call returns, bit for bit in pred_out and score_out, what the same call without the flag returns on the
 *      same arguments with every non-winning valid entry's id replaced by -1; invalid entries stay as they are, and with NaN
 *      smin / smax the extrema are still taken over ALL sims of the call.  Together with a cap the one-to-one blanking comes
 *      first and the cap's rule is applied to the blanked lists, where a blanked entry is invalid: it neither counts nor votes.
 *      With the flag clear the call issues the launches of before, in their order.  How: every entry gets the 64-bit key
 *      {sims mapped to an order-preserving uint32, ~p} and a hash table per query image ({id, best key} slots, two slots per
 *      entry, id claimed by compare-and-swap, key raised by a 64-bit max) selects each id's largest key; an entry keeps its id
 *      when its key is its slot's.  Launches added in front of the cap and the vote (stage "vote"): 1 when some query image has
 *      at most 4096 entries (S_b * k; one workgroup per image, the table in LDS), and 3 more -- a table fill, insert, resolve --
 *      when some image has more (the table in global scratch, agent-scope atomics; no grid barrier).  Scratch: the blanked copy,
 *      nq * k * 8 bytes, and for the larger images 32 bytes per entry of the rows from the first to the last of them.  Limit:
 *      the vote's, 2^24 entries per query image.  No synchronisation is added; idx and sims are read in the order of the
 *      context's stream; deterministic: two calls return the same bytes.                                                  */
#define SEGVLAD_VOTE_PER_IMAGE(m) ((m) << 8)
#define SEGVLAD_VOTE_UNIQUE_REF 0x80
int segvlad_vote(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg,
                 int64_t n_ref_seg, const int32_t* qseg_offsets, int n_img, int k, float smin, float smax, int n_top, int mode,
                 int32_t* pred_out, double* score_out);

/* ---- instrumentation: with profiling on, every kernel group of a stage ("incidence", "adjacency",
 *      "assign", "prep", "burst" (the kernels of the option vlad_burst: two under image scope, one under vlad_burst_scope=segment), "aggregate", "pca", "describe" (segvlad_describe as a whole: its parts overlap), "knn_level0", "knn_gemm", "knn_select", "knn_fallback", "knn_shortlist" (segvlad_search_shortlist), "knn_exclude" (the kernels segvlad_search_excluding adds to its inner search), "knn_group" (the kernels segvlad_search_grouped adds to its inner search), "knn_range" (the kernels of segvlad_range_search), "match_pairs" (segvlad_match_pairs), "verify_pairs" (segvlad_verify_pairs), "sequence_rerank" (segvlad_sequence_rerank), "incidence_rle", "rle_decode", "rle_encode" (the run-length entries), "mask_regions" (segvlad_mask_regions), "db_remove" (segvlad_db_remove), "vote") is bracketed by a HIP event pair
 *      on the context stream.  segvlad_stage_ms returns the SUM of the elapsed times (ms) and the number
 *      of kernel launches recorded for the stage since the last segvlad_profile_reset; it returns
 *      SEGVLAD_ERR_STATE if the stage has not run.  Replaces the (discarded) time.time() pair of
 *      vlad_matmuls_per_cluster, func_vpr.py:1185,1207-1210.                                          */
int segvlad_set_profiling(segvlad_ctx* ctx, int on);
int segvlad_profile_reset(segvlad_ctx* ctx);
int segvlad_stage_ms(segvlad_ctx* ctx, const char* stage, float* ms_out, int* launches_out);

/* ---- switches (no reference counterpart: the reference has one arithmetic, fp32/fp64 torch + faiss).
 *      Read ONCE: the environment variables SEGVLAD_KNN_FILTER / SEGVLAD_KNN_FP32 / SEGVLAD_PCA_FP32 / SEGVLAD_PCA_PATH /
 *      SEGVLAD_KNN_HEURISTIC / SEGVLAD_SEARCH_STATS give a context its defaults at segvlad_create; this call overrides them.
 *      No kNN switch changes a result (every filter is followed by the exact fp32 refinement: tests assert
 *      bit-equality); the PCA variants are all fp32-class and agree to ~1e-5 relative (tests hold each to the same
 *      oracle tolerance), not bit for bit.
 *        "knn_filter"   auto | f16 | bf16x3 | fp32     arithmetic of the candidate filter GEMM
 *        "pca_arith"    auto | f16x3 | fp32            projection GEMM arithmetic
 *        "search_stats" 0 | 1                          record list occupancies (segvlad_search_stats)
 *        "knn_heuristic" 1 | 0                         low-rank, a-posteriori verified level thresholds (5-10x fewer
 *                                                      candidates per level) | rigorous k-th-rank thresholds only
 *        "pca_path"      auto | planes | project       form of segvlad_images_pca when no descriptor output is asked
 *                                                      for: "planes" projects the finished K*D-wide descriptors,
 *                                                      "project" projects every token's residual with its cluster's
 *                                                      slice of the components and aggregates the segments in the
 *                                                      P-dimensional space (same fp32-class result, N*D*P instead of
 *                                                      S*K*D*P flops per image); auto = the smaller product, decided PER
 *                                                      CALL from the batch (tokens per cluster, segments): the same
 *                                                      image can therefore come out ~1e-5 relative apart in two batches
 *                                                      of different size -- fix the form when runs must be comparable
 *                                                      digit for digit (bench.py does)
 *        "small_plan"    1 | 0                         searches of <= 128 query rows (ONE query image per pass: the
 *                                                      HBM-bound regime of SURVEY 8d) take their own plan -- one filter
 *                                                      level behind an exact sample of 2048..4096 rows, a workgroup per
 *                                                      list in the selects, refinement lists shared by workgroups, the
 *                                                      query scale left on the device | the plan of the batches
 *        "query_group"   0 | 1 .. 64                   a HINT, never a result: the query rows of the coming batches are the
 *                                                      segments of query images, this many consecutive rows per image (0 =
 *                                                      unknown).  The exact level of a batch search re-evaluates the refine
 *                                                      bands of a group of rows -- an image's rows with the hint, 32-row
 *                                                      blocks without -- as ONE fp32 GEMM over the union of their database
 *                                                      rows when that is the cheaper way (the segments of an image share most
 *                                                      of their neighbours: a cost model with measured constants decides per
 *                                                      group), row by row otherwise
 *        "refine_group"  1 | 0 | 2                     that grouped refinement | every row on its own (rounds 1-4) | every group
 *                                                      whose union fits, whatever the cost model says (tests); same bits
 *        "vlad_assign"   hard | soft:<T> | soft_pooled:<T>
 *                                                      how a token is assigned to the centres (utilities.py:862-887, VLAD.generate's
 *                                                      vlad_mode / soft_temp).  hard (the default): every token goes to its
 *                                                      nearest centre; every call issues the launches and returns the bytes it
 *                                                      does without the option.  soft:<T>, T a decimal fp32 temperature, finite
 *                                                      and > 0: every token goes to EVERY centre.  With x^_n the L2-normalised
 *                                                      token n of the image, c_k the raw centre, c^_k its normalised copy and
 *                                                      U(s) the token set of segment s after the neighbour union (adj; identity
 *                                                      for order 0):
 *                                                        w[n][k] = softmax over the K real centres of T * <x^_n, c^_k>
 *                                                                  (max-subtracted; padded centres take no part)
 *                                                        V[s][k] = sum_{n in U(s)} w[n][k] x^_n - (sum_{n in U(s)} w[n][k]) c_k
 *                                                        out[s]  = L2( concat_k intra_norm(V[s][k]) )
 *                                                      intra_norm and L2 divide by max(norm, 1e-12) like the hard path, so a
 *                                                      segment that covers no token is a row of zeros and an all-zero block
 *                                                      stays zero.  soft_pooled:<T> has the same weights, normalisations and
 *                                                      outputs, and takes every block against ALL centres,
 *                                                        V[s][k] = sum_{n in U(s)} w[n][k] sum_c (x^_n - c_c)
 *                                                                = K sum_n w[n][k] x^_n - (sum_n w[n][k]) sum_c c_c
 *                                                      which is what VLAD.generate computes (utilities.py:883-884 sums the
 *                                                      weighted residuals over tokens and centres): with one all-token segment
 *                                                      per image and order 0 it is that function on normalised tokens, as aggFt
 *                                                      calls it.  soft:<T> tends to the hard descriptor as T grows, soft_pooled
 *                                                      does not.  Both cover segvlad_images, segvlad_images_pca, segvlad_describe
 *                                                      and segvlad_describe_begin / _end; labels_out and gap_out stay the hard
 *                                                      arg-max and the top-1 / top-2 gap, block_norms_out is ||V[s][k]|| of the
 *                                                      soft blocks.  Sums run in a fixed order without float atomics: two calls
 *                                                      return the same bytes and an image's rows do not depend on the rest of
 *                                                      the batch.  The "project" form of pca_path presupposes one cluster per
 *                                                      token: under soft, auto takes "planes" and an explicit project is
 *                                                      SEGVLAD_ERR_LIMIT.  segvlad_kmeans_step and segvlad_cluster_aggregate
 *                                                      ignore the option (hard by definition).  A missing, empty, non-positive,
 *                                                      non-finite or junk-trailed T and any other spelling are SEGVLAD_ERR_ARG
 *                                                      and leave the option as it was
 *        "vlad_burst"    off | <a>:<b>:<p>             burst discount: every token's assignment weight is divided by a soft
 *                                                      count of the tokens of ITS image that look like it (the aggregation of
 *                                                      VLAD-BuFF at its fixed test-time parameters, 8:7:1, with no training).
 *                                                      off (the default): every call issues the launches and returns the bytes
 *                                                      it does without the option.  a, b, p are decimal fp32 with
 *                                                      0 <= a <= 64, -8 <= b <= 16, 0 <= p <= 2.  For one image with tokens
 *                                                      x_0 .. x_{N-1} -- ALL N of them, whether a segment covers them or not --
 *                                                      and x^_n = x_n / max(||x_n||, 1e-12):
 *                                                        g[n] = sum_{m=0}^{N-1} sigmoid(a (2 <x^_n, x^_m> - 2) + b)    (m = n included)
 *                                                        u[n] = g[n]^-p
 *                                                      and every assignment weight is multiplied by u[n]: under vlad_assign=hard
 *                                                      w[n][k] = u[n] for k = label(n) and 0 otherwise, under soft:<T> and
 *                                                      soft_pooled:<T> w[n][k] = softmax_k(...) u[n]; V[s][k], intra_norm and the
 *                                                      row L2 are vlad_assign's formulas above with these weights.  g depends on
 *                                                      the image alone -- not on the segments, the adjacency or the rest of the
 *                                                      batch; an all-zero token has x^ = 0 and takes part with cosine 0.  Inside
 *                                                      the ranges g >= sigmoid(-8) and u <= 9e6, so no norm overflows fp32; with
 *                                                      p = 0, u is exactly 1.  labels_out and gap_out stay the hard arg-max and
 *                                                      gap, block_norms_out is ||V[s][k]|| with the discounted weights.  The
 *                                                      N x N similarities are fp32 (fp32 MFMA), exist one tile at a time in
 *                                                      registers, and are summed in a fixed order without float atomics: two
 *                                                      calls return the same bytes.  Covers segvlad_images, segvlad_images_pca,
 *                                                      segvlad_describe and segvlad_describe_begin / _end;
 *                                                      segvlad_kmeans_step and segvlad_cluster_aggregate ignore it.  Like soft
 *                                                      assignment it has no "project" form of pca_path (that form presupposes
 *                                                      unweighted one-cluster tokens): auto takes "planes", an explicit project
 *                                                      is SEGVLAD_ERR_LIMIT.  COST: hard assignment with the discount aggregates
 *                                                      from a one-hot weight buffer on the soft path's kernel, K times the hard
 *                                                      aggregation's matrix work (a label-grouped weighted aggregation is later
 *                                                      work).  A missing, non-finite, out-of-range or junk-trailed field and any
 *                                                      other spelling are SEGVLAD_ERR_ARG and leave the option as it was
 *        "vlad_burst_scope"  image | segment           over which tokens vlad_burst counts.  Read only while vlad_burst is on: with
 *                                                      vlad_burst=off the value is stored and changes neither bytes nor launches.
 *                                                      image (the default): the text above, all N tokens of the image, one weight
 *                                                      per token.  segment: the tokens that are aggregated with the token -- U(s),
 *                                                      the token set of segment s after the neighbour union -- so the discount is
 *                                                      a weight per (segment, token).  With x^_n the normalised token, c_k the raw
 *                                                      centre and w[n][k] vlad_assign's weight (the one-hot of the label, or the
 *                                                      softmax):
 *                                                        g[s][n] = sum_{m in U(s)} sigmoid(a (2 <x^_n, x^_m> - 2) + b)    n in U(s), m = n included
 *                                                        u[s][n] = g[s][n]^-p
 *                                                        V[s][k] = sum_{n in U(s)} u[s][n] w[n][k] (x^_n - c_k)
 *                                                        out[s]  = L2(concat_k intra_norm(V[s][k]))      both divide by max(norm, 1e-12)
 *                                                      (soft_pooled:<T>: K sum u w x^ - (sum u w) sum_c c_c, the formula above).
 *                                                      g depends on the image's tokens and on U(s) alone -- not on the other
 *                                                      segments, not on the rest of the batch.  With one all-token segment per
 *                                                      image and order 0 it is vlad_burst under image scope (NetVLAD.forward's
 *                                                      w_burst).  With p = 0, u is exactly 1.  A token with non-zero x^ has
 *                                                      g >= sigmoid(b) (its own term); an all-zero token takes part with cosine 0,
 *                                                      as under image scope.  labels_out and gap_out stay the hard arg-max and
 *                                                      gap, block_norms_out is ||V[s][k]||.  The similarities are fp32 (fp32 MFMA),
 *                                                      exist one tile at a time in registers, and every sum runs in a fixed order
 *                                                      (the image's tokens grouped by label) without float atomics: two calls
 *                                                      return the same bytes.  Covers segvlad_images, segvlad_images_pca,
 *                                                      segvlad_describe and segvlad_describe_begin / _end; segvlad_kmeans_step and
 *                                                      segvlad_cluster_aggregate ignore it.  pca_path: auto takes "planes", an
 *                                                      explicit project is SEGVLAD_ERR_LIMIT (naming vlad_burst), as under image
 *                                                      scope.  COST: the self-similarity runs as the full square, twice the image
 *                                                      scope's flops, once per 64 segments of the image; hard assignment
 *                                                      aggregates over label k's tokens for cluster k, the hard
 *                                                      aggregation's matrix work, with no weight buffer.  Any other spelling is
 *                                                      SEGVLAD_ERR_ARG and leaves the option as it was
 *      Every other key is a DEVELOPMENT switch (kernel tuning, A/B variants, debugging, the tests' own hooks), documented in
 *      revisit-anything_amd/csrc/segvlad_dev.h and NOT part of this ABI: none changes a result, the shipped library holds
 *      only the kernels they default to and rejects the values that select another (SEGVLAD_ERR_ARG).
 *
 *      Environment, read ONCE by segvlad_create: SEGVLAD_GUARD=1 creates a GUARDED context (development / test runs):
 *      every device buffer of the context is allocated at its exact size between two fences of poison words, the back
 *      fence of a per-call scratch buffer right behind the bytes of the CURRENT request, and every call -- and
 *      segvlad_synchronize -- ends with a check of all fences: an out-of-bounds write fails the call with
 *      SEGVLAD_ERR_STATE and names the buffer.  (The library's scratch only ever grows; without the guard a request that
 *      an earlier, larger one already covers cannot fail.)  Results are unchanged; calls synchronise the device. */
int segvlad_set_option(segvlad_ctx* ctx, const char* key, const char* value);

/* ---- statistics of the last segvlad_search on this context (HOST array, up to 13 values):
 *      [0] filter levels run after the sampled exact level (0 = distance-matrix path)
 *      [1] filter arithmetic used (0 none, 1 f16, 2 bf16x3, 3 fp32)
 *      [2] query rows whose candidate list overflowed and that were redone, as one dense batch, on the
 *          exact distance-matrix path (the other rows keep their filtered result)
 *      [3] max and [4] sum of the last level's candidate-list lengths   (option search_stats = 1)
 *      [5] max and [6] sum of the exact-refinement list lengths         (option search_stats = 1)
 *      [7] number of query rows
 *      [8] query rows whose low-rank ("heuristic") level thresholds did not verify and that were redone
 *          with the rigorous k-th-rank thresholds (option knn_heuristic = 0 disables the low-rank thresholds)
 *      [9] query rows whose refine band held more rows than the first-tier list (512) and that were refined
 *          from their whole candidate list instead (second tier; temporally redundant databases)
 *      [10] groups of 32 consecutive query rows whose refine bands overlapped enough to be evaluated as one exact fp32 GEMM over
 *           the union of their rows, and [11] the sum of those unions' lengths            (option search_stats = 1)
 *      [12] database rows the last filter level did not evaluate again: the rows of the stride-16 level, whose survivors stayed in
 *           the candidate lists (0: every level started from empty lists)                                                         */
int segvlad_search_stats(segvlad_ctx* ctx, int64_t* stats_out, int n);

/* ---- row-sharded index over the GPUs of a node: one process (and one context) per GPU.
 *      No reference counterpart -- the reference is single-process (place_rec_main.py:53-60 builds ONE faiss index);
 *      this is SURVEY 8b/8e's own layer: rank r adds the rows [base_r, base_r + n_r) of the reference-segment matrix to
 *      ITS context (segvlad_db_add), every rank searches the full query batch against its shard, the per-shard top-k
 *      lists travel in ONE all-gather of packed 12-byte records {fp32 distance bits, int64 global id} over RCCL (xGMI
 *      inside a node), and every rank merges them -- by distance, ties by lower global id: bit for bit what one index
 *      over all rows returns.  RCCL is bound at run time (dlopen; a copy already in the process -- PyTorch-ROCm's -- is
 *      shared): without it these calls return SEGVLAD_ERR_COMM and everything else keeps working.
 *
 *      segvlad_comm_unique_id   rank 0 draws the 128-byte id (HOST); it reaches the other ranks by any host channel
 *                               (MPI, a file, torch.distributed's store ...)
 *      segvlad_comm_init        collective over all ranks: binds an RCCL communicator to the context (its stream carries
 *                               the collectives); world = 1 is valid
 *      segvlad_comm_info        rank / world of the context's communicator (world 0 = none) and which RCCL was bound
 *      segvlad_allgather_rows   [n_local][d] fp32 of every rank -> [world * n_local][d], rank order (equal slices): the
 *                               query descriptors when every rank describes a slice of the query images
 *      segvlad_search_sharded   global exact top-k (ascending (d2, id); (inf, -1) beyond the total row count), identical
 *                               on every rank.  id_base = global index of this shard's first row.  Collective: every
 *                               rank enters the all-gather or none does -- a rank whose LOCAL search fails still
 *                               contributes ((inf, -1) records and its status in a trailer record), and then EVERY rank
 *                               returns an error (the failing rank its own, the others SEGVLAD_ERR_COMM naming it); a
 *                               rank that cannot join any more (no memory for the exchange buffers) aborts the
 *                               communicator (ncclCommAbort) instead of leaving its peers waiting.
 *      segvlad_allgather_rows   n_local must be the same on every rank. */
#define SEGVLAD_COMM_ID_BYTES 128
int segvlad_comm_unique_id(void* id_out);
int segvlad_comm_init(segvlad_ctx* ctx, const void* id, int rank, int world);
int segvlad_comm_destroy(segvlad_ctx* ctx);
int segvlad_comm_info(segvlad_ctx* ctx, int* rank_out, int* world_out, char* origin_out, int origin_len);
int segvlad_allgather_rows(segvlad_ctx* ctx, const float* local_rows, int n_local, int d, float* all_rows);
int segvlad_search_sharded(segvlad_ctx* ctx, const float* Q, int nq, int k, int64_t id_base, float* d2_out, int64_t* idx_out);

/* ---- query-sharded retrieval over a REPLICATED index: every rank adds the whole reference matrix to its context and
 *      searches and votes only ITS OWN query images (contiguous blocks: an image's segments never straddle ranks).
 *      The only step that crosses ranks before the predictions is the vote's normalisation: func_vpr.py:211-214 divides by
 *      the GLOBAL max - min over all kept similarities of the whole query set, and since a reference image's score is
 *      (sum s - n min) / (max - min) with n differing between images, per-rank extrema would change the ORDER of the
 *      predictions, not only their scale.
 *
 *      segvlad_vote_global      segvlad_vote's contract over this rank's query images, with the extrema taken over
 *                               the similarities of ALL ranks (no smin / smax arguments).  Collective: each rank
 *                               reduces its own min / max on the device (a rank without query segments contributes
 *                               (+inf, -inf)), ONE ncclAllGather exchanges a 16-byte record per rank {min bits, max bits,
 *                               local status, query segments}, and a one-wave kernel reduces the records in place on
 *                               the context stream; the vote reads the result from device memory.  min / max are exact,
 *                               so the extrema -- and the votes -- are bit for bit what one process computes over all
 *                               similarities, whatever the rank order.  Failure semantics of segvlad_search_sharded: a
 *                               rank whose local step fails (arguments included) still joins with its status in its
 *                               record, then every rank returns an error (the failing rank its own, the others
 *                               SEGVLAD_ERR_COMM naming it) and the communicator stays usable; a rank that cannot join
 *                               aborts the communicator.  Mode COUNT needs no extrema but stays collective; mode takes
 *                               segvlad_vote's SEGVLAD_VOTE_PER_IMAGE and SEGVLAD_VOTE_UNIQUE_REF bits (each rank blanks
 *                               its own rows).  No communicator bound: exactly segvlad_vote with NaN extrema.  Synchronises
 *                               the stream.
 *      Gathering the predictions in image order: segvlad_allgather_rows, a byte-exact copy.  Each rank packs its images
 *      as rows of 3 * n_top 32-bit words {pred int32 [n_top], score fp64 bits [n_top]} viewed as fp32, padded to the
 *      largest rank's image count (n_local must be equal on every rank); fp64 scores arrive bit for bit.           */
int segvlad_vote_global(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg,
                        int64_t n_ref_seg, const int32_t* qseg_offsets, int n_img, int k, int n_top, int mode,
                        int32_t* pred_out, double* score_out);

#ifdef __cplusplus
}
#endif
#endif /* SEGVLAD_H */
