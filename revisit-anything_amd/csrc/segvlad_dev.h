/*
 * segvlad_dev.h -- DEVELOPMENT switches of libsegvlad_hip.so (segvlad_set_option keys that are NOT part of the ABI declared in
 * include/segvlad.h).  Nothing here changes a result: every kNN switch is followed by the exact fp32 refinement
 * (tests/test_gpu_filter_variants.py holds each variant to the bits of the all-fp32 filter), the VLAD / PCA switches select
 * kernels that agree to ~1e-6 relative (tests/test_gpu_parity.py).
 *
 * Builds.  The SHIPPED library (revisit-anything_amd/build.py; lib/libsegvlad_hip.so) and the DEVELOPMENT build
 * (`python revisit-anything_amd/build.py --ablations`, -DSEGVLAD_ABLATIONS -> lib/libsegvlad_hip_abl.so, loaded with
 * SEGVLAD_LIB_PATH) hold the same kernels; the development build adds three probes of the batch filter kernel (f16_cfg 93:
 * phase timing; 94 / 95: timing ablations with WRONG results) and nothing else.  A value that names no kernel of the build is
 * rejected with SEGVLAD_ERR_ARG.  (The fp16 filter's measured-and-not-kept variants -- "f16_mf", "f16_epi", "f16_pp", "f16_dsplit",
 * "f16_small_mf", f16_deep_cfg 0 - 3, f16_buf 1, the other f16_cfg values -- left the tree; DESIGN.md 4 / 7 has their
 * measurements and names the commit that last held them.)
 *
 *   fp16 candidate filter of the exact kNN (knn_filter_kernels.hip: sv_choose_f16_kernel)           accepted values
 *     "f16_cfg"       kernel family; -1 = from the shape: 250 batches, 300 deep rows (d >= 4096), 62 / 63 one query
 *                     image per pass                                                             -1, 250, 300, 62, 63
 *                     development build: 93 = phase timing of the batch kernel, 94 = no epilogue, 95 = no epilogue and
 *                     no DMA in the k-loop                                                       + 93, 94, 95
 *     "f16_deep_cfg"  deep rows: -1 / 5 = the persistent batch kernel with flushed blocks where the launch fills it, 4
 *                     elsewhere; 4 = 256 x 128 tiles, 8 waves, 16 x 16 x 32, a second accumulator set   -1, 4, 5
 *     "f16_buf"       operand DMA of the register-blocked deep-row kernel as buffer_load ... lds: -1 = yes, 0 = no   -1, 0
 *     "f16_walk"      tile walk of the persistent kernel: bit 0 = an XCD keeps its block of query tiles, bit 1 = odd steps run
 *                     their k-tiles backwards, bit 2 = rotated k start per workgroup (-1 = 3)    any (a launch parameter)
 *     "f16_gm"        tile-block height of the XCD-aware order                                    any (a launch parameter)
 *   fused VLAD -> PCA (assign_kernels.hip, vlad_kernels.hip, block_norm_kernels.hip, project_kernels.hip, gemm_f16x3_kernels.hip)
 *     "tnk_gram"      1 | 0   block norms from the Gram matrix of a task's residuals (16-bit matrix pipe) | fp32 block sums
 *     "tnk_fork"      1 | 0   the two-tile Gram launch on the context's side stream | in line
 *     "pj_f16"        1 | 0   P-space tile sums on the 16-bit matrix pipe | fp32 MFMA
 *     "pj_nw"         8 | 4   waves per workgroup of the P-space aggregation
 *     "pj_planes"     1 | 0   project form, 16-bit tile sums: the grouped GEMM stores z * zscale as its fp16 pair (h | l << 16) where the
 *                             fp32 z stood, the aggregation takes the pairs from registers, three tiles in flight (same bits:
 *                             tests/test_gpu_pj_planes.py) | fp32 Z staged in LDS and split in every tile
 *     "cover_rows"    1 | 0   project form: only the tokens that some segment covers get a row of the grouped planes and of Z
 *                             (same bits: tests/test_gpu_cover_rows.py) | every token gets a row
 *     "x3_tile", "x3_gm", "agg_kpb", "assign_narrow"   tile / order / geometry of the projection GEMM, the descriptor
 *                     aggregation and the assignment kernel
 *     "f16_persist_wgs" 1..32 resident workgroups per XCD of the persistent batch filter (32 = every CU; fewer leave CUs to other streams)
 *     "level_carry"   1 | 0   batch searches (guessed thresholds): the last filter level skips the rows of the stride-16 level, whose
 *                             survivors stay in the candidate lists | every level from empty lists over all of its rows
 *     "batch_l0_f16"  1 | 0   batch searches (guessed thresholds): the sampled level from the filter's own fp16 product | the exact fp32 GEMM
 *                             (2: deep rows through sample_f16_batch_kernel instead of the filter kernel under +inf thresholds, A/B)
 *   single-image passes (small_pass_kernels.hip)
 *     "small_head"    1 | 0 | 3   the pass starts with small_head_kernel: plane, scale, norms, flags and the sample thresholds (from the
 *                     filter's own fp16 product) in one launch | query preparation -> exact fp32 sample level -> reduce + rank |
 *                     the same kernel with the query block loaded straight in MFMA fragment shape (measured slower: 22.7 vs 21 us)
 *     "small_tail"    1 | 2 | 0   no read-back, no host synchronisation in segvlad_search: flagged rows are finished on the DEVICE -- by the
 *                     refinement kernel's own workgroups where the shared-list refinement runs behind small_head_kernel (no extra launch),
 *                     else by small_tail_kernel, launched behind every pass | always small_tail_kernel | the read-back of rounds 3-5
 *   debugging and the tests' own hooks
 *     "debug_small_tail"   bit 0: every row of a device-driven pass is flagged for the exact brute force; bit 1: every row is sent through
 *                          the second tier; bit 2: the checked hand-over's sticky word is raised; bit 3: query row 1's hand-over is treated
 *                          as failed (the fused finish recomputes the band); bits 8..: grid of small_tail_kernel (A/B)
 *     "debug_search"       1 = per-level candidate statistics on stderr (synchronises); 7 = the Gram kernel waits for every
 *                          outstanding memory operation at every step (verification of its counted waits)
 *     "group_fetch"        segvlad_search_grouped: depth of the inner search, clamped to k .. 1024 (0 = min(1024, 4 k)); the tests reach
 *                          the exact tail on a small index with it
 *     "debug_fail_search"  segvlad_search fails at once (the sharded entry's error path)
 *     "guard_undersize"    "<buffer>:<bytes>": guard-mode tests (include/segvlad.h, SEGVLAD_GUARD)
 *   Environment read once by segvlad_create for these: SEGVLAD_F16_CFG, SEGVLAD_F16_GM, SEGVLAD_X3_TILE, SEGVLAD_X3_GM,
 *   SEGVLAD_ASSIGN_NARROW, SEGVLAD_DEBUG_SEARCH, SEGVLAD_AGG_KPB, SEGVLAD_COVER_ROWS.
 */
#ifndef SEGVLAD_DEV_H
#define SEGVLAD_DEV_H
#include "../../include/segvlad.h"
#endif
