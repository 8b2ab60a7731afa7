// Context, scratch management and launch declarations shared by the SegVLAD HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/segvlad.h"

#define SV_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      return ctx->fail(SEGVLAD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                       __FILE__, __LINE__);                                                       \
    }                                                                                             \
  } while (0)

#define SV_TRY(expr)          \
  do {                        \
    int _r = (expr);          \
    if (_r != SEGVLAD_OK) return _r; \
  } while (0)

// squared L2 distance from the norms and the dot product; ONE definition so that every path (matrix GEMM,
// filtered GEMM, exact refinement) rounds identically: fma(-2, dot, ||q||^2 + ||r||^2), negative results set to zero --
// faiss's IndexFlatL2 (1.7.3, utils/distances.cpp, exhaustive_L2sqr_blas: `if (dis < 0) dis = 0`, "negative values can occur
// for identical vectors due to roundoff errors") does the same BEFORE its heap sees the value, so an exact duplicate is at
// distance 0 and `2 - d2` (place_rec_main.py:78-81) never exceeds 2 (round 6).  max(0, .) is monotone and 1-Lipschitz: order
// statistics and the filters' margins |d2~ - d2| <= eps carry over to the clamped values unchanged.
// A NaN (a row or a query holding NaN / Inf) leaves here as +inf: every select orders the values by their bit patterns
// (f2key), where a NaN with the sign bit set -- what 0/0 gives -- would sort in FRONT of 0.0 and take the first slot of every
// list.  As +inf such a pair sorts last with the other pairs that are never listed (segvlad.h, "Non-finite rows"); finite
// values keep their bits.
#if defined(__HIPCC__)
__device__ __forceinline__ float sv_d2(float q2, float r2, float dot) {
  const float v = __fmaf_rn(-2.f, dot, q2 + r2);
  return v < 0.f ? 0.f : (v == v ? v : INFINITY);
}
// The same value with a NaN left a NaN, for the 16-bit filters' epilogues alone: they compare the value with a threshold (false for a
// NaN: never a candidate) and never order it.
__device__ __forceinline__ float sv_d2_screen(float q2, float r2, float dot) {
  const float v = __fmaf_rn(-2.f, dot, q2 + r2);
  return v < 0.f ? 0.f : v;
}
#endif

// Layout of the fp16 operand planes of the split projection GEMM (gemm_f16x3_kernel): [row / 128][k / 32][128 rows][32 k],
// the four 16-byte chunks of a row stored at chunk ^ sv_x3_swz(row).  One (128-row, 32-k) block is 8 KiB of CONTIGUOUS
// memory that is, byte for byte, the bank-conflict-free LDS image the MFMA fragment reads expect: the global->LDS DMA
// of a k-tile is a linear copy of whole 128-byte lines.  (Row-major planes made every DMA piece touch 16 half-lines
// 196 KiB apart; each line was fetched twice, one k-tile apart, and the XCD's L2 -- 4 MiB against 4 MiB of such
// half-used lines in flight -- kept nothing for the workgroups sharing a tile: 26 GB fetched for 4.4 GB of operands.)
// Rows are padded to a multiple of 256 (the pad rows hold garbage: they only feed output rows / columns that are never stored).
//
// The swizzle term.  The fragments are read for v_mfma_f32_16x16x32_f16 (round 4: the shape that needs less energy per flop):
// lane l holds row (l & 15) of a 16-row tile and chunk (l >> 4) of the 64-byte row.  A ds_read_b128 is served in four groups of
// 16 lanes, {0-3, 12-15, 20-27} being one: rows 0-3 and 12-15 with chunk c, rows 4-11 with chunk c + 1; bank group (16-byte
// unit mod 16) of row r, physical chunk p = 4 (r & 3) + p.  With p = c ^ a[(r >> 2) & 3] the sixteen lanes of every group hit
// sixteen different bank groups iff {a0, a3, 1 ^ a1, 1 ^ a2} and {a1, a2, 1 ^ a0, 1 ^ a3} are both {0, 1, 2, 3}:
// a = (0, 3, 2, 1), i.e. (-(r >> 2)) & 3.  (Rounds 1-3 read 32-row fragments -- lane l: row l & 31, chunk l >> 5 -- for which
// a = (0, 1, 2, 3) was the conflict-free choice; that one is 2-way conflicted for the 16-row pattern.)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int sv_x3_swz(int64_t row) { return (int)((0 - (row >> 2)) & 3); }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t sv_x3_off(int64_t row, int64_t k, int64_t Kd) {
  return ((size_t)(row >> 7) * (size_t)(Kd >> 5) + (size_t)(k >> 5)) * 4096 + (size_t)(row & 127) * 32 +
         (size_t)((((k & 31) >> 3) ^ sv_x3_swz(row)) << 3) + (size_t)(k & 7);
}
inline int64_t sv_x3_rows(int64_t n) { return (n + 255) & ~255ll; }
// the power-of-two scale of an fp16 split: 2^(14 - e) for a finite bound > 0 in [2^(e-1), 2^e), so that bound * scale < 2^15
inline float sv_fp16_scale(float bound) {
  int e;
  frexpf(bound, &e);
  return ldexpf(1.f, 14 - e);
}

// grow-only device buffer
//
// Guard mode (SEGVLAD_GUARD=1 at segvlad_create; development / test runs): every buffer sits between two fences of
// SV_GUARD_BYTES poison bytes.  A grow-only buffer hides under-sized requests -- a request that an earlier, larger one
// already covers never fails (round 3 found a real out-of-bounds write that way, only on a fresh context) -- so in guard
// mode the BACK fence of a per-call scratch buffer sits right behind the bytes of the CURRENT request (re-placed by every
// reserve(), after a device synchronisation), and every API call ends with a check of all fences (sv_finish;
// segvlad_synchronize): a trampled fence fails the call with SEGVLAD_ERR_STATE and names the buffer.  Buffers whose
// contents outlive a call (`fixed`: database, models, the refinement's hand-over words) keep their back fence at the end
// of the allocation.
constexpr size_t SV_GUARD_BYTES = 1024;
constexpr uint32_t SV_GUARD_WORD = 0xA5C3F00Du;
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;          // usable bytes behind p
  const char* tag = "";
  bool guard = false;      // set by segvlad_create for every buffer of a guarded context
  bool fixed = false;      // guard mode: contents persist across calls -> the back fence stays at p + cap
  void* raw = nullptr;     // guard mode: the allocation (front fence | cap bytes | back fence)
  size_t req = 0;          // guard mode: bytes of the current request (the back fence starts at p + round_up(req, 4))
  int shrink = 0;          // guard mode, tests only (option "guard_undersize"): the fence is placed `shrink` bytes EARLY
  hipError_t reserve(size_t bytes) {
    if (guard) return reserve_guarded(bytes);
    if (bytes <= cap) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return e;
    cap = want;
    return hipSuccess;
  }
  hipError_t reserve_guarded(size_t bytes);   // api.hip
  size_t fence_off() const { return fixed ? cap : ((req > (size_t)shrink ? req - (size_t)shrink : 0) + 3) & ~(size_t)3; }
  void release() {
    if (raw) (void)hipFree(raw);
    else if (p) (void)hipFree(p);
    raw = nullptr;
    p = nullptr;
    cap = 0;
    req = 0;
  }
  template <class T>
  T* as() { return reinterpret_cast<T*>(p); }
};

// Accumulating stage timer: every StageScope records one (start, stop) event pair on the context
// stream; segvlad_stage_ms() sums the elapsed times of all pairs recorded since the last
// segvlad_profile_reset() (events are resolved lazily, nothing synchronises while timing).
struct StageTimer {
  std::vector<hipEvent_t> ev;  // pairs: ev[2i], ev[2i+1]
  int used = 0;                // number of pairs in use
  int launches = 0;
};

// Tuning / arithmetic switches.  Read ONCE (environment at segvlad_create, then segvlad_set_option); the hot
// entry points never call getenv.
struct SvOptions {
  int knn_filter = 0;     // 0 auto (fp16 when d % 64 == 0, else bf16x3 when d % 32 == 0, else fp32), 1 f16, 2 bf16x3, 3 fp32
  int pca_fp32 = 0;       // 1: plain fp32-MFMA projection instead of the fp16x3 split GEMM
  int f16_cfg = -1;       // kNN fp16 filter tile configuration (-1 = chosen from the shape)
  int f16_gm = -1;        // tile-block height of the XCD-aware order (-1 = by the number of query tiles, 0 = plain tm-fastest order)
  int f16_walk = -1;      // tile walk of the persistent fp16 filter: bit 0 = an XCD keeps its block of query tiles while it steps
                          // through the database blocks, bit 1 = odd steps run their k-tiles backwards (-1 = default = 3, see
                          // launch_f16_filter); never changes a result
  int f16_persist_wgs = 32;   // resident workgroups per XCD of the persistent batch filter (1 .. 32): fewer leave CUs free for the whole
                          // launch to kernels of OTHER streams (the next batch's describe stage, bench.py --pipeline); never changes a result
  int f16_deep_cfg = -1;  // deep rows (blocked accumulation): -1 / 5 = the persistent 256 x 256 ping-pong kernel with blocks flushed to a global
                          // scratch where the launch fills it (>= 1024 tiles), 4 elsewhere; 4 = 8 waves of 64 x 64 on 256 x 128 tiles, 16 x 16 x 32 MFMA, plain loop
                          // (sv_choose_f16_kernel)
  int f16_buf = -1;       // operand DMA of the register-blocked deep-row kernel as buffer_load ... lds (measured faster there): -1 = yes, 0 = no
  int tnk_gram = 1;       // fused VLAD -> PCA, project form: block norms of tasks with <= 64 tokens from their Gram matrix on the
                          // 16-bit matrix pipe (gram_norms_kernel); 0 = the fp32 block sums for every task
  int tnk_fork = 1;       // the two-tile Gram kernel on the context's side stream, beside the one-tile kernel (0: one after the other)
  int x3_tile = 0;        // PCA split GEMM tile (0 = from the shape, 128, 256)
  int x3_gm = -1;         // PCA split GEMM XCD-aware block height (-1 = default of the kernel, 0 = plain order)
  int search_stats = 0;   // 1: segvlad_search records list occupancies (synchronises once per chunk)
  int knn_heuristic = 1;  // 1: low-rank (verified) thresholds in the level scheme; 0: rigorous k-th-rank thresholds only
  int assign_narrow = 0;  // 1: force the narrow assignment kernel
  int agg_kpb = 4;        // clusters per aggregation workgroup
  int debug_fail_search = 0;   // tests only: 1 = segvlad_search fails at once (SEGVLAD_ERR_STATE) -- the sharded entry's error path;
                               // 2 = segvlad_search_sharded fails BEHIND its local search, where it can only abort the communicator
  int debug_search = 0;   // 1: print per-level candidate statistics to stderr (synchronises); 7: token_norms_kernel waits for every
                          //    outstanding memory operation at every step (verification of its counted waits: same bits)
  int debug_small_tail = 0;   // tests only: bit 0 = every row of a device-driven pass is flagged for the tail's brute force, bit 1 = every
                              // row's band is sent to its second tier, bit 2 = the hand-over's sticky failure word is raised
  int batch_l0_f16 = 1;   // batch searches on the fp16 filter with guessed thresholds: the sampled level from the filter's own fp16 product
                          // (deep rows: through the filter kernel itself under +inf thresholds; 2 = the sample kernel there too, A/B)
                          // (sample_f16_batch_kernel) instead of the exact fp32 GEMM; 0 = rounds 2-5
  int level_carry = 1;    // batch searches, guessed thresholds, fp16 filter: the last level runs over the rows the stride-16 level has not
                          // seen and that level's survivors stay in the candidate lists (1/16 of the full-level GEMM saved); 0 = every
                          // level starts from empty lists and the last one covers every row (rounds 2-6a)
  int small_head = 1;     // single-image passes start with small_head_kernel (plane + scale + norms + flags + sample thresholds in one
                          // launch); 0 = query preparation -> exact sample level -> reduce + rank (rounds 3-5)
  int small_tail = 1;     // single-image passes end in small_tail_kernel (no read-back); 0 = the read-back of rounds 3-5
  int small_plan = 1;     // <= 128 queries (one query image per pass): one filter level behind an exact sample of 2048..4096
                          // rows (see plan_search, search.hip); 0 = the deep plan of the batches
  int pj_f16 = 1;         // P-space aggregation: the tile sums on the 16-bit matrix pipe (0: fp32 MFMA, as before round 4)
  int pj_nw = 8;          // waves (32-column slices) per workgroup of the P-space aggregation: 8, or 4 (three workgroups per
                          // CU instead of one: measured SLOWER, 3.72 vs 3.40 ms for the PCA stage of 200 images)
  int refine_group = 1;   // batch searches: the refine bands of 32 consecutive query rows evaluated as ONE exact fp32 GEMM over the union of
                          // their rows when that is cheaper (refine_group_kernels.hip); 0 = every row on its own (rounds 1-4); 2 = every group whose union
                          // fits, whatever the cost model says (tests)
  int query_group = 0;    // hint: the query rows of a batch come in runs of this many rows per query image (1 .. 64; else unknown):
                          // the grouped refinement then takes an image's rows as one group instead of 32-row blocks
  int pca_path = 0;       // fused images_pca: 0 auto, 1 "planes" (descriptor planes x W), 2 "project" (project tokens, then aggregate)
  int cover_rows = 1;     // project form: only the tokens some segment covers get a row of the grouped planes and of Z (prep_kernel's
                          // `phys` map; same bits: every kernel keeps its logical positions); 0 = every token gets a row
  int pj_planes = 1;      // project form, 16-bit tile sums: the grouped GEMM's epilogue stores z * zscale as its fp16 pair (h | l << 16) in
                          // place of the fp32 z and the aggregation consumes the pairs from registers (same bits:
                          // tests/test_gpu_pj_planes.py); 0 = fp32 Z, split again in every tile
  float vlad_soft_temp = 0.f;   // "vlad_assign": 0 = hard; > 0 = soft assignment at this temperature (soft_vlad_kernels.hip)
  int vlad_soft_pooled = 0;     // "vlad_assign" = soft_pooled:<T>: every block's residuals are taken against ALL centres (the reference's sum)
  int vlad_burst = 0;           // "vlad_burst": 0 = off; 1 = every assignment weight times u[n] = g[n]^-p (burst_kernels.hip)
  float burst_a = 0.f, burst_b = 0.f, burst_p = 0.f;   // ... g[n] = sum_m sigmoid(a (2 cos(x_n, x_m) - 2) + b) over the image's tokens
  int burst_segment = 0;        // "vlad_burst_scope": 0 = image (the sum runs over the image's N tokens); 1 = segment (over the tokens of
                                // U(s): a weight per (segment, token), burst_seg_kernels.hip).  Read only while vlad_burst is on
  int group_fetch = 0;    // segvlad_search_grouped: depth of the inner search, clamped to k .. 1024 (0 = min(1024, 4 k)); never changes a
                          // result, only which rows the exact tail finishes (tests reach the tail on a small index with it)
};

// fp16 filter of the exact kNN: length of the accumulation blocks (0 = one running fp32 accumulator over the whole row).
// Rows of d >= 4096 (raw K*D descriptors) take the blocked kernel (option f16_cfg = 300 forces it for any d, any other
// explicit f16_cfg switches it off); the error constant below must describe the kernel that actually runs.
constexpr int SV_F16_KBLOCK = 1024;
inline int sv_f16_kblock(const SvOptions& o, int d) {
  if (o.f16_cfg == 300) return SV_F16_KBLOCK;
  return (o.f16_cfg < 0 && d >= 4096) ? SV_F16_KBLOCK : 0;
}
// Deep rows, default geometry (f16_deep_cfg -1 / 5): launches that fill the persistent 256 x 256 kernel run it with blocks of
// SV_F16_KFLUSH k-tiles of 64 flushed into a global scratch (knn_f16_filter_kernel, KFL) -- the block length the error constant
// of a search has to cover (the smaller levels run the register-blocked kernel, whose bound is smaller).
constexpr int SV_F16_KFLUSH = 64;
int sv_f16_eps_kblock(const SvOptions& o, int d);   // knn_filter_kernels.hip: from the configuration of the kernel that runs
// May a search of nq query rows take a biased-accumulator kernel (batches on the default configurations)?  Then it reads back
// min ||q||^2 with the scale: the bias enters the margin (sv_f16_c_eps, bias_mult).
inline bool sv_f16_bias_possible(const SvOptions& o, int64_t nq) { return nq > 128 && (o.f16_cfg < 0 || o.f16_cfg == 250 || o.f16_cfg == 300); }
// The kernels of the fp16 filter (knn_filter_kernels.hip holds one configuration type per name) and the rule that picks one
// for a launch: sv_launch_f16_filter, sv_f16_filter_skip_ok and sv_f16_eps_kblock all ask sv_choose_f16_kernel.
enum class F16Kernel {
  None, BatchDefault, BatchComplement, BatchSmall, BatchUnbiased, BatchUnbiasedSmall, DeepFlush, DeepFlushComplement, DeepBlockedBuf, DeepBlocked,
  DeepBlockedBufComplement, DeepBlockedComplement, DeepUnbiased, OneImage64, OneImage128,
#ifdef SEGVLAD_ABLATIONS
  ProbePhases, ProbeNoEpilogue, ProbeNoEpilogueNoDma,
#endif
};
struct F16Choice {
  F16Kernel kernel;
  const char* why;   // kernel == None: the reason
};
// M x n_rows: the launch; skip = 16: over the complement of the stride-16 sample; bias_ok: segvlad_ctx::f16_bias_ok of the search
F16Choice sv_choose_f16_kernel(const SvOptions& o, bool bias_ok, int M, int64_t n_rows, int d, int b_stride, int skip);
// |d2~ - d2| <= sv_f16_c_eps * ||q|| * ||r|| for the single-product fp16 filter (25 % slack included):
//   2^-10        both operands rounded to fp16 (relative 2^-11 each; products of two fp16 are exact in fp32),
//   2^-22        power-of-two scaling, sub-normal operands, second-order terms,
//   accumulation one running accumulator: <= 2 roundings per product, 2 d 2^-24;
//                blocked (kb > 0): 2 kb 2^-24 inside a block -- whatever order the matrix pipe sums a k-step in -- plus
//                (d / kb + 1) 2^-24 for the fp32 additions of the block sums,
//                relative to the largest running magnitude: sum_i |q_i r_i| <= ||q|| ||r||.  The batch kernels' BIAS starts
//                the accumulators at -||r||^2 / 2, so the running magnitude is <= ||q|| ||r|| + ||r||^2 / 2
//                <= bias_mult ||q|| max||r|| with bias_mult = 1 + max||r|| / (2 min||q||) over the query batch (1.5 for unit
//                vectors; prepare_queries (search.hip) measures it and keeps the unbiased kernel when it exceeds 5); bias_mult = 1 without;
// the factor 2 turns the error of the dot product into that of d2.
inline float sv_f16_c_eps(int d, int kb, float bias_mult) {
  const float acc = kb > 0 ? (2.f * (float)kb + (float)((d + kb - 1) / kb) + 1.f) / 16777216.f : 2.f * (float)d / 16777216.f;
  return 2.5f * (1.f / 1024.f + 1.f / 4194304.f + bias_mult * acc);
}

// statistics of the last segvlad_search (segvlad_search_stats)
struct SvSearchStats {
  int64_t levels = 0;           // filter levels after the sampled exact level (0 = matrix path)
  int64_t filter = 0;           // arithmetic of the filter levels: 0 none, 1 f16, 2 bf16x3, 3 fp32
  int64_t n_fallback = 0;       // query rows redone on the exact matrix path (list overflow)
  int64_t cand_max = 0;         // largest candidate list of the LAST level (search_stats only)
  int64_t cand_sum = 0;         // sum of the last level's candidate-list lengths (search_stats only)
  int64_t refine_max = 0;       // largest refine list (search_stats only)
  int64_t refine_sum = 0;       // sum of refine-list lengths (search_stats only)
  int64_t n_queries = 0;
  int64_t n_redo = 0;           // query rows whose heuristic thresholds did not verify and that were redone rigorously
  int64_t n_refine2 = 0;        // query rows whose refine band exceeded the first-tier list (SV_RCAP) and took the second tier
  int64_t grp_groups = 0;       // groups of 32 query rows whose bands were refined over the union of their rows (search_stats only)
  int64_t grp_union_sum = 0;    // sum of those unions' lengths (search_stats only)
  int64_t carry_rows = 0;       // database rows the last filter level did not compute again (taken over from the stride-16 level: level_carry)
};

// An open describe (describe.hip): set by segvlad_describe_begin, cleared by close_describe -- the one way out of begin, end and cancel
struct OpenDescribe {
  bool open = false;           // the context's per-batch describe scratch belongs to this batch: other describe-side entry points refuse
  bool side_pending = false;   // the mask branch on the side stream has not been joined yet (read by join_mask_branch alone)
  int B = 0, S_tot = 0;        // what segvlad_describe_end's arguments must match
  StageTimer* timer = nullptr; // the "describe" stage's open event pair (null: profiling off) and its slot
  int slot = 0;
};

constexpr int SV_PIN_TOTALS = 8;   // word of segvlad_ctx::h_pin that mirrors the single-image pass's totals (layout: small_pass_dev.h)
struct segvlad_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // a second stream of the context's own, for kernels that share a launch slot with another one of the same call: forked off
  // `stream` behind an event and joined back before anything else is enqueued (sv_fork_side / sv_join_side); created on first use
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  uint32_t* h_pin = nullptr;          // 64 pinned bytes: scalars read back behind an event instead of a stream synchronisation;
                                      // words SV_PIN_TOTALS, + 1: the single-image pass's running totals (small_pass_dev.h)
  hipEvent_t ev_scalars = nullptr;
  unsigned char* h_desc = nullptr;    // pinned: the per-image flags and the centroids of a segvlad_describe_begin
  size_t h_desc_cap = 0;
  hipEvent_t ev_desc = nullptr;       // behind their copies on the side stream
  OpenDescribe desc;                  // describe.hip: the batch between segvlad_describe_begin and segvlad_describe_end
  char err[512] = {0};
  bool profiling = false;
  bool scope_mute = false;   // set while a redo / fallback pass runs: its inner stages are part of "knn_redo" / "knn_fallback" only
  std::map<std::string, StageTimer> timers;
  SvOptions opt;
  SvSearchStats sstats;

  // vocabulary
  int K = 0, D = 0, Kpad = 0;
  float vocab_maxabs = 0.f;   // max |C_kd| (set_vocab): scale of the residual planes of the "project" form
  float vocab_norm_max = 0.f; // max_k ||C_k||_2 (set_vocab): bound of the projected residuals (16-bit P-space sums)
  // PCA model
  int P = 0, KD = 0, whiten = 0;
  float pca_w_scale = 0.f, pca_mean_maxabs = 0.f;
  bool pca_cproj_valid = false;           // cleared by segvlad_pca_set
  // database (exact kNN)
  int db_d = 0;
  int64_t db_n = 0;
  bool db_has_img = false;
  bool db_added = false;                  // rows were added since the last reset: db_d and db_has_img are fixed (even once removal empties it)
  int64_t db_split_rows = 0;              // rows covered by the bf16 hi/lo planes (built lazily for the large-database search path)
  int64_t db_f16_rows = 0;                // rows covered by the fp16 image of the rows, scaled by a power of two (single-product filter)
  float db_f16_scale = 0.f, db_maxabs = 0.f;
  float db_rn_max = 0.f;
  int64_t db_rn_max_rows = 0;
  bool f16_bias_ok = false;   // this search's batch filter launches may use the biased-accumulator kernel (segvlad_search)
  const float* f16_scale_dev = nullptr;   // set by segvlad_search for the duration of a single-image search (see above)
  // small_head_kernel's grid barrier: arrivals on the device counter (s_tail_tick's last two words: small_pass_dev.h) of every head launched on this
  // context -- the next launch's target is this + its grid size (stream order: see segvlad_set_stream)
  uint64_t small_head_arrivals = 0;
  bool small_head_ran = false;   // this search's pass started with small_head_kernel (which also repairs a poisoned hand-over buffer)
  bool db_heur_off = false;   // set when > 25 % of a search's queries needed the rigorous redo (until the index changes)
  // shortlist search (shortlist_kernels.hip): largest image id of db_img (-1: none), and whether sl_img_off / sl_img_rows -- the
  // image -> row map -- describe the current index (cleared by segvlad_db_add / segvlad_db_reset, rebuilt by the next shortlist search)
  int db_img_max = -1;
  bool sl_map_valid = false;
  // segvlad_search_excluding (exclude_kernels.hip): the host copy of sl_img_off (valid while the map it was copied from is), and the
  // statistics of the last call -- [0] k_fetch, [1] max X_b, [3] images with excluded rows are the host's; [2], the rows the
  // exact tail finished, is a device word fetched by segvlad_exclude_stats (null: no call yet, or the call flagged nothing by construction)
  std::vector<uint32_t> sl_off_host;
  bool sl_off_host_valid = false;
  int64_t ex_stats[4] = {0, 0, 0, 0};
  int64_t rs_stats[5] = {0, 0, 0, 0, 0};   // segvlad_range_stats: total hits, long rows, max / sum of the candidate lists, path
  int64_t gr_stats[3] = {0, 0, 0};         // segvlad_group_stats: k_fetch, rows the exact tail finished, the longest read of a complete row
  const uint32_t* ex_short_dev = nullptr;
  // device-driven single-image passes (small_pass_kernels.hip): the tail kernel's counters of the LAST such search live in device
  // memory and are fetched by segvlad_search_stats (the search itself never reads them back); its running totals reach the host
  // through two pinned words that segvlad_search looks at WITHOUT synchronising -- a database on which the low-rank thresholds
  // keep failing is switched to the rigorous plan one or two calls late instead of never
  const uint32_t* tail_stats_dev = nullptr;   // [4]: rows redone by brute force, second-tier rows, hand-over failures; null = none pending
  uint32_t tail_fail_base = 0;                // h_pin[SV_PIN_TOTALS] when the index last changed
  int64_t tail_rows_since = 0;                // query rows sent through device-driven passes since then

  // Device buffers, as X-macro lists (segvlad_create tags them, segvlad_destroy releases them, guard mode walks them).
  //  persistent: contents outlive a call -- vocab: [K][D] raw centres; vocab_bt: normalised centres in MFMA-B order
  //  [D/2][Kpad/32][64]; pca_scale = 1/sqrt(var) or 1; pca_w1 / pca_w2: fp16 two-term split of comps * pca_w_scale (16-bit MFMA
  //  path); pca_cproj: [P] W mean ("project then aggregate"; rebuilt when stale); db_hi / db_lo / db_f16: 16-bit images of the rows;
  //  s_ref_keys / s_ref_tick: hand-over words of refine_exact_small_kernel (all ones / all zero between launches);
  //  s_tail_tick: tickets (all zero between launches) + running totals of small_tail_kernel
#define SV_PERSISTENT_BUFS(X)                                                                                                    \
  X(vocab) X(vocab_bt) X(pca_mean) X(pca_comps) X(pca_scale) X(pca_w1) X(pca_w2) X(pca_cproj) X(db_rows) X(db_norms) X(db_img)    \
  X(db_hi) X(db_lo) X(db_f16) X(s_ref_keys) X(s_ref_tick) X(s_tail_tick) X(sl_img_off) X(sl_img_rows)
  //  scratch: grow-only, reused across calls, nothing in them is read after the call that wrote it; s_sh_*: exchange buffers of
  //  the row-sharded index (comm.hip); s_rm_*: removal flags, block counts / offsets and the source of every surviving row
  //  (remove_kernels.hip); s_deep_*: the deep lists of the inner search and the query norms of segvlad_search_excluding and
  //  segvlad_search_grouped (one call at a time uses them); s_ex_*: the row flags (+ the short-row counter, which
  //  segvlad_exclude_stats reads after the call) and the tail's slot results of segvlad_search_excluding (exclude_kernels.hip);
  //  s_rs_*: segvlad_range_search (range_kernels.hip) -- the effective radii and filter thresholds, the long-row flags (+ the query
  //  preparation's flag block), per-row hit counts, where a short row's ordered words sit in s_rs_stage, the long rows' offsets /
  //  cursors / words before and after their ordering, the dense query block of the exact sweeps, the device lims of a host caller
  //  and a few counters; s_mp_min: segvlad_match_pairs (match_kernels.hip) -- the row minima [nq][C], then the live slots' column
  //  minima, 64-bit keys; s_vp_best: segvlad_verify_pairs (verify_kernels.hip) -- every slot's best (inlier count, hypothesis) key;
  //  s_sq_id / s_sq_sc: segvlad_sequence_rerank (sequence_kernels.hip) -- every frame's candidate ids and scores in id order;
  //  s_gr_*: segvlad_search_grouped (group_kernels.hip) -- the counters + row flags, and the exact tail's open
  //  rows, their dense query block, a batch's slots / word offsets, cursors, words before and after their ordering, per-image counts;
  //  s_re_*: segvlad_rle_encode (rle_encode_kernels.hip) -- the units' (changes, last change, set pixels) planes, the masks' run
  //  counts and final runs, and the device image of a host caller's counts;
  //  s_rg_*: segvlad_mask_regions (regions_kernels.hip) -- the label plane and the size plane [S][P] of a connected-component pass
  //  and the masks' decisions, areas and boxes;
  //  s_vote_cap: segvlad_vote with a per-image cap (vote_kernels.hip) -- the blanked copy of idx [nq][k] that the vote then reads;
  //  s_vote_uniq, s_vote_tab: segvlad_vote with SEGVLAD_VOTE_UNIQUE_REF -- the copy of idx [nq][k] with the non-winning claims on a
  //  reference segment blanked (the cap and the vote read it), and the {id, best key} hash tables of the query images that the
  //  LDS table does not hold (2 slots of 16 B per entry, zeroed per call);
  //  s_softw: the describe stage under vlad_assign=soft (soft_vlad_kernels.hip) -- the assignment weights w [B][N][K] of the batch;
  //  s_softc: under vlad_assign=soft_pooled -- the mean centre [D];
  //  s_burst: under vlad_burst (burst_kernels.hip) -- the tile sums [B][ceil(N / 128)][N] that add up to g; the discounted weights
  //  go to s_softw (under hard assignment: the one-hot of the labels times u);
  //  s_bseg: under vlad_burst with vlad_burst_scope=segment (burst_seg_kernels.hip) -- the weights u [B][N][64 SC], token rows in
  //  prep_kernel's label-grouped order, column s of a row the weight of that token in segment s (0 outside U(s))
#define SV_SCRATCH_BUFS(X)                                                                                                      \
  X(s_xt) X(s_labels) X(s_rnorm) X(s_gap) X(s_colmask) X(s_gscale) X(s_segimg) X(s_segoff) X(s_adjoff) X(s_dist) X(s_qnorm)      \
  X(s_misc) X(s_minmax) X(s_voteoff) X(s_cand_cnt) X(s_cand_d2) X(s_cand_id) X(s_thr_d2) X(s_thr_idx) X(s_flag) X(s_qh) X(s_ql)  \
  X(s_ref_cnt) X(s_ref_id) X(s_qscale) X(s_qf16) X(s_xh1) X(s_xh2) X(s_desc) X(s_tokorder) X(s_laboff) X(s_rnsorted) X(s_ovf)     \
  X(s_fb_q) X(s_fb_d2) X(s_fb_idx) X(s_fb_rows) X(s_rd_rows) X(s_rd_q) X(s_rd_d2) X(s_rd_idx) X(s_rd_flags) X(s_rd_p1) X(s_rd_p2)  \
  X(s_sel_todo) X(s_vote_keys) X(s_vote_cap) X(s_vote_uniq) X(s_vote_tab) X(s_softw) X(s_softc) X(s_burst) X(s_bseg) X(s_pz) X(s_rowbase) X(s_tilegrp) X(s_phys) X(s_covcnt) X(s_bn) X(s_l0part) X(s_ref_lim) X(s_sh_d2) X(s_sh_idx)          \
  X(s_sh_rec) X(s_sh_all) X(s_sh_d2c) X(s_sh_idc) X(s_grp_cnt) X(s_grp_ids) X(s_grp_rows) X(s_grp_keys) X(s_grp_work) X(s_grp_pos) X(s_tnk_redo) X(s_tail_part) X(s_km_part) X(s_km_cnt) X(s_kflush) \
  X(s_sl_misc) X(s_sl_q) X(s_sl_cur) X(s_sl_uids) X(s_sl_uoff) X(s_sl_unum) X(s_sl_cand) X(s_sl_lens)                            \
  X(s_deep_d2) X(s_deep_idx) X(s_deep_qn) X(s_ex_flag) X(s_ex_td2) X(s_ex_tidx)                                                        \
  X(s_rm_row) X(s_rm_img) X(s_rm_blk) X(s_rm_src) X(s_rm_misc)                                                                    \
  X(s_rs_thr) X(s_rs_flag) X(s_rs_fb) X(s_rs_cnt) X(s_rs_soff) X(s_rs_stage) X(s_rs_loff) X(s_rs_cur) X(s_rs_words) X(s_rs_sorted)  \
  X(s_rs_tmp) X(s_rs_rows) X(s_rs_q) X(s_rs_misc)                                                                                 \
  X(s_mp_min) X(s_vp_best) X(s_sq_id) X(s_sq_sc)                                                                                   \
  X(s_gr_flag) X(s_gr_rows) X(s_gr_q) X(s_gr_plan) X(s_gr_cur) X(s_gr_words) X(s_gr_sorted) X(s_gr_tab)                           \
  X(s_re_unit) X(s_re_mask) X(s_re_counts)                                                                                        \
  X(s_rg_label) X(s_rg_size) X(s_rg_state)
#define SV_DECL_BUF(n) DevBuf n;
  SV_PERSISTENT_BUFS(SV_DECL_BUF)
  SV_SCRATCH_BUFS(SV_DECL_BUF)
#undef SV_DECL_BUF
  template <class F>
  void for_each_buf(F&& f) {
#define SV_VISIT_BUF(n) f(n);
    SV_PERSISTENT_BUFS(SV_VISIT_BUF)
    SV_SCRATCH_BUFS(SV_VISIT_BUF)
#undef SV_VISIT_BUF
    for (auto& b : stage) f(b);
  }
  bool guard = false;          // SEGVLAD_GUARD=1 at segvlad_create
  char guard_hit[96] = {0};    // sticky: the first trampled fence found (buffer tag and which fence)
  // row-sharded index over several GPUs (comm.hip): an RCCL communicator bound at run time
  void* comm = nullptr;   // ncclComm_t
  int comm_rank = 0, comm_world = 1;
  std::vector<uint32_t> sh_flags_host;   // the ranks' status words of a sharded search (target of an asynchronous copy)
  // staging for host<->device pointers: a small ring, indexed by use inside one call
  std::vector<DevBuf> stage;
  struct Pending { void* host; void* dev; size_t bytes; };
  std::vector<Pending> pending_out;
  int stage_used = 0;

  int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
};

// hipFuncSetAttribute(fn, MaxDynamicSharedMemorySize, bytes), remembered per (device, kernel): the driver call takes a
// lock and tens of microseconds; a launcher that repeats it before every launch leaves the GPU idle between kernels
hipError_t sv_max_dyn_lds(const void* fn, size_t bytes);

extern char sv_rccl_lib_override[256];   // comm.hip; filled by segvlad_create from SEGVLAD_RCCL_LIB
// comm.hip: destroys the context's communicator, if any (segvlad_destroy / segvlad_comm_destroy)
void sv_comm_release(segvlad_ctx* ctx);

// ---- pointer staging ---------------------------------------------------------------------------
bool sv_is_device_ptr(const void* p);
// returns a device pointer holding `bytes` of *p (copy enqueued on ctx->stream if p is host memory)
int sv_in(segvlad_ctx* ctx, const void* p, size_t bytes, const void** dev);
// returns a device pointer to write into; if p is host memory the D2H copy happens in sv_finish()
int sv_out(segvlad_ctx* ctx, void* p, size_t bytes, void** dev);
// flushes pending host outputs (synchronises the stream only if there are any) and resets staging; guard mode: also
// synchronises and checks every fence
int sv_finish(segvlad_ctx* ctx);
// guard mode: SEGVLAD_ERR_STATE if any fence of the context's buffers has been written (synchronises the device)
int sv_guard_check(segvlad_ctx* ctx);
int sv_fork_side(segvlad_ctx* ctx);   // side stream waits for everything enqueued on `stream` so far
int sv_join_side(segvlad_ctx* ctx);   // `stream` waits for everything enqueued on the side stream so far
struct StreamSwitch {   // ctx->stream replaced for a scope: a branch is issued on the side stream by the code that serves the main one
  segvlad_ctx* ctx;
  hipStream_t saved;
  StreamSwitch(segvlad_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) { ctx->stream = s; }
  ~StreamSwitch() { ctx->stream = saved; }
};
void sv_begin(segvlad_ctx* ctx);
// first line of every entry point that takes a context
#define CHECK_CTX()                 \
  if (!ctx) return SEGVLAD_ERR_ARG; \
  sv_begin(ctx)
// Between segvlad_describe_begin and segvlad_describe_end the context's per-batch scratch (segment / adjacency offsets, the
// token-major copy, the labels) belongs to THAT batch, and the mask branch is in flight on the side stream: every other entry
// point that would write them refuses instead of describing a different batch with the open one's offsets.
// (describe.hip's mask entries, rle_kernels.hip's, rle_encode_kernels.hip's and regions_kernels.hip's)
#define CHECK_NO_OPEN_DESCRIBE(what)                                                                                        \
  if (ctx->desc.open)                                                                                                       \
  return ctx->fail(SEGVLAD_ERR_STATE, what ": a segvlad_describe_begin is open on this context (call segvlad_describe_end first)")

// a fresh (start, stop) event pair of stage `name`, its start recorded on the context's stream; null when profiling is off or muted
StageTimer* sv_stage_open(segvlad_ctx* ctx, const char* name, int* slot);
struct StageScope {
  segvlad_ctx* ctx;
  StageTimer* t = nullptr;
  int slot = 0;
  StageScope(segvlad_ctx* c, const char* name) : ctx(c) { t = sv_stage_open(c, name, &slot); }
  ~StageScope() { if (t) (void)hipEventRecord(t->ev[2 * slot + 1], ctx->stream); }
  void count(int n = 1) { if (t) t->launches += n; }
};

// ---- kernel launchers (defined in the *_kernels.hip units) ---------------------------------------
// mask_kernels.hip
int sv_launch_incidence(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch,
                        uint64_t* inc_bits, double* centroids /* may be null */);
int sv_launch_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, double* out);
bool sv_adjacency_fits(int S_max);   // an image of S_max segments fits the in-LDS Delaunay (else: SEGVLAD_ERR_LIMIT)
int sv_launch_adjacency(segvlad_ctx* ctx, const double* cent, const int32_t* seg_off_dev, const int64_t* adj_off_dev,
                        int B, int S_max, int order, uint8_t* adj, uint32_t* n_bad, uint8_t* img_flags = nullptr);
// assign_kernels.hip
int sv_launch_vocab_prepare(segvlad_ctx* ctx);
int sv_launch_assign(segvlad_ctx* ctx, const float* tokens, int B, int N, float* xt, uint8_t* labels, float* rnorm,
                     float* gap);
// vlad_kernels.hip
int sv_launch_prep(segvlad_ctx* ctx, const uint8_t* labels, const uint64_t* inc_bits, const int32_t* seg_off_dev,
                   const int64_t* adj_off_dev, const uint8_t* adj, int B, int N, int K, int S_max, int SC,
                   uint64_t* colmask, float* gscale, int32_t* phys /* [B][N], or null */, int32_t* cov_cnt /* [B][K] */,
                   int cover /* 0: every token counts as covered */);
// after sv_launch_prep, whose label-grouped token order and 1/||x|| it reads.  centres == nullptr: the inputs are residuals already
// (x * rnorm - 0)
int sv_launch_aggregate(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const float* centres, int K, int D,
                        const int32_t* seg_off_dev, const float* gscale, int B, int N, int SC, float* out, float* block_norms,
                        const float* mean = nullptr, float xscale = 0.f, uint16_t* h1 = nullptr, uint16_t* h2 = nullptr);

// soft_vlad_kernels.hip (option vlad_assign=soft:<T>; after sv_launch_prep, whose label-grouped token order, 1/||x|| and column masks
// they read).  weights: w[b][n][0..K) = softmax_k(temp * <x^_n, c^_k>) from the channel-major tokens.  aggregate (the frame of
// weighted_agg_dev.h, which sv_launch_burst_seg_aggregate shares: LDS layout, covered-position list, epilogue, launch geometry): the
// intra-normalised blocks V[s][k] / max(||V[s][k]||, 1e-12) into out [S][K*D] and ||V[s][k]|| into block_norms [S][K] (never null); with mean_centre
// (soft_pooled: [D] from sv_launch_soft_centre_mean) every block is K sum w (x^ - mean centre), the residuals against all K centres.
// finalize: every row of out scaled to unit length from its block norms.
int sv_launch_soft_weights(segvlad_ctx* ctx, const float* tokens, int B, int N, float temp, float* w);
int sv_launch_soft_centre_mean(segvlad_ctx* ctx, const float* centres, int K, int D, float* mean_centre);
int sv_launch_soft_aggregate(segvlad_ctx* ctx, const float* xt, const float* w, const uint64_t* colmask, const float* centres, int K, int D,
                             const int32_t* seg_off_dev, int B, int N, int SC, float* out, float* block_norms,
                             const float* mean_centre = nullptr);
int sv_launch_soft_finalize(segvlad_ctx* ctx, const float* block_norms, int S_tot, int K, int D, float* out);

// burst_kernels.hip (option vlad_burst=<a>:<b>:<p>; after sv_launch_assign, whose token-major copy and 1 / ||x|| they read).  The
// 128 x 128 self-similarity tile, the dealing of workgroups to images and u = g^-p are gram_tile_dev.h's, one definition for both scopes.
// gram: part [B][sv_burst_tiles(N)][N], the sums of sigmoid(a (2 cos(x_n, x_m) - 2) + b) over the m of one 128-token tile, every slot
// written once.  finish: g[n] = the tile sums in tile order, u = g^-p (exactly 1 for p = 0), and w [B][N][K]: one_hot -- u[n] at
// k = labels[n], 0 elsewhere; otherwise the rows of w (sv_launch_soft_weights) scaled by u[n].
int sv_burst_tiles(int N);
int sv_launch_burst_gram(segvlad_ctx* ctx, const float* xt, const float* rnorm, int B, int N, int D, float a, float b, float* part);
int sv_launch_burst_finish(segvlad_ctx* ctx, const float* part, const uint8_t* labels, int B, int N, int K, float p, bool one_hot, float* w);

// burst_seg_kernels.hip (vlad_burst with vlad_burst_scope=segment; after sv_launch_prep, whose label-grouped order, sorted 1 / ||x|| and
// column masks they read).  gram: u [B][N][64 SC], row = POSITION in the label-grouped order, column s = g[s][n]^-p where bit s of the
// position's column mask is set and 0 elsewhere, g[s][n] = sum_{m in U(s)} sigmoid(a (2 cos(x_n, x_m) - 2) + b); the chunks of 64
// columns beyond an image's segments are left unwritten.  aggregate: the frame of weighted_agg_dev.h -- the intra-normalised blocks
// into out [S][K*D], ||V[s][k]|| into block_norms [S][K], mean_centre as above -- with the A operand bit ? u : 0; w == nullptr is hard assignment (cluster k walks label k's positions with weight 1), else w [B][N][K] of
// sv_launch_soft_weights over every covered position.  sv_launch_soft_finalize follows as behind the soft aggregation.
int sv_launch_burst_seg_gram(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const int32_t* seg_off_dev, int B, int N, int D,
                             int SC, float a, float b, float p, float* u);
int sv_launch_burst_seg_aggregate(segvlad_ctx* ctx, const float* xt, const float* w, const float* u, const uint64_t* colmask,
                                  const float* centres, int K, int D, const int32_t* seg_off_dev, int B, int N, int SC, float* out,
                                  float* block_norms, const float* mean_centre = nullptr);

// block_norm_kernels.hip
// block norms + the fp16 planes of the token residuals x^ - C_k, grouped by cluster (rowbase from sv_launch_group_plan); after sv_launch_prep
int sv_launch_token_norms(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const float* centres, int K, int D,
                          const int32_t* seg_off_dev, int B, int N, int SC, float* block_norms, float xscale, uint16_t* h1,
                          uint16_t* h2, const int32_t* rowbase, int64_t dummy_row /* first row of a 256-row tile nobody reads */,
                          const int32_t* phys /* sv_launch_prep */);

// kmeans_kernels.hip: per-cluster sums of the normalised tokens + label counts of a batch, ACCUMULATED into sums / counts
int sv_launch_centroid_sums(segvlad_ctx* ctx, const float* xt, const float* rnorm, const uint8_t* labels, int B, int N, int D, int K,
                            double* sums, int64_t* counts);

// gemm_kernels.hip
int sv_launch_row_sumsq(segvlad_ctx* ctx, const float* X, int64_t n, int d, float* out);
int sv_launch_normalize_rows(segvlad_ctx* ctx, const float* X, int64_t n, int d, float* Y);
// C[M][N] = epilogue(A[M][Kd] . B[N][Kd]^T)
//   mode 0 (PCA):  A' = A - a_sub (a_sub [Kd] or null); C = acc * col_scale[n]
//   mode 1 (L2):   C = row_add[m] + col_add[n] - 2 acc
int sv_launch_gemm_nt(segvlad_ctx* ctx, int mode, const float* A, const float* Bm, float* C, int M, int N, int Kd,
                      int64_t ldc, const float* a_sub, const float* col_scale, const float* row_add,
                      const float* col_add);

// distance of every query to database rows 0, b_stride, 2*b_stride, ... (n_sample of them); column j of
// `dist` is sample j
int sv_launch_l2_strided(segvlad_ctx* ctx, const float* Q, const float* R, float* dist, int M, int n_sample, int Kd,
                         int64_t ldc, const float* qn, const float* rn, int b_stride, bool split_ok = false);
// the same launch with the K split's reduction left to the caller: *splits > 1 -> *parts = the partial dot products
// [*splits][M][ldc] (slices to be added in index order, then sv_d2 with the norms); *splits == 1 -> `dist` is finished
int sv_launch_l2_strided_parts(segvlad_ctx* ctx, const float* Q, const float* R, float* dist, int M, int n_sample, int Kd,
                               int64_t ldc, const float* qn, const float* rn, int b_stride, const float** parts, int* splits);
// the reduction of such a block fused with the rank select of every row (<= 4096 columns, <= 128 rows): thr_out[row] = the
// rank-th smallest distance of the row -- what splitk_reduce_d2_kernel + sv_launch_select_approx(Threshold, fixed_cnt) compute,
// value for value, in one launch instead of two (the single-image pass is a chain of dependent launches); also zeroes
// cand_cnt[row]; a row already flagged in fail_rows gets -inf
int sv_launch_l0_reduce_rank(segvlad_ctx* ctx, const float* parts, int splits, int M, int n_sample, int64_t ldc, const float* qn,
                             const float* rn, int b_stride, int rank, float* thr_out, uint32_t* cand_cnt, const uint32_t* fail_rows);
// same distances, but entries <= thr[m*thr_ld] are appended to (cand_d2, cand_id)[m][0..cap) via cand_cnt[m]
int sv_launch_l2_filter(segvlad_ctx* ctx, const float* Q, const float* R, int M, int n_sample, int Kd, const float* qn,
                        const float* rn, int b_stride, const float* thr, int64_t thr_ld, uint32_t* cand_cnt,
                        float* cand_d2, uint32_t* cand_id, int cap);

// knn_filter_kernels.hip (the fp16 filter; sv_choose_f16_kernel and sv_f16_eps_kblock, declared with the options above, live there too)
int sv_launch_f16_filter(segvlad_ctx* ctx, const uint16_t* Qh, const uint16_t* Rh, int M, int n_sample, int d, int b_stride,
                         float inv_scale, const float* qn, const float* rn, const float* thr, int64_t thr_ld, float eps_mult,
                         float c_eps, float rn_max, uint32_t* cand_cnt, float* cand_d2, uint32_t* cand_id, int cap, int skip = 0);
// skip = 16: the operand rows are the database rows that are NOT multiples of 16, in order (n_sample of them; b_stride = 1)
bool sv_f16_filter_skip_ok(const segvlad_ctx* ctx, int M, int64_t n_rows, int d);
// knn_operand_kernels.hip (the filters' operand planes and the scalars a search reads back)
int sv_launch_to_f16(segvlad_ctx* ctx, const float* X, int64_t n_elems, float scale, uint16_t* out);
// single-image searches: the query plane and its scales without a host round trip (scales_dev[0] = query scale,
// [1] = 1 / (query scale x db_scale)); ctx->f16_scale_dev != null makes the filter kernel read [1] instead of its argument
// qn_out != null (needs d % 4 == 0, 16-byte aligned rows): also the rows' squared norms, bit for bit sv_launch_row_sumsq's
int sv_launch_query_f16_small(segvlad_ctx* ctx, const float* X, int64_t n_elems, float db_scale, uint16_t* out, float* scales_dev,
                              float* qn_out, int nq, int d, uint32_t* zero, int zero_words);
int sv_launch_to_f16_devscale(segvlad_ctx* ctx, const float* X, int64_t n_elems, const float* scales_dev, uint16_t* out);
int sv_row_norm_max(segvlad_ctx* ctx, const float* norms, int64_t n, float* out_host, bool finite_only = false);
int sv_row_norm_min(segvlad_ctx* ctx, const float* norms, int64_t n, float* out_host);
int sv_maxabs(segvlad_ctx* ctx, const float* x, int64_t n, float* out_host, bool finite_only = false, bool* nonfinite_host = nullptr);
int sv_ensure_pinned_words(segvlad_ctx* ctx);
int sv_maxabs_and_norm_min_begin(segvlad_ctx* ctx, const float* x, int64_t n, const float* norms, int64_t n_norms);
// (the scalars over the finite values alone; *nonfinite_host: x holds a NaN or an Inf; *norm_max_host: the largest finite norm)
int sv_maxabs_and_norm_min_end(segvlad_ctx* ctx, int64_t n, int64_t n_norms, float* maxabs_host, float* norm_min_host, bool* nonfinite_host,
                               float* norm_max_host);
// knn_bf16_filter_kernels.hip
int sv_launch_split_bf16(segvlad_ctx* ctx, const float* X, int64_t n_elems, uint16_t* hi, uint16_t* lo);
int sv_launch_bf16_filter(segvlad_ctx* ctx, const uint16_t* Qh, const uint16_t* Ql, const uint16_t* Rh, const uint16_t* Rl,
                          int M, int n_sample, int d, int b_stride, const float* qn, const float* rn, const float* thr,
                          int64_t thr_ld, float eps_mult, float c_eps, float rn_max, uint32_t* cand_cnt, float* cand_d2,
                          uint32_t* cand_id, int cap);
// knn_select_kernels.hip (the filters' candidate lists ranked; sv_launch_l0_reduce_rank above lives there too)
// A select ranks every row's candidate list and then decides what its order statistic A (the k-th smallest d2~) means:
//   Threshold  thr_out[row] = A, the next level's threshold; cnt[row] is ZEROED (the next level's filter appends from zero, no
//              memset launch between the levels).
//   Band       the refine list ref_id[row][0 .. ref_cnt[row]) = {d2~ <= A + 2 eps} (unordered).  A band longer than rcap marks
//              its row in rovf_rows, with the band's limit in ref_lim, counted in *rovf_count (second tier:
//              sv_launch_refine2_compact + sv_launch_refine_exact(..., rcap = cap, only_rows = rovf_rows) refine it straight
//              from the candidate list) -- or, without a second tier, flags it.
//   Carry      (batches, the level before the last one when that runs over the complement of this level's sample -- option
//              level_carry) thr_out = min(A, thr_in) and the entries with d2~ <= thr_out + 2 eps STAY in the list, compacted to
//              its front, cnt[row] = their number: the last level appends behind them instead of computing the sample's rows a
//              second time.
// check != 0 (guessed thresholds): a list shorter than k is flagged, and Band flags A > thr_in[row * thr_in_ld] (the threshold
// the list was collected under).  Flagged rows (also: list overflow, rows flagged at a coarser level) are marked in ovf_rows and
// counted once in *ovf_count; they get an empty refine list (Band) or a threshold of -inf.
// Passed to the kernels by value; the row rule itself is select_dev.h.
enum class SvSelect : int { Threshold = 0, Band = 1, Carry = 2 };
struct SvSelectArgs {
  uint32_t* cnt = nullptr;        // [nq] list lengths (not read when fixed_cnt >= 0)
  float* cd2 = nullptr;           // [nq][cap] d2~
  uint32_t* cid = nullptr;        // [nq][cap] index rows
  int cap = 0;
  int k = 0;                      // which order statistic of the list is A (Threshold, Carry: the next level's rank; Band: k)
  SvSelect mode = SvSelect::Threshold;
  int check = 0;
  const float* thr_in = nullptr;
  int64_t thr_in_ld = 0;
  const float* qn = nullptr;      // eps(q) = c_eps sqrt(qn[row] rn_max)
  float c_eps = 0.f, rn_max = 0.f;
  float* thr_out = nullptr;
  uint32_t* ref_cnt = nullptr;
  uint32_t* ref_id = nullptr;     // [nq][rcap]
  int rcap = 0;
  uint32_t* ovf_rows = nullptr;
  uint32_t* ovf_count = nullptr;
  uint32_t* rovf_rows = nullptr;  // second tier (optional)
  uint32_t* rovf_count = nullptr;
  float* ref_lim = nullptr;
  int fixed_cnt = -1;             // >= 0: every row is a list of that length (the sampled level's distance block)
};
int sv_launch_select_approx(segvlad_ctx* ctx, int nq, const SvSelectArgs& a);
int sv_launch_refine2_compact(segvlad_ctx* ctx, const uint32_t* rovf_rows, const float* ref_lim, uint32_t* cand_cnt,
                              const float* cand_d2, uint32_t* cand_id, int nq, int cap);
// knn_refine_kernels.hip (the refine lists evaluated exactly)
// only_rows != null: rows whose flag is clear are skipped (their outputs stay as they are)
// fail_rows / fail_count / poison_dev (optional): the single-image refinement hands keys between workgroups through global
// memory and CHECKS the hand-over (refine_exact_small_kernel): a query whose keys did not all arrive is flagged there like
// a failed threshold check, and *poison_dev (set to a device word when that kernel ran, else to null) is non-zero afterwards;
// the caller then calls sv_refine_small_repair before the buffers' next use.
// fz / fused_done (round 6): when the shared-list kernel of a single-image pass runs, it finishes the rows the select flagged itself
// (small_pass_dev.h: SvSmallFinish) and *fused_done is set: the caller then launches no small_tail_kernel behind it.
struct SvSmallFinish;
int sv_launch_refine_exact(segvlad_ctx* ctx, const float* Q, const float* R, int nq, int d, const float* qn, const float* rn,
                           const uint32_t* ref_cnt, const uint32_t* ref_id, int rcap, int k, float* d2_out, int64_t* idx_out,
                           const uint32_t* only_rows = nullptr, uint32_t* fail_rows = nullptr, uint32_t* fail_count = nullptr,
                           const uint32_t** poison_dev = nullptr, const SvSmallFinish* fz = nullptr, bool* fused_done = nullptr);
int sv_refine_small_repair(segvlad_ctx* ctx);
// small_pass_kernels.hip
int sv_small_words(segvlad_ctx* ctx);   // ctx->s_tail_tick reserved and zeroed (its words: small_pass_dev.h)
// tests only (option debug_small_tail): force the flags of a pass that needed none
int sv_launch_small_tail_debug(segvlad_ctx* ctx, int m, uint32_t* fail_rows, uint32_t* fail_count, uint32_t* rovf_rows, float* ref_lim);
// the device-driven tail of a single-image pass (<= 128 rows): launched behind the refinement, returns at
// once when fail_count[0] == fail_count[1] == 0, else finishes the flagged rows on the device (second tier from the candidate
// lists; exact brute force for rows flagged for a redo) -- the search needs no read-back.  stats: [4] device words of this search.
int sv_launch_small_tail(segvlad_ctx* ctx, const float* Q, const float* R, const float* qn, const float* rn, int64_t n, int d, int m, int k,
                         uint32_t* fail_rows, uint32_t* fail_count, uint32_t* rovf_rows, const float* ref_lim, const uint32_t* cand_cnt,
                         const float* cand_d2, const uint32_t* cand_id, int cap, float* d2_out, int64_t* idx_out, uint32_t* stats);
// the HEAD of such a pass in one launch: the queries' fp16 plane (scales_dev[0] = scale, [1] = 1 / (scale x db_scale)), their squared
// norms (row_sumsq's bits), the zeroed flag block, and thr_out[q] = the rank-th smallest APPROXIMATE distance (the filter's own fp16
// product) of query q to the n0 sample rows 0, stride, 2 stride, ... of the fp16 plane Rh; cand_cnt[q] = 0.
// cand_scratch: m x n0 floats.  sv_small_head_ok: the shapes it takes.
bool sv_small_head_ok(int m, int d, int n0, int rank);
// a BATCH search's sampled level from the same product: dist[q][j] = d2~(query q, database row j * stride), j < n0 (row stride ld)
int sv_launch_sample_f16_batch(segvlad_ctx* ctx, const uint16_t* Qh, const uint16_t* Rh, int m, int n0, int d, int64_t stride, float inv_scale,
                               const float* qn, const float* rn, float* dist, int64_t ld);
int sv_launch_small_head(segvlad_ctx* ctx, const float* X, int m, int d, const uint16_t* Rh, const float* rn, int64_t stride, int n0,
                         float db_scale, int rank, uint16_t* qplane, float* scales_dev, float* qn_out, uint32_t* zero, int zero_words,
                         float* cand_scratch, float* thr_out, uint32_t* cand_cnt);   // ctx->h_pin (16 zeroed words) + ctx->ev_scalars
// refine_group_kernels.hip: the same refinement for a batch, with the bands of 32 consecutive query rows evaluated over the
// union of their rows where they overlap (option refine_group); *launches = kernels launched
constexpr int SV_RG_UCAP = 2048;   // longest union a group may hold (longer: its rows keep the per-row kernels)
int sv_launch_refine_grouped(segvlad_ctx* ctx, const float* Q, const float* R, int nq, int d, const float* qn, const float* rn,
                             const uint32_t* ref_cnt, const uint32_t* ref_id, int rcap, int k, float* d2_out, int64_t* idx_out,
                             int* launches, const uint32_t* only_rows = nullptr, int live_groups_hint = 0);
int sv_refine_group_stats(segvlad_ctx* ctx, int nq, int64_t* groups, int64_t* grouped, int64_t* union_sum);
// gemm_f16x3_kernels.hip
int sv_launch_split_f16x2(segvlad_ctx* ctx, const float* X, int64_t n_rows, int d, const float* sub, float scale, uint16_t* h1,
                          uint16_t* h2);
int sv_launch_gemm_f16x3(segvlad_ctx* ctx, const uint16_t* A1, const uint16_t* A2, const uint16_t* B1, const uint16_t* B2, int M,
                         int N, int Kd, float out_scale, const float* col_scale, float* C);
int sv_launch_gemm_f16x3_grouped(segvlad_ctx* ctx, const uint16_t* A1, const uint16_t* A2, const uint16_t* B1, const uint16_t* B2,
                                 int M_pad, int N, int Kd, int n_groups, const int32_t* tile_group, float out_scale, float* C,
                                 float pair_scale);
// project_kernels.hip ("project then aggregate" form of segvlad_images_pca)
int sv_launch_group_plan(segvlad_ctx* ctx, const int32_t* cov_cnt, int B, int K, int32_t* rowbase, int32_t* tile_group, int max_tiles);
int sv_launch_project_consts(segvlad_ctx* ctx, const float* comps, const float* mean, int P, int64_t KD, float* wmu /*[P] = W mean*/);
bool sv_project_z_pairs(const segvlad_ctx* ctx, float zscale, int64_t rows, int P);
int sv_launch_project_aggregate(segvlad_ctx* ctx, const float* Z, const float* wmu, const float* block_norms, const float* gscale,
                                const uint64_t* colmask, const int32_t* lab_off, const int32_t* rowbase, const int32_t* phys,
                                const int32_t* seg_off_dev, int B, int N, int K, int P, int SC, int S_max, const float* col_scale,
                                float* Y, float zscale, int z_pairs, int64_t zero_row);

// select_kernels.hip
// top-k of per-query candidate lists (LDS sort on (distance, id)); a list longer than cap flags its query row in
// ovf_rows (and counts it once in *ovf_count): that query is redone on the matrix path
int sv_launch_select_cand(segvlad_ctx* ctx, const uint32_t* cand_cnt, const float* cand_d2, const uint32_t* cand_id,
                          int nq, int cap, int k, float* d2_out, int64_t* idx_out, uint32_t* ovf_rows, uint32_t* ovf_count);
int sv_launch_select_topk(segvlad_ctx* ctx, const float* dist, int64_t ld, int nq, int64_t n, int k, float* d2_out,
                          int64_t* idx_out, int64_t out_ld, int64_t id_base);
int sv_launch_merge_topk(segvlad_ctx* ctx, const float* d2_parts, const int64_t* idx_parts, int nq, int cand, int k,
                         float* d2_out, int64_t* idx_out);
int sv_launch_sims(segvlad_ctx* ctx, const float* d2, const int64_t* idx, int nq, int k_in, int k_keep, float* sims,
                   int64_t* idx_out);
int sv_launch_minmax(segvlad_ctx* ctx, const float* sims, int64_t count, float* minmax_dev);

// shortlist_kernels.hip: the largest id of img_dev[0, n) (synchronises)
int sv_img_max(segvlad_ctx* ctx, const int32_t* img_dev, int64_t n, int* out);

// search.hip: segvlad_search behind its checks and staging (q / d2 / idx on the device, nq >= 1, the index has a dimension)
int sv_search_dev(segvlad_ctx* ctx, const float* q, int nq, int k, float* d2, int64_t* idx);
// shortlist_kernels.hip, for segvlad_search_excluding: the image -> row map with its offsets mirrored in ctx->sl_off_host; and the
// exact tail (see there)
constexpr int SV_EX_MAX_E = 8;                  // exclusion intervals per query image
constexpr int SV_EX_RANGES = SV_EX_MAX_E + 1;   // ... whose complement is at most this many ranges of image ids
int sv_sl_map_host(segvlad_ctx* ctx);
int sv_launch_exclude_tail(segvlad_ctx* ctx, const float* Q, const float* qn, const int32_t* groups, int ng, int gmax, int n_slots,
                           const uint32_t* unum, const uint32_t* uoff, const uint32_t* ustart, int n_tab, const uint32_t* flags,
                           int k, float* d2_tmp, int64_t* idx_tmp);

// search.hip: the entry preamble of the searches derived from segvlad_search; `entry` is the name the messages start with.
// SEGVLAD_ERR_ARG unless qseg_offsets [n_img + 1] is there, host memory, runs from 0 to nq and never decreases; SEGVLAD_ERR_STATE
// unless the index has a dimension and an img_of_seg map; *out = dq [nq][db_d] itself or -- a row-offset view of a device tensor,
// off the 16-byte boundary the exact GEMMs load by -- its copy in ctx->s_sl_q; every one of n slots (+inf, -1): an emptied index
int sv_check_qseg_offsets(segvlad_ctx* ctx, const char* entry, const int32_t* qseg_offsets, int n_img, int nq);
int sv_check_img_index(segvlad_ctx* ctx, const char* entry);
int sv_aligned_queries(segvlad_ctx* ctx, const float* dq, int nq, const float** out);
hipError_t sv_fill_none(segvlad_ctx* ctx, float* d2, int64_t* idx, size_t n);

// range_kernels.hip (segvlad_range_search; see the kernels): thresholds and long-row flags from the radii; one chunk's list
// statistics out_dev = {stage words needed, sum, max, long rows}; the exact evaluation + ordering of the short rows' lists into
// `stage`; the counts -> offsets scan (flags != null: flagged rows only); the dense block of the listed query rows; one exact
// distance block counted (words == null) or emitted; the ordering of the emitted segments; the unpacking of ordered words
int sv_launch_range_thr(segvlad_ctx* ctx, const float* radius2, int nq, float* eff, float* thr, uint32_t* flags, bool all_long);
int sv_launch_range_cand_stats(segvlad_ctx* ctx, const uint32_t* cand_cnt, int m, int cap, uint32_t* flags, uint64_t* out_dev);
int sv_launch_range_refine(segvlad_ctx* ctx, const float* Q, const float* R, int m, int d, const float* qn, const float* rn,
                           const float* eff, const uint32_t* cand_cnt, const uint32_t* cand_id, int cap, uint32_t list_max,
                           const uint32_t* flags, uint32_t* cnt, int64_t* soff, uint64_t* stage, uint64_t* cursor);
int sv_launch_range_scan(segvlad_ctx* ctx, const uint32_t* cnt, const uint32_t* flags, int nq, int64_t* lims);
int sv_launch_range_gather(segvlad_ctx* ctx, const float* Q, const float* qn, const float* eff, const int32_t* rows, int nr, int d,
                           float* Y, float* yn, float* yeff);
int sv_launch_range_block(segvlad_ctx* ctx, const float* dist, int64_t ld, int mq, int ns, int64_t col0, const float* eff,
                          const int32_t* rows, uint32_t* cnt, const int64_t* woff, uint32_t* cur, uint64_t* words);
int sv_range_sort_segments(segvlad_ctx* ctx, const uint64_t* words, uint64_t* sorted, int64_t n_words, int nq, const int64_t* off);
// search.hip: one sweep of the exact distance blocks of nl dense query rows (qx, norms qnx, effective radii effx; rows_dev: the
// row of cnt / woff / cur each one is) over the whole index -- counted into cnt (words == null) or emitted at
// words[woff[row] + cur[row]++]; also the exact tail of segvlad_search_grouped
int sv_range_exact_sweep(segvlad_ctx* ctx, const float* qx, const float* qnx, const float* effx, const int32_t* rows_dev, int nl,
                         uint32_t* cnt, const int64_t* woff, uint32_t* cur, uint64_t* words, int* launches);
int sv_launch_range_unpack(segvlad_ctx* ctx, const uint64_t* src, const int64_t* srcoff, const uint32_t* flags, uint32_t want, int nq,
                           const int64_t* lims, float* d2_out, int64_t* idx_out);

// remove_kernels.hip (segvlad_db_remove): the keep flags of the listed rows / images, every surviving row's new position
// (src_of_dst in ctx->s_rm_src, new_id [db_n] or null), then counts_host [3] = {n', survivors below plane_rows_a, below plane_rows_b}
// (synchronises; *launches = kernels launched); and the gather of one plane's first n_dst surviving rows (row pitch in bytes, a
// multiple of 4) into dst -- one launch
int sv_remove_positions(segvlad_ctx* ctx, const int64_t* row_ids, int64_t n_row_ids, const int32_t* img_ids, int64_t n_img_ids,
                        int64_t* new_id, int64_t plane_rows_a, int64_t plane_rows_b, int64_t* counts_host, int* launches);
int sv_launch_remove_gather(segvlad_ctx* ctx, const void* src, void* dst, size_t pitch, int64_t n_dst);

// vote_kernels.hip
int sv_launch_vote(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg,
                   int64_t n_ref_seg, const int32_t* qoff_dev, const int32_t* qoff_host, int n_img, int k,
                   const float* minmax_dev, int n_top, int mode, int32_t* pred, double* score);
// the per-image cap of segvlad_vote's mode bits: out [nq][k] = idx with every valid entry blanked (-1) that has m earlier valid
// entries of its row on the same image (one launch)
int sv_launch_vote_cap(segvlad_ctx* ctx, const int64_t* idx, const int32_t* img_of_seg, int64_t n_ref_seg, int nq, int k, int m,
                       int64_t* out);
// SEGVLAD_VOTE_UNIQUE_REF: out [nq][k] = idx with every valid entry blanked (-1) that is not the winner (largest sim, then first in
// visiting order) among its query image's entries on the same reference segment; sims may be null.  *launches: what was enqueued
int sv_launch_vote_unique(segvlad_ctx* ctx, const int64_t* idx, const float* sims, int64_t n_ref_seg, const int32_t* qoff_dev,
                          const int32_t* qoff_host, int n_img, int k, int64_t* out, int* launches);

// api.hip: the checks and staging of segvlad_vote, shared with segvlad_vote_global (comm.hip)
struct SvVote {
  const void* di = nullptr;    // idx on the device (with UNIQUE_REF / a per-image cap: its blanked copy in ctx->s_vote_uniq / s_vote_cap)
  const void* ds = nullptr;    // sims on the device (null in COUNT mode without sims)
  const void* dimg = nullptr;  // segment -> image map on the device
  int64_t n_ref = 0;
  void* op = nullptr;          // pred / score outputs (device, or staging flushed by sv_finish)
  void* os = nullptr;
  float* mm = nullptr;         // the two-float extrema slot the vote kernel reads
  int nq = 0;                  // query segments (qseg_offsets[n_img])
  int base = 0;                // mode & 0x7f: SEGVLAD_VOTE_WT_BORDA_IM or SEGVLAD_VOTE_COUNT
};
int sv_vote_prepare(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg, int64_t n_ref_seg,
                    const int32_t* qseg_offsets, int n_img, int k, int n_top, int mode, int32_t* pred_out, double* score_out,
                    SvVote* v);
