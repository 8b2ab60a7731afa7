// The index and the exact kNN search of the C-ABI (segvlad_db_*, segvlad_search, segvlad_search_stats): host-side
// orchestration only -- the search plan, scratch sizing and the kernel sequence of each pass on the context stream.  Also the
// entry preamble (sv_check_qseg_offsets ... sv_fill_none) of the searches derived from it, which live with their kernels.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.h"
#include "small_pass_dev.h"

// Grows b to at least new_bytes (plus new_bytes / slack of room), keeping its first old_bytes (synchronises when it copies).
static hipError_t grow_keep(segvlad_ctx* ctx, DevBuf& b, size_t old_bytes, size_t new_bytes, size_t slack) {
  if (new_bytes <= b.cap) return hipSuccess;
  DevBuf nb;
  nb.tag = b.tag;
  nb.guard = b.guard;
  nb.fixed = b.fixed;
  hipError_t e = nb.reserve(new_bytes + new_bytes / slack);
  if (e != hipSuccess) return e;
  if (old_bytes) {
    e = hipMemcpyAsync(nb.p, b.p, old_bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return e;
  }
  b.release();
  b = nb;
  return hipSuccess;
}

// The index changed: the shortlist map, the heuristic switch-off and the device tail's redo totals start again.
static void index_changed(segvlad_ctx* ctx) {
  ctx->sl_map_valid = false;
  ctx->db_heur_off = false;
  if (ctx->tail_rows_since > 0) (void)hipStreamSynchronize(ctx->stream);   // (the tail's pinned totals have landed)
  ctx->tail_fail_base = ctx->h_pin ? reinterpret_cast<volatile uint32_t*>(ctx->h_pin)[SV_PIN_TOTALS] : 0u;
  ctx->tail_rows_since = 0;
}

extern "C" {

int segvlad_db_reset(segvlad_ctx* ctx) {
  CHECK_CTX();
  ctx->db_n = 0;
  ctx->db_d = 0;
  ctx->db_has_img = false;
  ctx->db_added = false;
  ctx->db_img_max = -1;
  ctx->db_split_rows = 0;
  ctx->db_f16_rows = 0;
  ctx->db_f16_scale = 0.f;
  ctx->db_maxabs = 0.f;
  ctx->db_rn_max = 0.f;
  ctx->db_rn_max_rows = 0;
  index_changed(ctx);
  return SEGVLAD_OK;
}

int segvlad_db_add(segvlad_ctx* ctx, const float* R, int n, int d, const int32_t* img_of_seg) {
  CHECK_CTX();
  if (n < 0 || d <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "db_add: bad shape");
  // (an index that removal has emptied keeps its dimension and its img_of_seg rule until db_reset)
  if (ctx->db_added && d != ctx->db_d) return ctx->fail(SEGVLAD_ERR_ARG, "db_add: d=%d but the index holds d=%d", d, ctx->db_d);
  if (ctx->db_added && ctx->db_has_img != (img_of_seg != nullptr))
    return ctx->fail(SEGVLAD_ERR_ARG, "db_add: img_of_seg must be given for all rows or none");
  if (n == 0) return SEGVLAD_OK;
  if (!R) return ctx->fail(SEGVLAD_ERR_ARG, "db_add: null rows");
  const int64_t n_new = ctx->db_n + n;
  SV_HIP(grow_keep(ctx, ctx->db_rows, (size_t)ctx->db_n * d * 4, (size_t)n_new * d * 4, 2));
  SV_HIP(grow_keep(ctx, ctx->db_norms, (size_t)ctx->db_n * 4, (size_t)n_new * 4, 2));
  float* dst = ctx->db_rows.as<float>() + (size_t)ctx->db_n * d;
  SV_HIP(hipMemcpyAsync(dst, R, (size_t)n * d * 4, hipMemcpyDefault, ctx->stream));
  if (img_of_seg) {
    SV_HIP(grow_keep(ctx, ctx->db_img, (size_t)ctx->db_n * 4, (size_t)n_new * 4, 2));
    SV_HIP(hipMemcpyAsync(ctx->db_img.as<int32_t>() + ctx->db_n, img_of_seg, (size_t)n * 4, hipMemcpyDefault, ctx->stream));
    ctx->db_has_img = true;
    // the largest image id sizes the image -> row map of segvlad_search_shortlist (rebuilt by its next call)
    int mx = -1;
    SV_TRY(sv_img_max(ctx, ctx->db_img.as<int32_t>() + ctx->db_n, n, &mx));
    ctx->db_img_max = std::max(ctx->db_img_max, mx);
  }
  SV_TRY(sv_launch_row_sumsq(ctx, dst, n, d, ctx->db_norms.as<float>() + ctx->db_n));
  ctx->db_n = n_new;
  ctx->db_d = d;
  ctx->db_added = true;
  index_changed(ctx);
  return sv_finish(ctx);
}

// One plane of the index to be compacted: the old buffer, its row pitch in bytes, the surviving rows it takes, and the fresh
// buffer (same tag, guard and persistence) that receives them.
struct PlaneMove {
  DevBuf* old;
  size_t pitch;
  int64_t rows;
  DevBuf fresh;
};

static void release_fresh(std::vector<PlaneMove>& mv) {
  for (auto& m : mv) m.fresh.release();
}

int segvlad_db_remove(segvlad_ctx* ctx, const int64_t* row_ids, int64_t n_row_ids, const int32_t* img_ids, int n_img_ids,
                      int64_t* new_id_out, int64_t* n_removed_out) {
  CHECK_CTX();
  if (n_row_ids < 0 || n_img_ids < 0) return ctx->fail(SEGVLAD_ERR_ARG, "db_remove: negative list length");
  if ((n_row_ids > 0 && !row_ids) || (n_img_ids > 0 && !img_ids)) return ctx->fail(SEGVLAD_ERR_ARG, "db_remove: null id list");
  if (n_img_ids > 0 && !ctx->db_has_img)
    return ctx->fail(SEGVLAD_ERR_STATE, "db_remove: image ids given, but the index holds no img_of_seg map");
  if (n_removed_out) *n_removed_out = 0;
  const int64_t n = ctx->db_n;
  const int d = ctx->db_d;
  if (n == 0 || (n_row_ids == 0 && n_img_ids == 0)) {
    if (n > 0 && new_id_out) {   // nothing listed: every row keeps its id
      void* dn;
      SV_TRY(sv_out(ctx, new_id_out, (size_t)n * 8, &dn));
      std::vector<int64_t> ident(n);
      for (int64_t r = 0; r < n; ++r) ident[r] = r;
      SV_HIP(hipMemcpyAsync(dn, ident.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
      SV_HIP(hipStreamSynchronize(ctx->stream));
    }
    return sv_finish(ctx);
  }
  const void *drow = nullptr, *dimg = nullptr;
  void* dnew = nullptr;
  SV_TRY(sv_in(ctx, row_ids, (size_t)n_row_ids * 8, &drow));
  SV_TRY(sv_in(ctx, img_ids, (size_t)n_img_ids * 4, &dimg));
  if (new_id_out) SV_TRY(sv_out(ctx, new_id_out, (size_t)n * 8, &dnew));
  int64_t cnt[3] = {n, 0, 0};   // n', survivors below db_f16_rows, below db_split_rows
  StageScope sc(ctx, "db_remove");
  int launches = 0;
  SV_TRY(sv_remove_positions(ctx, (const int64_t*)drow, n_row_ids, (const int32_t*)dimg, n_img_ids, (int64_t*)dnew, ctx->db_f16_rows,
                             ctx->db_split_rows, cnt, &launches));
  sc.count(launches);
  const int64_t n_new = cnt[0];
  if (n_removed_out) *n_removed_out = n - n_new;
  if (n_new == n) return sv_finish(ctx);   // (a removal that removes nothing moves nothing)
  // Every destination is reserved before anything is moved: a failed allocation releases the fresh buffers and leaves the index as
  // it was.  The gathers only READ the old planes, so until the swap below the index still describes its old buffers whatever
  // happens; after it nothing can fail.  Peak memory: the old and the new planes together.
  std::vector<PlaneMove> mv;
  mv.push_back({&ctx->db_rows, (size_t)d * 4, n_new, {}});
  mv.push_back({&ctx->db_norms, 4, n_new, {}});
  if (ctx->db_has_img) mv.push_back({&ctx->db_img, 4, n_new, {}});
  if (ctx->db_f16_rows > 0) mv.push_back({&ctx->db_f16, (size_t)d * 2, cnt[1], {}});
  if (ctx->db_split_rows > 0) {
    mv.push_back({&ctx->db_hi, (size_t)d * 2, cnt[2], {}});
    mv.push_back({&ctx->db_lo, (size_t)d * 2, cnt[2], {}});
  }
  for (auto& m : mv) {
    m.fresh.tag = m.old->tag;
    m.fresh.guard = m.old->guard;
    m.fresh.fixed = m.old->fixed;
    if (m.rows <= 0) continue;
    const hipError_t e = m.fresh.reserve((size_t)m.rows * m.pitch);
    if (e != hipSuccess) {
      release_fresh(mv);
      return ctx->fail(e == hipErrorOutOfMemory ? SEGVLAD_ERR_NOMEM : SEGVLAD_ERR_HIP,
                       "db_remove: reserving %zu bytes for %s: %s (the index is unchanged)", (size_t)m.rows * m.pitch, m.old->tag,
                       hipGetErrorString(e));
    }
  }
  for (auto& m : mv) {
    if (m.rows <= 0) continue;
    const int rc = sv_launch_remove_gather(ctx, m.old->p, m.fresh.p, m.pitch, m.rows);
    if (rc != SEGVLAD_OK) {
      (void)hipStreamSynchronize(ctx->stream);
      release_fresh(mv);
      return rc;
    }
    sc.count();
  }
  const hipError_t e = hipStreamSynchronize(ctx->stream);   // (the gathers have read the old planes)
  if (e != hipSuccess) {
    release_fresh(mv);
    return ctx->fail(SEGVLAD_ERR_HIP, "db_remove: the gathers failed: %s (the index is unchanged)", hipGetErrorString(e));
  }
  for (auto& m : mv) {
    m.old->release();
    *m.old = m.fresh;
  }
  // the surviving rows keep their order, so the planes' prefixes stay valid; the fp16 scale still bounds every surviving row.  The max
  // row norm is recomputed from the compacted norms by the next search that needs it (prepare_index_planes: exact, as a fresh index's)
  ctx->db_n = n_new;
  ctx->db_f16_rows = cnt[1];
  ctx->db_split_rows = cnt[2];
  ctx->db_rn_max = 0.f;
  ctx->db_rn_max_rows = 0;
  if (n_new == 0) {
    ctx->db_f16_scale = 0.f;
    ctx->db_maxabs = 0.f;
  }
  index_changed(ctx);
  return sv_finish(ctx);
}

int segvlad_db_size(segvlad_ctx* ctx, int64_t* n_rows, int* d) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  if (n_rows) *n_rows = ctx->db_n;
  if (d) *d = ctx->db_d;
  return SEGVLAD_OK;
}

int segvlad_search_stats(segvlad_ctx* ctx, int64_t* stats_out, int n) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  if (!stats_out || n < 0) return ctx->fail(SEGVLAD_ERR_ARG, "search_stats: bad arguments");
  if (ctx->tail_stats_dev) {   // the last search was a device-driven pass: its tail's counters are still on the device
    uint32_t h[4] = {0, 0, 0, 0};
    (void)hipSetDevice(ctx->device);
    SV_HIP(hipStreamSynchronize(ctx->stream));
    SV_HIP(hipMemcpy(h, ctx->tail_stats_dev, sizeof(h), hipMemcpyDeviceToHost));
    ctx->sstats.n_redo = h[0];      // rows redone exactly (brute force on the device)
    ctx->sstats.n_refine2 = h[1];   // rows refined from their candidate lists (second tier)
    ctx->tail_stats_dev = nullptr;
  }
  const SvSearchStats& t = ctx->sstats;
  const int64_t v[13] = {t.levels, t.filter, t.n_fallback, t.cand_max, t.cand_sum, t.refine_max, t.refine_sum, t.n_queries, t.n_redo, t.n_refine2,
                         t.grp_groups, t.grp_union_sum, t.carry_rows};
  for (int j = 0; j < n && j < 13; ++j) stats_out[j] = v[j];
  return SEGVLAD_OK;
}

}  // extern "C"

// Exact search.  Small databases: distance matrix + radix select.  Large ones: a strided 1/16^L sample gives an
// exact UPPER bound T0[q] of the k-th smallest distance; each finer level re-runs the distance GEMM with the
// epilogue keeping only entries <= T[q] (about 16 k per query), whose exact top-k tightens T for the next level;
// the last level covers every row, so the final top-k is exact (ties included: all entries <= T are candidates
// and the final order is (distance, id)).  A query whose candidate or refine list overflows (adversarial data) is
// redone -- alone -- on the matrix path; the other queries keep their filtered result.
static int search_matrix(segvlad_ctx* ctx, const float* dq, int m, int64_t n, int d, int k, const float* qn, float* dd2,
                         int64_t* didx) {
  const int64_t ld = (n + 3) & ~3ll;
  int64_t rows = ld > 0 ? (int64_t)(2ll << 30) / (ld * 4) : m;
  if (rows < 128) rows = 128;
  if (rows > m) rows = m;
  SV_HIP(ctx->s_dist.reserve((size_t)rows * (ld > 0 ? ld : 1) * 4));
  for (int64_t q0 = 0; q0 < m; q0 += rows) {
    const int mm = (int)((m - q0 < rows) ? (m - q0) : rows);
    {
      StageScope sc(ctx, "knn_gemm");
      SV_TRY(sv_launch_gemm_nt(ctx, 1, dq + (size_t)q0 * d, ctx->db_rows.as<float>(), ctx->s_dist.as<float>(), mm, (int)n, d,
                               ld, nullptr, nullptr, qn + q0, ctx->db_norms.as<float>()));
      sc.count();
    }
    {
      StageScope sc(ctx, "knn_select");
      SV_TRY(sv_launch_select_topk(ctx, ctx->s_dist.as<float>(), ld, mm, n, k, dd2 + (size_t)q0 * k, didx + (size_t)q0 * k, k, 0));
      sc.count();
    }
  }
  return SEGVLAD_OK;
}

// rows of the redo / overflow passes: gather flagged query rows into a dense block, scatter their results back (C linkage:
// their symbols are the plain kernel names)
extern "C" {
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ X, const float* __restrict__ xn,
                                                          const int32_t* __restrict__ rows, int d, float* __restrict__ Y,
                                                          float* __restrict__ yn) {
  const int r = blockIdx.x;
  const int64_t src = rows[r];
  for (int j = threadIdx.x; j < d; j += 256) Y[(int64_t)r * d + j] = X[src * d + j];
  if (threadIdx.x == 0) yn[r] = xn[src];
}
__global__ __launch_bounds__(256) void scatter_topk_kernel(const float* __restrict__ d2, const int64_t* __restrict__ idx,
                                                           const int32_t* __restrict__ rows, int k, float* __restrict__ d2_out,
                                                           int64_t* __restrict__ idx_out) {
  const int r = blockIdx.x;
  const int64_t dst = rows[r];
  for (int j = threadIdx.x; j < k; j += 256) {
    d2_out[dst * k + j] = d2[(int64_t)r * k + j];
    idx_out[dst * k + j] = idx[(int64_t)r * k + j];
  }
}
// The last kernel of every search (segvlad.h, "Non-finite rows"): a pair whose distance is not < +inf is never listed.  Such
// values sort behind every finite one (sv_d2 turns a NaN into +inf), so they are the tail of a list: their slots become
// (+inf, -1), and so does every slot of a query row whose squared norm is not finite -- a row holding NaN or Inf, whatever the
// passes before made of it.
__global__ __launch_bounds__(256) void unlisted_slots_kernel(const float* __restrict__ qn, int64_t total, int k, float* __restrict__ d2,
                                                             int64_t* __restrict__ idx) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  const bool bad_row = !(fabsf(qn[j / k]) < INFINITY);
  if (bad_row || !(d2[j] < INFINITY)) {
    d2[j] = INFINITY;
    idx[j] = -1;
  }
}
}  // extern "C"

static int unlist_nonfinite(segvlad_ctx* ctx, const float* qn, int nq, int k, float* d2, int64_t* idx) {
  const int64_t total = (int64_t)nq * k;
  StageScope sc(ctx, "knn_select");
  hipLaunchKernelGGL(unlisted_slots_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, qn, total, k, d2, idx);
  SV_HIP(hipGetLastError());
  sc.count();
  return SEGVLAD_OK;
}

// ---- the search plan ----------------------------------------------------------------------------------------------
constexpr int SV_RATIO = 16, SV_CAP = 8192, SV_RCAP = 512, SV_CHUNK = 16384;
constexpr double SV_PFAIL = 2e-5;   // heur_rank_small's tolerance (one redone query in ~1000 passes of 50)

// Smallest rank r such that a threshold at the r-th smallest value of a 1/16 sample admits, 4 sigma below its
// expectation 16 r, still `target` values of the full set (relative spread of the r-th order statistic ~ 1/sqrt(r)).
static int heur_rank(int target) {
  int r = 16;
  while (16.0 * r - 64.0 * std::sqrt((double)r) < (double)target) ++r;
  return r;
}

// The same question for a sample `ratio` times smaller and SMALL ranks, where the normal approximation is off: the
// number of full-set values below the r-th smallest sample value is ~ ratio * Gamma(r, 1), so take the smallest r with
// P[Gamma(r, 1) < target / ratio] < pfail (2e-5: one redo in ~1000 passes of 50 queries).
static int heur_rank_small(int target, int ratio, double pfail) {
  const double x = (double)target / ratio, ex = std::exp(-x);
  double term = 1.0, sum = 0.0;   // sum_{i < r} x^i / i!
  for (int r = 1; r < target; ++r) {
    sum += term;
    term *= x / r;
    if (r >= 2 && 1.0 - ex * sum < pfail) return r;
  }
  return target;
}

// power-of-two scale that puts the largest magnitude in [8192, 16384): no overflow, negligible underflow
static float pow2_scale(float maxabs) {
  if (!(maxabs > 0.f) || !std::isfinite(maxabs)) return 1.f;
  int e;
  frexpf(maxabs, &e);  // maxabs = m * 2^e, m in [0.5, 1)
  return ldexpf(1.f, 14 - e);
}

// Filter arithmetic (option knn_filter, see SvOptions); the values are search_stats' `filter` field.
enum class Filter { F16 = 1, BF16X3 = 2, FP32 = 3 };

// How the queries are made ready for the pass (prepare_queries):
//   Fp32             norms only
//   Bf16Split        the bf16 hi / lo planes
//   SmallHead        one query image: small_head_kernel -- plane, scale, norms, flags AND level 0 in one launch
//   SmallF16         one query image: query_f16_small_kernel -- plane and scale on the device, flags (and norms when aligned)
//   BatchF16         batches: the query scale read back, then the plane
//   BatchF16EarlyL0  the same, with level 0 of the first chunk enqueued before the host waits for the scale
enum class Prep { Fp32, Bf16Split, SmallHead, SmallF16, BatchF16, BatchF16EarlyL0 };

// One pass of the level scheme: an exact (or, guessed, fp16) level 0 over rows 0, stride0, 2 stride0, ..., then `levels`
// filter GEMMs over samples 16x larger each (ratio_last into the last one), the last one covering every row, then the exact
// refinement.
//   rigorous : every threshold is the k-th smallest distance of the previous (coarser) sample -- an UPPER bound of
//              the k-th smallest of the finer one, so no true neighbour is ever dropped; ~16 k candidates per level.
//   guessed  : thresholds at much lower ranks r_j (heur_rank) that admit ~16 r_j candidates -- 5-10x fewer -- and are
//              verified afterwards: a level whose list holds fewer than r_{j+1} entries, or a final list whose k-th
//              smallest approximate distance A_k exceeds the threshold T it was collected under (then {d2~ <= A_k + 2 eps}
//              might not be contained in the collected {d2~ <= T + 2 eps}), flags the query; flagged queries are redone
//              with the rigorous thresholds.  Exactness never depends on the ranks; they only decide how often the redo runs.
struct Schedule {
  int levels = 0;          // filter levels after level 0
  int64_t stride0 = 1;     // stride of level 0's sample (16^levels)
  int ratio_last = SV_RATIO;   // sample growth into the LAST (full) level; the levels before it grow by SV_RATIO
  bool guessed = false;
  bool device_tail = false;    // the pass ends in small_tail_kernel on the device, without a read-back
  int rank[8] = {};        // rank[j]: rank of the threshold handed to level j + 1; rank[levels] = k (the final top-k)
};

struct SearchPlan {
  int nq = 0, d = 0, k = 0;
  int64_t n = 0;
  bool matrix = false;     // a small index: distance matrix + select, nothing below applies
  Filter filter = Filter::FP32;
  Schedule rigorous;       // the redo's (and, without guessed thresholds, the pass's)
  Schedule pass;           // the main pass's
  Prep prep = Prep::Fp32;
  bool fuse_qn = false;    // the single-image preparation kernel writes the norms too
  bool q2min = false;      // batches: min ||q||^2 read back with the scale (the biased-accumulator kernel's margin)
  int mrows = 0;           // rows of one chunk: per-chunk scratch is sized for min(nq, SV_CHUNK)
};

static void set_ranks(Schedule& s, int k) {
  s.rank[s.levels] = k;
  for (int j = s.levels - 1; j >= 0; --j) {
    const int ratio = (j + 1 == s.levels) ? s.ratio_last : SV_RATIO;   // growth from level j's sample to level j + 1's
    s.rank[j] = !s.guessed ? k
                           : std::min(s.rank[j + 1], ratio == SV_RATIO ? heur_rank(s.rank[j + 1]) : heur_rank_small(s.rank[j + 1], ratio, SV_PFAIL));
  }
}

// Every decision that depends on the call alone (shape, options, index state, the query pointer's alignment).
static SearchPlan plan_search(const segvlad_ctx* ctx, int nq, int k, const void* dq) {
  const SvOptions& o = ctx->opt;
  const int d = ctx->db_d;
  const int64_t n = ctx->db_n;
  SearchPlan p{nq, d, k, n};
  // Rigorous plan: strides 16^L, ..., 16, 1.  Level 0 goes through the exact fp32 matrix path (an order of magnitude dearer per
  // row than the fp16 filter), so take as many levels as keep it selective: a sample of s rows admits a fraction k/s of the next
  // level, which must stay below the filter's per-wave list capacity (25 % of a block) -> s >= 4.8 k.  Databases of <= 32768 rows
  // keep the plain matrix path; the sample never exceeds 32768 rows.  (Row shards of 250 k - 500 k rows -- the 1 M-row database
  // on 2 or 4 GPUs -- get two levels instead of a 15 k - 31 k row exact level.)
  Schedule& rig = p.rigorous;
  if (n > 32768) {
    const int64_t want = std::max<int64_t>((24 * (int64_t)k + 4) / 5, 512);
    while (n / (rig.stride0 * SV_RATIO) >= want) {
      rig.stride0 *= SV_RATIO;
      ++rig.levels;
    }
    while (n / rig.stride0 > 32768) {
      rig.stride0 *= SV_RATIO;
      ++rig.levels;
    }
  }
  p.matrix = rig.levels == 0 || n / rig.stride0 < 4 * (int64_t)k;
  if (p.matrix) return p;
  // "f16" = one fp16 product (d % 64 == 0), "bf16x3" = three bf16 products (d % 32 == 0), else plain fp32
  const bool f16 = (o.knn_filter == 0 || o.knn_filter == 1) && d % 64 == 0;
  const bool bf16 = !f16 && o.knn_filter != 3 && d % 32 == 0;
  p.filter = f16 ? Filter::F16 : bf16 ? Filter::BF16X3 : Filter::FP32;
  // The guessed ("heuristic") thresholds need only a few dozen sample rows per rank, so their plan goes deeper: level 0 (an order
  // of magnitude dearer per row than a filter level) shrinks to >= 192 rows -- 1 M rows: strides 4096, 256, 16, 1 instead of
  // 256, 16, 1 (0.9 ms of exact GEMM per 10 000 queries -> 0.06 ms); a 125 k-row shard: 256, 16, 1 instead of 16, 1
  // (1.35 -> 0.1 ms).  The rigorous redo keeps the plan above.
  const bool guessed = p.filter != Filter::FP32 && o.knn_heuristic && !ctx->db_heur_off && heur_rank(k) < k;
  Schedule& s = p.pass;
  s = rig;
  s.guessed = guessed;
  // One query image per pass (<= 128 rows) is bound by its chain of dependent launches, not by level 0's flops (option
  // small_plan): ONE filter level behind a sample of 2048..4096 rows (stride = the power of two that gives it: 256 for 1 M rows,
  // 64 for a 250 k-row shard).  The threshold is a low rank of that sample (heur_rank_small: ~7 at stride 256), the full level
  // collects stride x rank candidates per query (~1800 + the margin's ~900 at 1 M rows: a workgroup select's worth, SV_CAP
  // bounds it -- hence stride <= 512).  (The same last step for batches -- strides 4096, 256, 1 instead of 4096, 256, 16, 1 --
  // was measured and dropped: the stride-16 level's 1.3 ms come back as epilogue time of the full level, which then collects
  // 2900 candidates per query instead of 780, and as 0.2 ms of longer selects.)
  int small_stride = 16;
  while ((n + small_stride - 1) / small_stride > 4096 && small_stride <= 512) small_stride *= 2;
  const bool small = guessed && nq <= 128 && o.small_plan && small_stride <= 512;
  if (small) {
    s.levels = 1;
    s.stride0 = small_stride;
    s.ratio_last = small_stride;
  } else if (guessed) {
    while (s.levels < 6 && n / (s.stride0 * SV_RATIO) >= 192) {
      s.stride0 *= SV_RATIO;
      ++s.levels;
    }
  }
  set_ranks(rig, k);
  set_ranks(s, k);
  p.mrows = std::min(nq, SV_CHUNK);
  const int64_t n0 = (n + s.stride0 - 1) / s.stride0;
  if (p.filter == Filter::F16) {
    if (nq <= 128 && (((int64_t)nq * d) & 3) == 0 && (int64_t)nq * d <= (1 << 18)) {
      // one query image per pass: the scale is computed AND consumed on the device (a host round trip in front of every pass was
      // ~45 us of a ~600 us call).  One workgroup reads the block twice: up to 1 MiB of queries (128 x 2048 floats); deeper rows
      // (raw K*D descriptors) keep the many-workgroup kernels and their read-back.
      p.fuse_qn = (reinterpret_cast<uintptr_t>(dq) & 15) == 0;   // (d % 64 == 0 on this path)
      const bool head = small && p.fuse_qn && o.small_head && o.debug_search == 0 && n0 <= 4096 && sv_small_head_ok(nq, d, (int)n0, s.rank[0]);
      p.prep = head ? Prep::SmallHead : Prep::SmallF16;
      // option small_tail = 0: the read-back of rounds 3-5, for A/B and for the tests that compare the two
      s.device_tail = small && o.small_tail && o.debug_search == 0 && n <= 0xffffffffLL;
    } else {
      // batches on the default configuration take the biased-accumulator kernel when the norms allow it: min ||q||^2
      p.q2min = sv_f16_bias_possible(o, nq);
      // level 0 of the first chunk goes out BEFORE the host waits for the scale: it needs neither the query plane nor the margin,
      // and the device runs it during the round trip -- not when level 0 runs on the fp16 product (batch_l0_f16: that needs the
      // plane; it is ten times cheaper than the exact GEMM it replaces, which is worth more than hiding that GEMM)
      p.prep = p.q2min && guessed && o.debug_search == 0 && !(o.batch_l0_f16 && n0 <= 4096) ? Prep::BatchF16EarlyL0 : Prep::BatchF16;
    }
  } else {
    p.prep = p.filter == Filter::BF16X3 ? Prep::Bf16Split : Prep::Fp32;
  }
  return p;
}

// Values measured on the call's data: the filter's margin |d2~ - d2| <= c_eps ||q|| ||r|| (rn_max = max ||r||^2), the fp16
// product's 1 / (query scale x index scale) and the query scale.  Level 0 of a batch's first chunk runs before they are known,
// with the defaults.
struct PassScalars {
  float c_eps = 0.f, inv_scale = 1.f, rn_max = 0.f, qscale = 1.f;
  float qmax = 0.f;   // batch preparations: max |q| over the finite entries, or NaN when a query holds NaN / Inf (segvlad_range_search looks at it)
};

// Flag block of one pass: [nrows] row flags, 2 counts (flagged rows, second-tier rows: ONE read-back per chunk), [mrows]
// second-tier flags of the current chunk; the main pass's block adds the device-driven tail's 4 counters and is a whole number
// of 256-byte blocks (one fill).  `flagged` / `tier2_seen`: the host's copies of the two counts after the last read-back.
struct FlagBlock {
  DevBuf* buf;
  int nrows, mrows;
  bool main;
  uint32_t flagged = 0, tier2_seen = 0;
  size_t bytes() const {
    const size_t b = ((size_t)nrows + 2 + mrows + (main ? 4 : 0)) * 4;
    return main ? (b + 255) & ~(size_t)255 : b;
  }
  uint32_t* rows() const { return buf->as<uint32_t>(); }
  uint32_t* count() const { return rows() + nrows; }
  uint32_t* tier2() const { return count() + 2; }
  uint32_t* tail() const { return tier2() + mrows; }
};

// Up to SV_CHUNK query rows of a pass: fp32 rows, 16-bit planes (f16: plane, null; bf16x3: hi, lo), squared norms, outputs,
// and rows [row0, row0 + m) of the pass's flag block.
struct Chunk {
  const float* q;
  const uint16_t *qa, *qb;
  const float* qn;
  int m;
  float* d2;
  int64_t* idx;
  FlagBlock* fb;
  int row0;
  std::vector<uint32_t> host;   // list lengths read back for search_stats / debug_search
  uint32_t* flags() const { return fb->rows() + row0; }
};

// What every select of a chunk is handed: the candidate lists, the margin, the refine list, the flag and second-tier words.
// The caller sets mode, k, check, the thresholds in and out.
static SvSelectArgs select_args(segvlad_ctx* ctx, const Chunk& c, const PassScalars& v) {
  SvSelectArgs a;
  a.cnt = ctx->s_cand_cnt.as<uint32_t>();
  a.cd2 = ctx->s_cand_d2.as<float>();
  a.cid = ctx->s_cand_id.as<uint32_t>();
  a.cap = SV_CAP;
  a.qn = c.qn;
  a.c_eps = v.c_eps;
  a.rn_max = v.rn_max;
  a.ref_cnt = ctx->s_ref_cnt.as<uint32_t>();
  a.ref_id = ctx->s_ref_id.as<uint32_t>();
  a.rcap = SV_RCAP;
  a.ovf_rows = c.flags();
  a.ovf_count = c.fb->count();
  a.rovf_rows = c.fb->tier2();
  a.rovf_count = c.fb->count() + 1;
  a.ref_lim = ctx->s_ref_lim.as<float>();
  return a;
}

// ---- one chunk: level 0, the filter levels, the finish -------------------------------------------------------------
// Level 0's form:
//   SplitReduce  one query image: the K split's reduction and the rank select in ONE launch (l0_reduce_rank_kernel)
//   FilterLists  deep rows, guessed: the sample through the filter kernel under +inf thresholds, ranked like any level's lists
//   SampleF16    batches, guessed: the sample from the filter's own fp16 product
//   ExactGemm    exact fp32 distances to the sample
enum class Level0 { SplitReduce, FilterLists, SampleF16, ExactGemm };

// The decisions that depend on the chunk's row count: a batch's last chunk and the redo of a few rows take the small-m forms.
struct ChunkPath {
  int64_t n0, ld0;      // level 0's sample rows, and its distance block's row stride
  bool short_sample;    // n0 <= 4096 on an approximate filter: level 0 leaves one threshold per row
  Level0 l0;
  int64_t n_comp;       // rows that are not multiples of 16
  bool carry;           // the last level runs over those n_comp rows only, the stride-16 level's survivors stay in the lists
  bool grouped;         // refinement by bands of 32 query rows over their union (refine_group_kernels.hip)
  bool grouped_tier2;   // the second tier as its own union GEMM (deep rows)
};

static ChunkPath chunk_path(const segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, int m) {
  const SvOptions& o = ctx->opt;
  const bool batch = m > 128;
  const bool f16_guess = s.guessed && p.filter == Filter::F16;
  ChunkPath c;
  c.n0 = (p.n + s.stride0 - 1) / s.stride0;
  c.ld0 = (c.n0 + 3) & ~3ll;
  c.short_sample = c.n0 <= 4096 && p.filter != Filter::FP32;
  if (!batch && c.short_sample)
    c.l0 = Level0::SplitReduce;
  else if (f16_guess && batch && c.n0 <= 4096 && o.batch_l0_f16)
    // deep rows (raw K*D descriptors): the no-LDS sample kernel re-reads the query plane (2 GB at 10 000 x 98 304: not L2
    // resident) once per 32 sample rows: 8.5 ms for 196 rows, against ~0.6 ms at the filter's rate
    c.l0 = sv_f16_kblock(o, p.d) && o.batch_l0_f16 != 2 ? Level0::FilterLists : Level0::SampleF16;
  else
    c.l0 = Level0::ExactGemm;
  // carry: the stride-16 level's filter has already evaluated 1/16 of the rows with the arithmetic of the last level; its
  // survivors under the NEXT threshold stay in the lists (SvSelect::Carry).  Guessed thresholds only (every level collects under
  // thr + 2 eps there, so the kept set is exactly what the last level would append).
  c.n_comp = p.n - (p.n + SV_RATIO - 1) / SV_RATIO;
  c.carry = f16_guess && s.levels >= 2 && s.ratio_last == SV_RATIO && batch && c.n_comp < 0x7fffffffLL &&
            sv_f16_filter_skip_ok(ctx, m, c.n_comp, p.d);
  c.grouped = batch;
  c.grouped_tier2 = batch && p.d > 4096;
  return c;
}

// The thresholds level lv's filter reads (and its select checks against): level 0's, or the previous select's.
struct LevelThr { const float* p; int64_t ld; float eps_mult; };
static LevelThr level_thr(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const ChunkPath& cp, int lv) {
  float* thr = ctx->s_thr_d2.as<float>();
  // level 0: exact distances need one margin (rigorous), guessed ones the collected set to reach 2 eps beyond them
  if (lv == 1) return cp.short_sample ? LevelThr{thr, 1, s.guessed ? 2.f : 1.f} : LevelThr{thr + (s.rank[0] - 1), s.rank[0], s.guessed ? 2.f : 1.f};
  // approximate filters: rank-th approximate distances A_r -- the exact one is <= A_r + eps, and any row at least that close
  // has d2~ <= A_r + 2 eps; fp32: the select's exact top-k
  if (p.filter != Filter::FP32) return LevelThr{thr, 1, 2.f};
  return LevelThr{thr + (p.k - 1), p.k, 2.f};
}

// list lengths cnt[0, m) for search_stats / debug_search (synchronises)
struct Occupancy { uint64_t sum = 0; uint32_t max = 0, over = 0; };
static int read_counts(segvlad_ctx* ctx, const DevBuf& cnt, int m, std::vector<uint32_t>& h, Occupancy* o) {
  h.resize(m);
  SV_HIP(hipStreamSynchronize(ctx->stream));
  SV_HIP(hipMemcpy(h.data(), cnt.p, (size_t)m * 4, hipMemcpyDeviceToHost));
  for (uint32_t c : h) {
    o->sum += c;
    o->max = std::max(o->max, c);
    o->over += c > (uint32_t)SV_CAP;
  }
  return SEGVLAD_OK;
}

// Level 0: the sample's thresholds thr[q] (rank[0]-th smallest distance).
static int level0(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const PassScalars& v, Chunk& c, const ChunkPath& cp) {
  const int m = c.m, d = p.d, r0 = s.rank[0];
  const float* R = ctx->db_rows.as<float>();
  const float* rn = ctx->db_norms.as<float>();
  float* thr = ctx->s_thr_d2.as<float>();
  bool fused = false;
  {
    StageScope sc(ctx, "knn_level0");   // its own stage: "knn_gemm" then times the filter kernel's launches only
    if (cp.l0 == Level0::SplitReduce) {
      const float* parts = nullptr;
      int splits = 1;
      SV_TRY(sv_launch_l2_strided_parts(ctx, c.q, R, ctx->s_dist.as<float>(), m, (int)cp.n0, d, cp.ld0, c.qn, rn, (int)s.stride0, &parts,
                                        &splits));
      if (splits > 1) {
        SV_TRY(sv_launch_l0_reduce_rank(ctx, parts, splits, m, (int)cp.n0, cp.ld0, c.qn, rn, (int)s.stride0, r0, thr,
                                        ctx->s_cand_cnt.as<uint32_t>(), c.flags()));
        fused = true;
      }
    } else if (cp.l0 == Level0::FilterLists) {
      SV_HIP(hipMemsetD32Async((hipDeviceptr_t)thr, 0x7f800000, (size_t)m, ctx->stream));
      SV_HIP(hipMemsetAsync(ctx->s_cand_cnt.p, 0, (size_t)m * 4, ctx->stream));
      SV_TRY(sv_launch_f16_filter(ctx, c.qa, ctx->db_f16.as<uint16_t>(), m, (int)cp.n0, d, (int)s.stride0, v.inv_scale, c.qn, rn, thr, 1,
                                  2.f, v.c_eps, v.rn_max, ctx->s_cand_cnt.as<uint32_t>(), ctx->s_cand_d2.as<float>(),
                                  ctx->s_cand_id.as<uint32_t>(), SV_CAP));
    } else if (cp.l0 == Level0::SampleF16) {
      // a guessed threshold needs no exact distances: the thresholds are then approximate-domain values like every later level's
      SV_TRY(sv_launch_sample_f16_batch(ctx, c.qa, ctx->db_f16.as<uint16_t>(), m, (int)cp.n0, d, s.stride0, v.inv_scale, c.qn, rn,
                                        ctx->s_dist.as<float>(), cp.ld0));
    } else {
      SV_TRY(sv_launch_l2_strided(ctx, c.q, R, ctx->s_dist.as<float>(), m, (int)cp.n0, d, cp.ld0, c.qn, rn, (int)s.stride0, true));
    }
    sc.count(fused ? 2 : 1);
  }
  StageScope sc(ctx, "knn_select");
  if (fused) return SEGVLAD_OK;   // (thr[q] is in place)
  if (cp.l0 == Level0::FilterLists || cp.short_sample) {
    SvSelectArgs a = select_args(ctx, c, v);
    a.mode = SvSelect::Threshold;
    a.k = r0;
    a.thr_out = thr;
    if (cp.l0 == Level0::FilterLists) {
      a.check = 1;
    } else {
      // a short sample row: only its r0-th smallest distance is needed -- the wave-per-query register select of the candidate
      // lists, the distance block standing in for a list of n0 entries
      a.cd2 = ctx->s_dist.as<float>();
      a.cap = (int)cp.ld0;
      a.fixed_cnt = (int)cp.n0;
    }
    SV_TRY(sv_launch_select_approx(ctx, m, a));
  } else {
    SV_TRY(sv_launch_select_topk(ctx, ctx->s_dist.as<float>(), cp.ld0, m, cp.n0, r0, thr, ctx->s_thr_idx.as<int64_t>(), r0, 0));
  }
  sc.count();
  return SEGVLAD_OK;
}

// Levels 1 .. levels: each one's filter GEMM under the previous level's thresholds and the select that ranks its lists into the
// next level's thresholds.  The fp32 filter's last select is the chunk's top-k (the flag count is read back behind it); the
// approximate filters' last lists are left to finish().
static int filter_levels(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const PassScalars& v, Chunk& c, const ChunkPath& cp) {
  const int m = c.m, d = p.d;
  const float* rn = ctx->db_norms.as<float>();
  float* thr = ctx->s_thr_d2.as<float>();
  uint32_t* cand_cnt = ctx->s_cand_cnt.as<uint32_t>();
  float* cand_d2 = ctx->s_cand_d2.as<float>();
  uint32_t* cand_id = ctx->s_cand_id.as<uint32_t>();
  if (cp.carry) ctx->sstats.carry_rows = p.n - cp.n_comp;
  int64_t stride = s.stride0;
  for (int lv = 1; lv <= s.levels; ++lv) {
    const bool last = lv == s.levels;
    stride /= last ? s.ratio_last : SV_RATIO;
    const int64_t ns = (last && cp.carry) ? cp.n_comp : (p.n + stride - 1) / stride;
    const LevelThr t = level_thr(ctx, p, s, cp, lv);
    // the candidate counters start every level at zero: the mode-0 selects of the approximate-domain filters leave them so;
    // only the first filter level behind a select_topk level 0, and the fp32 filter's select, need the memset
    if (p.filter == Filter::FP32 || (lv == 1 && !cp.short_sample)) SV_HIP(hipMemsetAsync(ctx->s_cand_cnt.p, 0, (size_t)m * 4, ctx->stream));
    if (p.filter == Filter::FP32) {
      {
        StageScope sc(ctx, "knn_gemm");
        SV_TRY(sv_launch_l2_filter(ctx, c.q, ctx->db_rows.as<float>(), m, (int)ns, d, c.qn, rn, (int)stride, t.p, t.ld, cand_cnt, cand_d2,
                                   cand_id, SV_CAP));
        sc.count();
      }
      StageScope sc(ctx, "knn_select");
      // the filter pass has consumed thr; the select may overwrite it with the tighter thresholds -- or, last, write the top-k
      SV_TRY(sv_launch_select_cand(ctx, cand_cnt, cand_d2, cand_id, m, SV_CAP, p.k, last ? c.d2 : thr, last ? c.idx : nullptr, c.flags(),
                                   c.fb->count()));
      sc.count();
      if (last) {
        SV_HIP(hipMemcpyAsync(&c.fb->flagged, c.fb->count(), 4, hipMemcpyDeviceToHost, ctx->stream));
        SV_HIP(hipStreamSynchronize(ctx->stream));
      }
      continue;
    }
    {
      StageScope sc(ctx, "knn_gemm");
      if (p.filter == Filter::F16)
        SV_TRY(sv_launch_f16_filter(ctx, c.qa, ctx->db_f16.as<uint16_t>(), m, (int)ns, d, (int)stride, v.inv_scale, c.qn, rn, t.p, t.ld,
                                    t.eps_mult, v.c_eps, v.rn_max, cand_cnt, cand_d2, cand_id, SV_CAP, (last && cp.carry) ? SV_RATIO : 0));
      else
        SV_TRY(sv_launch_bf16_filter(ctx, c.qa, c.qb, ctx->db_hi.as<uint16_t>(), ctx->db_lo.as<uint16_t>(), m, (int)ns, d, (int)stride,
                                     c.qn, rn, t.p, t.ld, t.eps_mult, v.c_eps, v.rn_max, cand_cnt, cand_d2, cand_id, SV_CAP));
      sc.count();
    }
    if (ctx->opt.debug_search || (ctx->opt.search_stats && last)) {
      Occupancy o;
      SV_TRY(read_counts(ctx, ctx->s_cand_cnt, m, c.host, &o));
      if (last) {
        ctx->sstats.cand_sum += (int64_t)o.sum;
        ctx->sstats.cand_max = std::max<int64_t>(ctx->sstats.cand_max, o.max);
      }
      if (ctx->opt.debug_search)
        fprintf(stderr, "[search] %s m=%d level %d/%d ns=%lld rank %d: candidates mean %.1f max %u, %u lists over cap %d\n",
                s.guessed ? "heuristic" : "rigorous", m, lv, s.levels, (long long)ns, s.rank[lv], (double)o.sum / m, o.max, o.over, SV_CAP);
    }
    if (last) break;
    StageScope sc(ctx, "knn_select");
    SvSelectArgs a = select_args(ctx, c, v);
    a.mode = (cp.carry && lv + 1 == s.levels) ? SvSelect::Carry : SvSelect::Threshold;
    a.k = s.rank[lv];
    a.check = s.guessed ? 1 : 0;
    a.thr_in = t.p;
    a.thr_in_ld = t.ld;
    a.thr_out = thr;
    SV_TRY(sv_launch_select_approx(ctx, m, a));
    sc.count();
  }
  return SEGVLAD_OK;
}

// Approximate filters: from the last level's candidate lists to the chunk's exact top-k -- the final select, the refinement,
// and either the device-driven tail or the read-back of the flag counts with the second tier of this chunk's rows.
static int finish(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const PassScalars& v, Chunk& c, const ChunkPath& cp) {
  const int m = c.m, d = p.d, k = p.k;
  const float* R = ctx->db_rows.as<float>();
  const float* rn = ctx->db_norms.as<float>();
  uint32_t* cand_cnt = ctx->s_cand_cnt.as<uint32_t>();
  float* cand_d2 = ctx->s_cand_d2.as<float>();
  uint32_t* cand_id = ctx->s_cand_id.as<uint32_t>();
  FlagBlock& fb = *c.fb;
  const LevelThr t = level_thr(ctx, p, s, cp, s.levels);
  uint32_t* tier2 = fb.tier2();
  float* ref_lim = ctx->s_ref_lim.as<float>();
  const uint32_t* poison_dev = nullptr;   // see sv_launch_refine_exact
  bool tail_fused = false;                // the refinement kernel finished the flagged rows itself (no small_tail_kernel)
  {
    StageScope sc(ctx, "knn_select");
    SvSelectArgs a = select_args(ctx, c, v);
    a.mode = SvSelect::Band;
    a.k = k;
    a.check = s.guessed ? 1 : 0;
    a.thr_in = t.p;
    a.thr_in_ld = t.ld;
    a.thr_out = ctx->s_thr_d2.as<float>();
    SV_TRY(sv_launch_select_approx(ctx, m, a));
    sc.count();
    if (cp.grouped) {
      // batches: bands of 32 consecutive query rows (the segments of an image) over the union of their rows where they
      // overlap, the rest row by row (refine_group_kernels.hip); same bits either way
      int nl = 0;
      SV_TRY(sv_launch_refine_grouped(ctx, c.q, R, m, d, c.qn, rn, ctx->s_ref_cnt.as<uint32_t>(), ctx->s_ref_id.as<uint32_t>(), SV_RCAP, k,
                                      c.d2, c.idx, &nl));
      sc.count(nl);
      if (ctx->opt.search_stats && nl > 1) {
        int64_t ng = 0, gg = 0, us = 0;
        SV_TRY(sv_refine_group_stats(ctx, m, &ng, &gg, &us));
        ctx->sstats.grp_groups += gg;
        ctx->sstats.grp_union_sum += us;
      }
    } else {
      // a device-driven pass whose head was small_head_kernel (it repairs a poisoned hand-over buffer): the refinement finishes the
      // flagged rows itself -- no small_tail_kernel behind it (a kernel boundary of 4-5 us, whatever the kernel does)
      SvSmallFinish fz;
      if (s.device_tail && ctx->small_head_ran && ctx->opt.small_tail != 2) {
        fz.on = 1;
        fz.rovf_rows = tier2;
        fz.ref_lim = ref_lim;
        fz.cand_cnt = cand_cnt;
        fz.cand_d2 = cand_d2;
        fz.cand_id = cand_id;
        fz.cap = SV_CAP;
        fz.n_db = p.n;
        fz.stats = fb.tail();
        SV_TRY(sv_launch_small_tail_debug(ctx, m, c.flags(), fb.count(), tier2, ref_lim));
      }
      SV_TRY(sv_launch_refine_exact(ctx, c.q, R, m, d, c.qn, rn, ctx->s_ref_cnt.as<uint32_t>(), ctx->s_ref_id.as<uint32_t>(), SV_RCAP, k,
                                    c.d2, c.idx, nullptr, c.flags(), fb.count(), &poison_dev, &fz, &tail_fused));
      sc.count();
    }
  }   // (the stage's stop event is recorded before the host waits below)
  if (s.device_tail) {
    // no read-back: small_tail_kernel reads the two counters on the device and finishes flagged rows there; the host learns
    // nothing about them in this call, segvlad_search_stats fetches the tail's counters on demand
    if (!tail_fused) {
      StageScope sc(ctx, "knn_select");
      SV_TRY(sv_launch_small_tail(ctx, c.q, R, c.qn, rn, p.n, d, m, k, c.flags(), fb.count(), tier2, ref_lim, cand_cnt, cand_d2, cand_id,
                                  SV_CAP, c.d2, c.idx, fb.tail()));
      sc.count();
    }
  } else {
    // one read-back per chunk: rows flagged for the redo / matrix-path fallback (handled by the caller) and rows whose refine
    // band outgrew the first-tier list.  The latter are refined here, straight from their candidate lists, which the next
    // chunk would overwrite.
    uint32_t h_cnt[2] = {0, 0}, h_poison = 0;
    SV_HIP(hipMemcpyAsync(&h_cnt[0], fb.count(), 8, hipMemcpyDeviceToHost, ctx->stream));
    if (poison_dev) SV_HIP(hipMemcpyAsync(&h_poison, poison_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    if (h_poison) SV_TRY(sv_refine_small_repair(ctx));   // a checked hand-over failed (its rows are flagged): fresh buffers
    fb.flagged = h_cnt[0];
    const uint32_t n2 = h_cnt[1] - fb.tier2_seen;   // the second-tier rows of THIS chunk
    fb.tier2_seen = h_cnt[1];
    if (n2) {
      StageScope sc(ctx, "knn_select");
      SV_TRY(sv_launch_refine2_compact(ctx, tier2, ref_lim, cand_cnt, cand_d2, cand_id, m, SV_CAP));
      if (cp.grouped_tier2) {
        // In blocks of <= 1024 + 128 query rows: the grouped path's scratch is per ROW of the block it is handed (40 KiB per row --
        // 670 MB for a whole 16 384-row chunk, kept for the context's life, where a handful of rows are flagged).  Blocks without
        // a flagged row cost four early-exit launches in a path that is taken once in a blue moon.
        int nl_sum = 0;
        for (int b0 = 0; b0 < m;) {
          int mb = std::min(1024, m - b0);
          if (m - (b0 + mb) < 129) mb = m - b0;   // (the grouped path wants > 128 rows: the tail joins the last block)
          int nl = 0;
          SV_TRY(sv_launch_refine_grouped(ctx, c.q + (size_t)b0 * d, R, mb, d, c.qn + b0, rn, cand_cnt + b0, cand_id + (size_t)b0 * SV_CAP,
                                          SV_CAP, k, c.d2 + (size_t)b0 * k, c.idx + (size_t)b0 * k, &nl, tier2 + b0,
                                          std::min<int>((int)n2, mb)));
          nl_sum += nl;
          b0 += mb;
        }
        sc.count(1 + nl_sum);
      } else {
        SV_TRY(sv_launch_refine_exact(ctx, c.q, R, m, d, c.qn, rn, cand_cnt, cand_id, SV_CAP, k, c.d2, c.idx, tier2));
        sc.count(2);
      }
      ctx->sstats.n_refine2 += n2;
    }
  }
  if (ctx->opt.search_stats) {
    Occupancy o;
    SV_TRY(read_counts(ctx, ctx->s_ref_cnt, m, c.host, &o));
    ctx->sstats.refine_sum += (int64_t)o.sum;
    ctx->sstats.refine_max = std::max<int64_t>(ctx->sstats.refine_max, o.max);
  }
  return SEGVLAD_OK;
}

static int run_chunk(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const PassScalars& v, Chunk& c, bool level0_done) {
  const ChunkPath cp = chunk_path(ctx, p, s, c.m);
  if (p.filter != Filter::FP32) SV_HIP(ctx->s_ref_lim.reserve((size_t)c.m * 4));
  if (!level0_done) SV_TRY(level0(ctx, p, s, v, c, cp));
  SV_TRY(filter_levels(ctx, p, s, v, c, cp));
  return p.filter == Filter::FP32 ? SEGVLAD_OK : finish(ctx, p, s, v, c, cp);
}

// One pass over nrows query rows in chunks of SV_CHUNK.  level0_done: the first chunk's level 0 has run already (the single-image
// head, or the early level 0 of a batch).
static int run_pass(segvlad_ctx* ctx, const SearchPlan& p, const Schedule& s, const PassScalars& v, const float* q, const uint16_t* qa,
                    const uint16_t* qb, const float* qn, int nrows, float* d2, int64_t* idx, FlagBlock& fb, bool level0_done) {
  const int d = p.d, k = p.k;
  for (int q0 = 0; q0 < nrows; q0 += SV_CHUNK) {
    const int m = std::min(nrows - q0, SV_CHUNK);
    if (q0) SV_HIP(hipMemsetAsync(fb.tier2(), 0, (size_t)m * 4, ctx->stream));
    Chunk c{q + (size_t)q0 * d, qa ? qa + (size_t)q0 * d : nullptr, qb ? qb + (size_t)q0 * d : nullptr, qn + q0, m, d2 + (size_t)q0 * k,
            idx + (size_t)q0 * k, &fb, q0, {}};
    SV_TRY(run_chunk(ctx, p, s, v, c, q0 == 0 && level0_done));
  }
  return SEGVLAD_OK;
}

// ---- flagged rows: the redo and the matrix-path fallback -----------------------------------------------------------
// Dense scratch of a pass over flagged rows: their indices, their query rows followed by their norms, their results.
struct RowScratch { DevBuf &rows, &q, &d2, &idx; };

// Reads flags[0, nrows) back (synchronises) and lists the flagged rows.
static int read_flagged(segvlad_ctx* ctx, const uint32_t* flags, int nrows, std::vector<int32_t>& rows) {
  std::vector<uint32_t> hf(nrows);
  SV_HIP(hipMemcpyAsync(hf.data(), flags, (size_t)nrows * 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  for (int r = 0; r < nrows; ++r)
    if (hf[r]) rows.push_back(r);
  return SEGVLAD_OK;
}

// Gathers the listed rows of (q, qn) into s.q: [nf][d] rows, then [nf] norms.
static int gather_flagged(segvlad_ctx* ctx, const RowScratch& s, const std::vector<int32_t>& rows, const float* q, const float* qn, int d,
                          int k) {
  const size_t nf = rows.size();
  SV_HIP(s.rows.reserve(nf * 4));
  SV_HIP(s.q.reserve(nf * ((size_t)d + 1) * 4));
  SV_HIP(s.d2.reserve(nf * k * 4));
  SV_HIP(s.idx.reserve(nf * k * 8));
  SV_HIP(hipMemcpyAsync(s.rows.p, rows.data(), nf * 4, hipMemcpyHostToDevice, ctx->stream));
  float* fq = s.q.as<float>();
  hipLaunchKernelGGL(gather_rows_kernel, dim3(nf), dim3(256), 0, ctx->stream, q, qn, s.rows.as<int32_t>(), d, fq, fq + nf * d);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// Scatters the nf rows of results in (s.d2, s.idx) back to their rows of (d2, idx).
static int scatter_flagged(segvlad_ctx* ctx, const RowScratch& s, int nf, int k, float* d2, int64_t* idx) {
  hipLaunchKernelGGL(scatter_topk_kernel, dim3(nf), dim3(256), 0, ctx->stream, s.d2.as<float>(), s.idx.as<int64_t>(), s.rows.as<int32_t>(),
                     k, d2, idx);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// rows flagged in flags[0..nrows) are redone on the exact distance-matrix path; their results replace rows of (d2, idx)
static int fallback_rows(segvlad_ctx* ctx, const SearchPlan& p, const float* q, const float* qn, const uint32_t* flags, int nrows,
                         float* d2, int64_t* idx) {
  std::vector<int32_t> rows;
  SV_TRY(read_flagged(ctx, flags, nrows, rows));
  const int nf = (int)rows.size();
  ctx->sstats.n_fallback = nf;
  if (nf == 0) return SEGVLAD_OK;
  const RowScratch s{ctx->s_fb_rows, ctx->s_fb_q, ctx->s_fb_d2, ctx->s_fb_idx};
  SV_TRY(gather_flagged(ctx, s, rows, q, qn, p.d, p.k));
  {
    StageScope sc(ctx, "knn_fallback");   // one stage (the matrix path's own scopes are muted: no double counting)
    const bool was_muted = ctx->scope_mute;
    ctx->scope_mute = true;
    const float* fq = s.q.as<float>();
    const int rc = search_matrix(ctx, fq, nf, p.n, p.d, p.k, fq + (size_t)nf * p.d, s.d2.as<float>(), s.idx.as<int64_t>());
    ctx->scope_mute = was_muted;
    SV_TRY(rc);
    sc.count(nf);
  }
  SV_TRY(scatter_flagged(ctx, s, nf, p.k, d2, idx));
  SV_HIP(hipStreamSynchronize(ctx->stream));  // rows[] lives on this frame
  return SEGVLAD_OK;
}

// The flagged queries of a guessed pass, redone with the rigorous thresholds as one dense batch.
static int redo_rows(segvlad_ctx* ctx, const SearchPlan& p, const PassScalars& v, const float* q, const float* qn, const FlagBlock& fb,
                     float* d2, int64_t* idx) {
  const int nq = p.nq, d = p.d;
  std::vector<int32_t> rows;
  SV_TRY(read_flagged(ctx, fb.rows(), nq, rows));
  const int nr = (int)rows.size();
  ctx->sstats.n_redo = nr;
  if ((int64_t)nr * 4 > nq && nq >= 64) ctx->db_heur_off = true;   // the sample misleads on this database: stop guessing
  FlagBlock rb{&ctx->s_rd_flags, nr, std::min(nr, SV_CHUNK), false};
  SV_HIP(ctx->s_rd_flags.reserve(rb.bytes()));
  SV_HIP(hipMemsetAsync(ctx->s_rd_flags.p, 0, rb.bytes(), ctx->stream));
  const RowScratch s{ctx->s_rd_rows, ctx->s_rd_q, ctx->s_rd_d2, ctx->s_rd_idx};
  SV_TRY(gather_flagged(ctx, s, rows, q, qn, d, p.k));
  const float* rq = s.q.as<float>();
  const float* rqn = rq + (size_t)nr * d;
  SV_HIP(ctx->s_rd_p1.reserve((size_t)nr * d * 2));
  if (p.filter == Filter::F16) {
    if (ctx->f16_scale_dev)   // same scale as the main pass
      SV_TRY(sv_launch_to_f16_devscale(ctx, rq, (int64_t)nr * d, ctx->f16_scale_dev, ctx->s_rd_p1.as<uint16_t>()));
    else
      SV_TRY(sv_launch_to_f16(ctx, rq, (int64_t)nr * d, v.qscale, ctx->s_rd_p1.as<uint16_t>()));
  } else {
    SV_HIP(ctx->s_rd_p2.reserve((size_t)nr * d * 2));
    SV_TRY(sv_launch_split_bf16(ctx, rq, (int64_t)nr * d, ctx->s_rd_p1.as<uint16_t>(), ctx->s_rd_p2.as<uint16_t>()));
  }
  {
    StageScope sc(ctx, "knn_redo");   // the whole redo is ONE stage: its inner level / filter / select scopes are muted,
    ctx->scope_mute = true;           // so "knn_gemm" etc. keep describing the main pass only (no double counting)
    const int rc = run_pass(ctx, p, p.rigorous, v, rq, ctx->s_rd_p1.as<uint16_t>(),
                            p.filter == Filter::BF16X3 ? ctx->s_rd_p2.as<uint16_t>() : nullptr, rqn, nr, s.d2.as<float>(), s.idx.as<int64_t>(),
                            rb, false);
    ctx->scope_mute = false;
    SV_TRY(rc);
    sc.count(nr);
  }
  SV_HIP(hipStreamSynchronize(ctx->stream));   // rows[] lives on this frame
  if (rb.flagged) SV_TRY(fallback_rows(ctx, p, rq, rqn, rb.rows(), nr, s.d2.as<float>(), s.idx.as<int64_t>()));
  return scatter_flagged(ctx, s, nr, p.k, d2, idx);
}

// ---- segvlad_search ------------------------------------------------------------------------------------------------
// The index's 16-bit planes and max ||r||^2, extended lazily to the rows added since the last search that needed them.
static int prepare_index_planes(segvlad_ctx* ctx, Filter kind) {
  if (kind == Filter::FP32) return SEGVLAD_OK;
  const int d = ctx->db_d;
  const int64_t n = ctx->db_n;
  const float* R = ctx->db_rows.as<float>();
  if (ctx->db_rn_max_rows < n) {
    float m = 0.f;
    SV_TRY(sv_row_norm_max(ctx, ctx->db_norms.as<float>() + ctx->db_rn_max_rows, n - ctx->db_rn_max_rows, &m, /*finite_only=*/true));
    if (m > ctx->db_rn_max) ctx->db_rn_max = m;
    ctx->db_rn_max_rows = n;
  }
  if (kind == Filter::F16 && ctx->db_f16_rows < n) {
    float m_new = 0.f;
    // The scale is taken over the SAME rows as max ||r||^2 above -- those whose squared norm is finite, the rows that can be listed:
    // the fp16 error bound (ctx.h, sv_f16_c_eps) rests on max |R| <= max ||r||.  A row that is never listed (it holds NaN / Inf, or
    // its norm overflowed) may hold finite entries of any size; they are cut at sqrt(max ||r||^2), which every listed row's entries
    // stay below and which is max |R| itself when all rows are finite.  (Such a row's own plane may overflow: its column is dropped.)
    SV_TRY(sv_maxabs(ctx, R + (size_t)ctx->db_f16_rows * d, (n - ctx->db_f16_rows) * d, &m_new, /*finite_only=*/true));
    m_new = std::min(m_new, std::sqrt(ctx->db_rn_max));
    const bool rescale = ctx->db_f16_rows == 0 || m_new * ctx->db_f16_scale >= 32768.f;
    if (m_new > ctx->db_maxabs) ctx->db_maxabs = m_new;
    int64_t r0 = ctx->db_f16_rows;
    if (rescale) {
      ctx->db_f16_scale = pow2_scale(ctx->db_maxabs);
      r0 = 0;
    }
    SV_HIP(grow_keep(ctx, ctx->db_f16, (size_t)r0 * d * 2, (size_t)n * d * 2, 4));
    SV_TRY(sv_launch_to_f16(ctx, R + (size_t)r0 * d, (n - r0) * d, ctx->db_f16_scale, ctx->db_f16.as<uint16_t>() + (size_t)r0 * d));
    ctx->db_f16_rows = n;
  }
  if (kind == Filter::BF16X3 && ctx->db_split_rows < n) {
    const int64_t r0 = ctx->db_split_rows;
    SV_HIP(grow_keep(ctx, ctx->db_hi, (size_t)r0 * d * 2, (size_t)n * d * 2, 4));
    SV_HIP(grow_keep(ctx, ctx->db_lo, (size_t)r0 * d * 2, (size_t)n * d * 2, 4));
    SV_TRY(sv_launch_split_bf16(ctx, R + (size_t)r0 * d, (n - r0) * d, ctx->db_hi.as<uint16_t>() + (size_t)r0 * d,
                                ctx->db_lo.as<uint16_t>() + (size_t)r0 * d));
    ctx->db_split_rows = n;
  }
  return SEGVLAD_OK;
}

// The call's scratch, each buffer sized for the whole call before the first launch.  Per-query scratch is sized for the rows of
// one chunk -- min(nq, SV_CHUNK), not SV_CHUNK: a one-image search on a large index used to allocate > 1 GiB of candidate lists.
static int reserve_scratch(segvlad_ctx* ctx, const SearchPlan& p, const FlagBlock& fb) {
  const size_t nq = p.nq, d = p.d, k = p.k, mrows = p.mrows;
  if (p.filter != Filter::FP32) {
    SV_HIP(ctx->s_ref_cnt.reserve(mrows * 4));
    SV_HIP(ctx->s_ref_id.reserve(mrows * SV_RCAP * 4));
  }
  if (p.filter == Filter::F16) SV_HIP(ctx->s_qf16.reserve(nq * d * 2));
  if (p.prep == Prep::SmallHead || p.prep == Prep::SmallF16) SV_HIP(ctx->s_qscale.reserve(16));
  if (p.filter == Filter::BF16X3) {
    SV_HIP(ctx->s_qh.reserve(nq * d * 2));
    SV_HIP(ctx->s_ql.reserve(nq * d * 2));
  }
  SV_HIP(ctx->s_cand_cnt.reserve(mrows * 4));
  SV_HIP(ctx->s_cand_d2.reserve(mrows * SV_CAP * 4));
  SV_HIP(ctx->s_cand_id.reserve(mrows * SV_CAP * 4));
  SV_HIP(ctx->s_thr_d2.reserve(mrows * k * 4));
  SV_HIP(ctx->s_thr_idx.reserve(mrows * k * 8));
  // level 0's distance block: the larger of the two plans' samples (the single-image plan's stride can be SMALLER than the
  // rigorous plan's: 64 against 256 for a 250 k-row shard)
  const int64_t stride_min = std::min(p.rigorous.stride0, p.pass.stride0);
  const int64_t n0 = (p.n + stride_min - 1) / stride_min;
  SV_HIP(ctx->s_dist.reserve(mrows * ((n0 + 3) & ~3ll) * 4));
  SV_HIP(fb.buf->reserve(fb.bytes()));
  return SEGVLAD_OK;
}

// The queries' squared norms, their 16-bit planes and the scalars of the filter's margin; zeroes the flag block (the
// single-image kernels do that in their own launch).
static int prepare_queries(segvlad_ctx* ctx, const SearchPlan& p, const float* q, FlagBlock& fb, PassScalars& v) {
  const int nq = p.nq, d = p.d;
  const int64_t ne = (int64_t)nq * d;
  float* qn = ctx->s_qnorm.as<float>();
  float q2min = 0.f;
  if (p.filter != Filter::FP32) v.rn_max = ctx->db_rn_max;
  switch (p.prep) {
    case Prep::SmallHead: {
      // the whole head of a single-image pass in ONE launch (small_pass_kernels.hip) -- plane, scale, norms, flags AND level 0's
      // thresholds from the filter's own fp16 product on the sample (guesses the pass verifies: they need no exact distances)
      StageScope sc(ctx, "knn_level0");
      SV_TRY(sv_launch_small_head(ctx, q, nq, d, ctx->db_f16.as<uint16_t>(), ctx->db_norms.as<float>(), p.pass.stride0,
                                  (int)((p.n + p.pass.stride0 - 1) / p.pass.stride0), ctx->db_f16_scale, p.pass.rank[0],
                                  ctx->s_qf16.as<uint16_t>(), ctx->s_qscale.as<float>(), qn, fb.rows(), (int)(fb.bytes() / 4),
                                  ctx->s_dist.as<float>(), ctx->s_thr_d2.as<float>(), ctx->s_cand_cnt.as<uint32_t>()));
      sc.count();
      break;
    }
    case Prep::SmallF16:
      SV_TRY(sv_launch_query_f16_small(ctx, q, ne, ctx->db_f16_scale, ctx->s_qf16.as<uint16_t>(), ctx->s_qscale.as<float>(),
                                       p.fuse_qn ? qn : nullptr, nq, d, fb.rows(), (int)(fb.bytes() / 4)));
      break;
    case Prep::BatchF16:
    case Prep::BatchF16EarlyL0: {
      SV_TRY(sv_launch_row_sumsq(ctx, q, nq, d, qn));
      float qmax = 0.f;
      float q2max = 0.f;
      bool q_nonfinite = false;   // the scale and min ||q||^2 are those of the finite entries / rows: one bad row must not cost the others their plane
      if (p.q2min) {   // both scalars behind one read-back
        SV_TRY(sv_maxabs_and_norm_min_begin(ctx, q, ne, qn, nq));
        if (p.prep == Prep::BatchF16EarlyL0) {
          // level 0 of the first chunk while the host waits; it reads none of the scalars (PassScalars' defaults)
          SV_HIP(hipMemsetAsync(fb.buf->p, 0, fb.bytes(), ctx->stream));
          Chunk c{q, nullptr, nullptr, qn, p.mrows, nullptr, nullptr, &fb, 0, {}};
          SV_TRY(level0(ctx, p, p.pass, PassScalars{}, c, chunk_path(ctx, p, p.pass, p.mrows)));
        }
        SV_TRY(sv_maxabs_and_norm_min_end(ctx, ne, nq, &qmax, &q2min, &q_nonfinite, &q2max));
      } else {
        SV_TRY(sv_row_norm_max(ctx, qn, nq, &q2max, /*finite_only=*/true));
        SV_TRY(sv_maxabs(ctx, q, ne, &qmax, /*finite_only=*/true, &q_nonfinite));
      }
      // (as for the index: the scale of the rows whose norm is finite -- a bad row's finite entries are cut at the largest finite ||q||)
      qmax = std::min(qmax, std::sqrt(q2max));
      v.qmax = q_nonfinite ? NAN : qmax;
      v.qscale = pow2_scale(qmax);
      SV_TRY(sv_launch_to_f16(ctx, q, ne, v.qscale, ctx->s_qf16.as<uint16_t>()));
      v.inv_scale = 1.f / (v.qscale * ctx->db_f16_scale);
      break;
    }
    case Prep::Bf16Split:
      SV_TRY(sv_launch_split_bf16(ctx, q, ne, ctx->s_qh.as<uint16_t>(), ctx->s_ql.as<uint16_t>()));
      // |d2~ - d2| <= 2 * (3*2^-16 + 4*d*2^-24) * ||q|| * ||r||   (+25 % slack)
      v.c_eps = 2.5f * (3.f / 65536.f + 4.f * (float)d / 16777216.f);
      break;
    case Prep::Fp32:
      break;
  }
  if (p.prep == Prep::SmallHead || p.prep == Prep::SmallF16) {
    ctx->f16_scale_dev = ctx->s_qscale.as<float>();   // the kernels read s_qscale[1]: inv_scale unused
    v.inv_scale = 0.f;
  }
  if (p.filter == Filter::F16) {
    // |d2~ - d2| <= c_eps ||q|| ||r||: ctx.h, sv_f16_c_eps (the constant of the kernel variant that will run).  Batches (default
    // configuration) take the biased-accumulator kernel when the norms are balanced enough for its margin:
    // bias_mult = 1 + max||r|| / (2 min||q||), 1.5 for unit vectors
    const float bm = 1.f + std::sqrt(v.rn_max) / (2.f * std::sqrt(q2min));
    ctx->f16_bias_ok = p.q2min && q2min > 0.f && v.rn_max > 0.f && std::isfinite(bm) && bm <= 5.f;
    v.c_eps = sv_f16_c_eps(d, sv_f16_eps_kblock(ctx->opt, d), ctx->f16_bias_ok ? bm : 1.f);
  }
  // the norms of the paths that have not produced them on the way (batches: first of all); the flag block, unless zeroed already
  const bool batch = p.prep == Prep::BatchF16 || p.prep == Prep::BatchF16EarlyL0;
  if (!batch && !p.fuse_qn) SV_TRY(sv_launch_row_sumsq(ctx, q, nq, d, qn));
  if (p.prep == Prep::Bf16Split || p.prep == Prep::Fp32 || p.prep == Prep::BatchF16)
    SV_HIP(hipMemsetAsync(fb.buf->p, 0, fb.bytes(), ctx->stream));
  return SEGVLAD_OK;
}

// The entry preamble of the searches derived from segvlad_search (ctx.h): each entry runs these in the order its own checks had.
int sv_check_qseg_offsets(segvlad_ctx* ctx, const char* entry, const int32_t* qseg_offsets, int n_img, int nq) {
  if (!qseg_offsets) return ctx->fail(SEGVLAD_ERR_ARG, "%s: null qseg_offsets", entry);
  if (sv_is_device_ptr(qseg_offsets)) return ctx->fail(SEGVLAD_ERR_ARG, "%s: qseg_offsets must be host memory", entry);
  if (qseg_offsets[0] != 0 || qseg_offsets[n_img] != nq)
    return ctx->fail(SEGVLAD_ERR_ARG, "%s: qseg_offsets must run from 0 to nq=%d", entry, nq);
  for (int b = 0; b < n_img; ++b)
    if (qseg_offsets[b + 1] < qseg_offsets[b]) return ctx->fail(SEGVLAD_ERR_ARG, "%s: qseg_offsets decrease at %d", entry, b);
  return SEGVLAD_OK;
}

int sv_check_img_index(segvlad_ctx* ctx, const char* entry) {
  if (ctx->db_d == 0) return ctx->fail(SEGVLAD_ERR_STATE, "%s: the index is empty and has no dimension yet", entry);
  if (!ctx->db_has_img) return ctx->fail(SEGVLAD_ERR_STATE, "%s: no img_of_seg map: give it to segvlad_db_add", entry);
  return SEGVLAD_OK;
}

int sv_aligned_queries(segvlad_ctx* ctx, const float* dq, int nq, const float** out) {
  *out = dq;
  if ((reinterpret_cast<uintptr_t>(dq) & 15) == 0) return SEGVLAD_OK;
  const size_t bytes = (size_t)nq * ctx->db_d * 4;
  SV_HIP(ctx->s_sl_q.reserve(bytes));
  SV_HIP(hipMemcpyAsync(ctx->s_sl_q.p, dq, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  *out = ctx->s_sl_q.as<float>();
  return SEGVLAD_OK;
}

hipError_t sv_fill_none(segvlad_ctx* ctx, float* d2, int64_t* idx, size_t n) {
  const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d2), 0x7f800000, n, ctx->stream);
  return e != hipSuccess ? e : hipMemsetAsync(idx, 0xff, n * 8, ctx->stream);
}

extern "C" int segvlad_search(segvlad_ctx* ctx, const float* Q, int nq, int k, float* d2_out, int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || k < 1 || k > 1024) return ctx->fail(SEGVLAD_ERR_ARG, "search: need nq>=0 and 1<=k<=1024 (k=%d)", k);
  if (nq == 0) return SEGVLAD_OK;
  if (!Q || !d2_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "search: null pointer");
  if (ctx->db_d == 0) return ctx->fail(SEGVLAD_ERR_STATE, "search: the index is empty and has no dimension yet");
  if (ctx->opt.debug_fail_search == 1) return ctx->fail(SEGVLAD_ERR_STATE, "search: failing on request (option debug_fail_search)");
  const void* dq;
  void *dd2, *didx;
  SV_TRY(sv_in(ctx, Q, (size_t)nq * ctx->db_d * 4, &dq));
  SV_TRY(sv_out(ctx, d2_out, (size_t)nq * k * 4, &dd2));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k * 8, &didx));
  SV_TRY(sv_search_dev(ctx, (const float*)dq, nq, k, (float*)dd2, (int64_t*)didx));
  return sv_finish(ctx);
}

// segvlad_search behind its argument checks and staging: q / d2 / idx on the device, nq >= 1, the index has a dimension.  Also the
// inner search of segvlad_search_excluding and segvlad_search_grouped, which run it at a larger depth into ctx->s_deep_*.
int sv_search_dev(segvlad_ctx* ctx, const float* q, int nq, int k, float* d2, int64_t* idx) {
  const void* dq = q;
  ctx->f16_scale_dev = nullptr;
  SV_HIP(ctx->s_qnorm.reserve((size_t)nq * 4));
  float* qn = ctx->s_qnorm.as<float>();
  ctx->sstats = SvSearchStats();
  ctx->sstats.n_queries = nq;
  ctx->tail_stats_dev = nullptr;
  ctx->small_head_ran = false;
  // device-driven single-image passes never tell the host how many rows they had to redo -- but their running total lands in a
  // pinned word (small_tail_kernel): looked at here WITHOUT synchronising (it may be a pass or two behind).  More than a quarter
  // of >= 64 rows redone since the index last changed: the sample misleads on this database, stop guessing (as redo_rows
  // decides for its own redos).
  if (ctx->h_pin && ctx->tail_rows_since >= 64) {
    const uint32_t redone = reinterpret_cast<volatile uint32_t*>(ctx->h_pin)[SV_PIN_TOTALS] - ctx->tail_fail_base;
    if ((int64_t)redone * 4 > ctx->tail_rows_since) ctx->db_heur_off = true;
  }

  if (ctx->db_n == 0) {   // emptied by segvlad_db_remove: every slot beyond the (zero) rows is (+inf, -1)
    SV_HIP(sv_fill_none(ctx, d2, idx, (size_t)nq * k));
    return SEGVLAD_OK;
  }
  const SearchPlan p = plan_search(ctx, nq, k, dq);
  if (p.matrix) {
    SV_TRY(sv_launch_row_sumsq(ctx, q, nq, p.d, qn));
    SV_TRY(search_matrix(ctx, q, nq, p.n, p.d, k, qn, d2, idx));
    return unlist_nonfinite(ctx, qn, nq, k, d2, idx);
  }
  ctx->sstats.filter = (int)p.filter;
  ctx->sstats.levels = p.pass.levels;
  FlagBlock fb{&ctx->s_ovf, nq, p.mrows, true};
  SV_TRY(prepare_index_planes(ctx, p.filter));
  SV_TRY(reserve_scratch(ctx, p, fb));
  PassScalars v;
  SV_TRY(prepare_queries(ctx, p, q, fb, v));
  const uint16_t* qa = p.filter == Filter::F16 ? ctx->s_qf16.as<uint16_t>() : p.filter == Filter::BF16X3 ? ctx->s_qh.as<uint16_t>() : nullptr;
  const uint16_t* qb = p.filter == Filter::BF16X3 ? ctx->s_ql.as<uint16_t>() : nullptr;
  SV_TRY(run_pass(ctx, p, p.pass, v, q, qa, qb, qn, nq, d2, idx, fb, p.prep == Prep::SmallHead || p.prep == Prep::BatchF16EarlyL0));
  if (p.pass.device_tail) {
    ctx->tail_stats_dev = fb.tail();
    ctx->tail_rows_since += nq;
  }
  // a guessed pass flags the queries whose thresholds did not verify (-> redo with the rigorous thresholds); a rigorous pass
  // flags list overflows (-> exact distance-matrix path, alone)
  if (fb.flagged && !p.pass.guessed) SV_TRY(fallback_rows(ctx, p, q, qn, fb.rows(), nq, d2, idx));
  else if (fb.flagged) SV_TRY(redo_rows(ctx, p, v, q, qn, fb, d2, idx));
  return unlist_nonfinite(ctx, qn, nq, k, d2, idx);
}

// ---- segvlad_range_search ------------------------------------------------------------------------------------------
// Every index row within a squared radius of each query row (faiss IndexFlat::range_search), in the search's own bits.
//   filter path : ONE full-level fp16 filter launch per chunk under thr = radius2 with one margin (an exact d2 < r2 has
//                 d2~ <= r2 + eps: the argument of the rigorous level 0), then range_refine_kernel evaluates every candidate with
//                 the exact chain, keeps the hits and orders them.  A row whose list outgrew SV_CAP (the filter keeps counting),
//                 or whose radius is +inf, is a LONG row.
//   exact path  : small index, d % 64 != 0, option knn_filter = fp32, a NaN / inf among the queries: every row is a long row.
//   long rows   : exact distance blocks (the fp32 distance GEMM: same chain, same bits) of those rows against slabs of the index,
//                 counted in one sweep and -- once the offsets are known and the result fits -- emitted in a second one, each
//                 row's segment then ordered by its 64-bit words.
// The counts of all rows are scanned into lims on the device; the total reaches the host, and only a result that fits is unpacked.
constexpr int64_t SV_RS_SLAB = 65536;   // index rows of one exact distance block
constexpr int SV_RS_QBLOCK = 512;       // ... and its query rows (128 MiB of distances)

// Grows a scratch buffer whose first `keep` bytes are still needed (the staged words of the chunks so far).
static hipError_t regrow_keep(segvlad_ctx* ctx, DevBuf& b, size_t keep, size_t bytes) {
  if (b.p && (b.guard ? bytes <= b.req : bytes <= b.cap)) return hipSuccess;
  if (!keep || !b.p) return b.reserve(bytes);
  DevBuf nb;
  nb.tag = b.tag;
  nb.guard = b.guard;
  nb.fixed = b.fixed;
  hipError_t e = nb.reserve(bytes + bytes / 2);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    nb.release();
    return e;
  }
  b.release();
  b = nb;
  return hipSuccess;
}

// One sweep of the exact distance blocks of the nl dense query rows (qx, their norms qnx, their radii effx; rows_dev: the row of
// the call each one is) over the whole index: counted into cnt (words == null) or emitted.  (Also the exact tail of
// segvlad_search_grouped, group_kernels.hip.)
int sv_range_exact_sweep(segvlad_ctx* ctx, const float* qx, const float* qnx, const float* effx, const int32_t* rows_dev, int nl,
                         uint32_t* cnt, const int64_t* woff, uint32_t* cur, uint64_t* words, int* launches) {
  const int d = ctx->db_d;
  const int64_t n = ctx->db_n;
  const int64_t ld = (std::min(n, SV_RS_SLAB) + 3) & ~3ll;
  SV_HIP(ctx->s_dist.reserve((size_t)std::min(nl, SV_RS_QBLOCK) * ld * 4));
  for (int qb = 0; qb < nl; qb += SV_RS_QBLOCK) {
    const int mq = std::min(nl - qb, SV_RS_QBLOCK);
    for (int64_t c0 = 0; c0 < n; c0 += SV_RS_SLAB) {
      const int ns = (int)std::min(n - c0, SV_RS_SLAB);
      SV_TRY(sv_launch_gemm_nt(ctx, 1, qx + (size_t)qb * d, ctx->db_rows.as<float>() + (size_t)c0 * d, ctx->s_dist.as<float>(), mq, ns, d,
                               ld, nullptr, nullptr, qnx + qb, ctx->db_norms.as<float>() + c0));
      SV_TRY(sv_launch_range_block(ctx, ctx->s_dist.as<float>(), ld, mq, ns, c0, effx + qb, rows_dev + qb, cnt, woff, cur, words));
      *launches += 2;
    }
  }
  return SEGVLAD_OK;
}

// segvlad_range_search behind its checks: q / radius2 / lims on the device, nq >= 1, the index holds rows.
static int range_search_dev(segvlad_ctx* ctx, const float* q, int nq, const float* radius2, int64_t* lims, float* d2_out, int64_t* idx_out,
                            int64_t capacity, int64_t* total_out) {
  const SvOptions& o = ctx->opt;
  const int d = ctx->db_d;
  const int64_t n = ctx->db_n;
  const float* R = ctx->db_rows.as<float>();
  const float* rn = ctx->db_norms.as<float>();
  ctx->f16_scale_dev = nullptr;
  StageScope sc(ctx, "knn_range");
  SV_HIP(ctx->s_qnorm.reserve((size_t)nq * 4));
  SV_HIP(ctx->s_rs_thr.reserve((size_t)nq * 8));
  SV_HIP(ctx->s_rs_flag.reserve((size_t)nq * 4));
  SV_HIP(ctx->s_rs_cnt.reserve((size_t)nq * 4));
  SV_HIP(ctx->s_rs_soff.reserve((size_t)nq * 8));
  SV_HIP(ctx->s_rs_misc.reserve(64));
  float* qn = ctx->s_qnorm.as<float>();
  float* eff = ctx->s_rs_thr.as<float>();
  float* thr = eff + nq;
  uint32_t* flags = ctx->s_rs_flag.as<uint32_t>();
  uint32_t* cnt = ctx->s_rs_cnt.as<uint32_t>();
  int64_t* soff = ctx->s_rs_soff.as<int64_t>();
  uint64_t* misc = ctx->s_rs_misc.as<uint64_t>();   // [0] the stage cursor, [2..5] one chunk's list statistics
  SV_HIP(hipMemsetAsync(cnt, 0, (size_t)nq * 4, ctx->stream));
  SV_HIP(hipMemsetAsync(misc, 0, 64, ctx->stream));

  // the filter path: where plan_search starts filtering, on the fp16 product; the refinement keeps a query row and up to SV_CAP
  // words in LDS (d <= 8192) and reads rows in 16-byte pieces
  bool filt = (o.knn_filter == 0 || o.knn_filter == 1) && d % 64 == 0 && d <= 8192 && n > 32768 && n <= 0x7fffffffLL &&
              (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  SearchPlan p{nq, d, 1, n};
  PassScalars v;
  if (filt) {
    // query preparation as the search's batches: norms, scale (read back), plane, the margin constant of the filter variant
    // that runs -- the forms that only prepare, whatever the number of rows
    p.filter = Filter::F16;
    p.prep = Prep::BatchF16;
    p.q2min = sv_f16_bias_possible(o, nq);
    p.mrows = std::min(nq, SV_CHUNK);
    FlagBlock fb{&ctx->s_rs_fb, nq, p.mrows, false};
    SV_TRY(prepare_index_planes(ctx, Filter::F16));
    SV_HIP(ctx->s_qf16.reserve((size_t)nq * d * 2));
    SV_HIP(ctx->s_cand_cnt.reserve((size_t)p.mrows * 4));
    SV_HIP(ctx->s_cand_d2.reserve((size_t)p.mrows * SV_CAP * 4));
    SV_HIP(ctx->s_cand_id.reserve((size_t)p.mrows * SV_CAP * 4));
    SV_HIP(fb.buf->reserve(fb.bytes()));
    SV_TRY(prepare_queries(ctx, p, q, fb, v));
    sc.count(4);
    // a NaN or inf among the queries: no scale serves the other rows' plane -- the exact path takes the call
    if (!std::isfinite(v.qmax)) filt = false;
  } else {
    SV_TRY(sv_launch_row_sumsq(ctx, q, nq, d, qn));
    sc.count();
  }
  SV_TRY(sv_launch_range_thr(ctx, radius2, nq, eff, thr, flags, !filt));
  sc.count();
  ctx->rs_stats[4] = filt ? 1 : 0;

  int64_t n_long = filt ? 0 : nq;
  if (filt) {
    uint64_t used = 0;   // words of s_rs_stage the chunks so far may have filled
    for (int q0 = 0; q0 < nq; q0 += SV_CHUNK) {
      const int m = std::min(nq - q0, SV_CHUNK);
      uint32_t* cand_cnt = ctx->s_cand_cnt.as<uint32_t>();
      SV_HIP(hipMemsetAsync(cand_cnt, 0, (size_t)m * 4, ctx->stream));
      SV_TRY(sv_launch_f16_filter(ctx, ctx->s_qf16.as<uint16_t>() + (size_t)q0 * d, ctx->db_f16.as<uint16_t>(), m, (int)n, d, 1, v.inv_scale,
                                  qn + q0, rn, thr + q0, 1, 1.f, v.c_eps, v.rn_max, cand_cnt, ctx->s_cand_d2.as<float>(),
                                  ctx->s_cand_id.as<uint32_t>(), SV_CAP));
      SV_TRY(sv_launch_range_cand_stats(ctx, cand_cnt, m, SV_CAP, flags + q0, misc + 2));
      uint64_t h[4] = {0, 0, 0, 0};   // words the short rows may stage, sum and max of the list lengths, long rows
      SV_HIP(hipMemcpyAsync(h, misc + 2, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      SV_HIP(hipStreamSynchronize(ctx->stream));
      ctx->rs_stats[3] += (int64_t)h[1];
      ctx->rs_stats[2] = std::max<int64_t>(ctx->rs_stats[2], (int64_t)h[2]);
      n_long += (int64_t)h[3];
      const hipError_t e = regrow_keep(ctx, ctx->s_rs_stage, (size_t)used * 8, (size_t)std::max<uint64_t>(used + h[0], 1) * 8);
      if (e != hipSuccess)
        return ctx->fail(e == hipErrorOutOfMemory ? SEGVLAD_ERR_NOMEM : SEGVLAD_ERR_HIP, "range search: staging %llu candidate words: %s",
                         (unsigned long long)(used + h[0]), hipGetErrorString(e));
      SV_TRY(sv_launch_range_refine(ctx, q + (size_t)q0 * d, R, m, d, qn + q0, rn, eff + q0, cand_cnt, ctx->s_cand_id.as<uint32_t>(), SV_CAP,
                                    (uint32_t)std::min<uint64_t>(h[2], SV_CAP), flags + q0, cnt + q0, soff + q0,
                                    ctx->s_rs_stage.as<uint64_t>(), misc));
      used += h[0];
      sc.count(3);
    }
  }
  ctx->rs_stats[1] = n_long;

  // long rows: the dense block of their query rows, and the counting sweep
  std::vector<int32_t> rows;
  const float *qx = nullptr, *qnx = nullptr, *effx = nullptr;
  if (n_long > 0) {
    if (filt) {
      SV_TRY(read_flagged(ctx, flags, nq, rows));
    } else {
      rows.resize(nq);
      for (int r = 0; r < nq; ++r) rows[r] = r;
    }
    const size_t nl = rows.size();
    SV_HIP(ctx->s_rs_rows.reserve(nl * 4));
    SV_HIP(ctx->s_rs_q.reserve(nl * ((size_t)d + 2) * 4));
    SV_HIP(hipMemcpyAsync(ctx->s_rs_rows.p, rows.data(), nl * 4, hipMemcpyHostToDevice, ctx->stream));
    float* qxw = ctx->s_rs_q.as<float>();
    qx = qxw;
    qnx = qxw + nl * d;
    effx = qxw + nl * d + nl;
    SV_TRY(sv_launch_range_gather(ctx, q, qn, eff, ctx->s_rs_rows.as<int32_t>(), (int)nl, d, qxw, qxw + nl * d, qxw + nl * d + nl));
    int launches = 1;
    SV_TRY(sv_range_exact_sweep(ctx, qx, qnx, effx, ctx->s_rs_rows.as<int32_t>(), (int)nl, cnt, nullptr, nullptr, nullptr, &launches));
    sc.count(launches);
  }

  // counts -> lims; the long rows' own offsets; the totals to the host
  int64_t total = 0, total_long = 0;
  int64_t* loff = nullptr;
  SV_TRY(sv_launch_range_scan(ctx, cnt, nullptr, nq, lims));
  sc.count();
  SV_HIP(hipMemcpyAsync(&total, lims + nq, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (n_long > 0) {
    SV_HIP(ctx->s_rs_loff.reserve(((size_t)nq + 1) * 8));
    loff = ctx->s_rs_loff.as<int64_t>();
    SV_TRY(sv_launch_range_scan(ctx, cnt, flags, nq, loff));
    sc.count();
    SV_HIP(hipMemcpyAsync(&total_long, loff + nq, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  SV_HIP(hipStreamSynchronize(ctx->stream));   // (rows[] has been copied, too)
  ctx->rs_stats[0] = total;
  *total_out = total;
  if (total == 0 || total > capacity) return SEGVLAD_OK;   // nothing to write, or the caller's buffers stay untouched

  void *dd2 = nullptr, *didx = nullptr;
  SV_TRY(sv_out(ctx, d2_out, (size_t)total * 4, &dd2));
  SV_TRY(sv_out(ctx, idx_out, (size_t)total * 8, &didx));
  if (filt) {
    SV_TRY(sv_launch_range_unpack(ctx, ctx->s_rs_stage.as<uint64_t>(), soff, flags, 0u, nq, lims, (float*)dd2, (int64_t*)didx));
    sc.count();
  }
  if (total_long > 0) {
    SV_HIP(ctx->s_rs_cur.reserve((size_t)nq * 4));
    SV_HIP(ctx->s_rs_words.reserve((size_t)total_long * 8));
    SV_HIP(ctx->s_rs_sorted.reserve((size_t)total_long * 8));
    SV_HIP(hipMemsetAsync(ctx->s_rs_cur.p, 0, (size_t)nq * 4, ctx->stream));
    int launches = 0;
    SV_TRY(sv_range_exact_sweep(ctx, qx, qnx, effx, ctx->s_rs_rows.as<int32_t>(), (int)rows.size(), cnt, loff, ctx->s_rs_cur.as<uint32_t>(),
                             ctx->s_rs_words.as<uint64_t>(), &launches));
    SV_TRY(sv_range_sort_segments(ctx, ctx->s_rs_words.as<uint64_t>(), ctx->s_rs_sorted.as<uint64_t>(), total_long, nq, loff));
    SV_TRY(sv_launch_range_unpack(ctx, ctx->s_rs_sorted.as<uint64_t>(), loff, flags, 1u, nq, lims, (float*)dd2, (int64_t*)didx));
    sc.count(launches + 2);
  }
  return SEGVLAD_OK;
}

extern "C" int segvlad_range_search(segvlad_ctx* ctx, const float* Q, int nq, const float* radius2, int64_t* lims_out, float* d2_out,
                                    int64_t* idx_out, int64_t capacity, int64_t* n_total_out) {
  CHECK_CTX();
  if (nq < 0 || capacity < 0) return ctx->fail(SEGVLAD_ERR_ARG, "range_search: need nq>=0 and capacity>=0");
  if (!lims_out || (nq > 0 && (!Q || !radius2)) || (capacity > 0 && (!d2_out || !idx_out)))
    return ctx->fail(SEGVLAD_ERR_ARG, "range_search: null pointer");
  if (nq > 0 && ctx->db_d == 0) return ctx->fail(SEGVLAD_ERR_STATE, "range_search: the index is empty and has no dimension yet");
  if (ctx->db_n > 0xffffffffLL) return ctx->fail(SEGVLAD_ERR_LIMIT, "range_search: %lld index rows (candidate ids are 32-bit)", (long long)ctx->db_n);
  for (int64_t& s : ctx->rs_stats) s = 0;
  if (n_total_out) *n_total_out = 0;
  void* dlims;
  SV_TRY(sv_out(ctx, lims_out, ((size_t)nq + 1) * 8, &dlims));
  if (nq == 0 || ctx->db_n == 0) {   // no query rows, or an index that removal has emptied: all-zero lims
    SV_HIP(hipMemsetAsync(dlims, 0, ((size_t)nq + 1) * 8, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    return sv_finish(ctx);
  }
  const void *dq, *drad;
  SV_TRY(sv_in(ctx, Q, (size_t)nq * ctx->db_d * 4, &dq));
  SV_TRY(sv_in(ctx, radius2, (size_t)nq * 4, &drad));
  int64_t total = 0;
  SV_TRY(range_search_dev(ctx, (const float*)dq, nq, (const float*)drad, (int64_t*)dlims, d2_out, idx_out, capacity, &total));
  if (n_total_out) *n_total_out = total;
  return sv_finish(ctx);
}

extern "C" int segvlad_range_stats(segvlad_ctx* ctx, int64_t* stats_out, int n) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  if (!stats_out || n < 0) return ctx->fail(SEGVLAD_ERR_ARG, "range_stats: bad arguments");
  for (int j = 0; j < n && j < 5; ++j) stats_out[j] = ctx->rs_stats[j];
  return SEGVLAD_OK;
}
