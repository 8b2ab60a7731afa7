// The describe stage's host side: masks + tokens -> (projected) segment descriptors, and the two other users of the assign / prep /
// aggregate launchers (k-means step, cluster aggregation).  Like a search (search.hip), a call is PLANNED before anything is enqueued
// (plan_describe) and then run as staged passes over the plan (run_describe).  A public entry point that enqueued something calls
// sv_finish exactly once, last, on the context's main stream (segvlad_describe: in its segvlad_describe_end half); no pass does.
#include <cmath>
#include "ctx.h"

// (CHECK_NO_OPEN_DESCRIBE: ctx.h)

// One walk over a batch's segment offsets for every caller: the largest image, the offsets of the adjacency blocks (adj_off[b] = sum of
// S_b'^2 over the images before b), and whether every size is >= 0 -- which each caller reports in its own words.
struct SegWalk { int S_max = 0; bool monotone = true; std::vector<int64_t> adj_off; };
static SegWalk walk_seg_offsets(const int32_t* seg_offsets, int B) {
  SegWalk w;
  w.adj_off.assign((size_t)B + 1, 0);
  for (int b = 0; b < B && w.monotone; ++b) {
    const int s = seg_offsets[b + 1] - seg_offsets[b];
    w.monotone = s >= 0;
    if (s > w.S_max) w.S_max = s;
    w.adj_off[b + 1] = w.adj_off[b] + (int64_t)s * s;
  }
  return w;
}

// ---- incidence / centroids, adjacency: everything of the entry points but the finish (the mask branch of a describe issues the same) ----
static int incidence_run(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch, uint64_t* inc_bits,
                         double* centroids, bool want_centroids) {
  if (S < 0 || Hm <= 0 || Wm <= 0 || H <= 0 || W <= 0 || patch <= 0 || H / patch <= 0 || W / patch <= 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "incidence: bad geometry S=%d masks %dx%d image %dx%d patch %d", S, Hm, Wm, H, W, patch);
  if (S == 0) return SEGVLAD_OK;
  if (!masks || !inc_bits || (want_centroids && !centroids)) return ctx->fail(SEGVLAD_ERR_ARG, "incidence: null pointer");
  const int N = (H / patch) * (W / patch), nw = (N + 63) / 64;
  const void* dm;
  void *dout, *dcent = nullptr;
  SV_TRY(sv_in(ctx, masks, (size_t)S * Hm * Wm, &dm));
  SV_TRY(sv_out(ctx, inc_bits, (size_t)S * nw * 8, &dout));
  if (want_centroids) SV_TRY(sv_out(ctx, centroids, (size_t)S * 2 * sizeof(double), &dcent));
  StageScope sc(ctx, "incidence");
  SV_TRY(sv_launch_incidence(ctx, (const uint8_t*)dm, S, Hm, Wm, H, W, patch, (uint64_t*)dout, (double*)dcent));
  sc.count();
  return SEGVLAD_OK;
}

static int adjacency_run(segvlad_ctx* ctx, const double* centroids, const int32_t* seg_offsets, int B, int order, uint8_t* adj_out,
                         uint8_t* img_flags_out) {
  if (B < 0 || order < 1) return ctx->fail(SEGVLAD_ERR_ARG, "adjacency: need B>=0 and order>=1 (order 0 = pass adj=NULL)");
  if (B == 0) return SEGVLAD_OK;
  if (!centroids || !seg_offsets || !adj_out) return ctx->fail(SEGVLAD_ERR_ARG, "adjacency: null pointer");
  if (sv_is_device_ptr(seg_offsets)) return ctx->fail(SEGVLAD_ERR_ARG, "adjacency: seg_offsets must be host memory");
  const SegWalk w = walk_seg_offsets(seg_offsets, B);
  if (!w.monotone) return ctx->fail(SEGVLAD_ERR_ARG, "adjacency: seg_offsets must be non-decreasing");
  const int S_tot = seg_offsets[B];
  if (S_tot == 0) return SEGVLAD_OK;
  const void* dc;
  void *dout, *dflags = nullptr;
  SV_TRY(sv_in(ctx, centroids, (size_t)S_tot * 2 * sizeof(double), &dc));
  SV_TRY(sv_out(ctx, adj_out, (size_t)w.adj_off[B], &dout));
  SV_HIP(ctx->s_segoff.reserve((size_t)(B + 1) * sizeof(int32_t)));
  SV_HIP(ctx->s_adjoff.reserve((size_t)(B + 1) * sizeof(int64_t)));
  SV_HIP(ctx->s_flag.reserve(64));
  SV_HIP(hipMemcpyAsync(ctx->s_segoff.p, seg_offsets, (size_t)(B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  SV_HIP(hipMemcpyAsync(ctx->s_adjoff.p, w.adj_off.data(), (size_t)(B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  // (pageable sources: the runtime stages them before hipMemcpyAsync returns, so the walk's vector and the caller's array may go)
  uint32_t* bad = ctx->s_flag.as<uint32_t>() + 4;   // the counter of empty masks (segvlad_adjacency reads it back)
  SV_HIP(hipMemsetAsync(bad, 0, 4, ctx->stream));
  if (img_flags_out) {
    SV_TRY(sv_out(ctx, img_flags_out, (size_t)B, &dflags));
    SV_HIP(hipMemsetAsync(dflags, 0, (size_t)B, ctx->stream));
  }
  StageScope sc(ctx, "adjacency");
  SV_TRY(sv_launch_adjacency(ctx, (const double*)dc, ctx->s_segoff.as<int32_t>(), ctx->s_adjoff.as<int64_t>(), B, w.S_max, order,
                             (uint8_t*)dout, bad, (uint8_t*)dflags));
  sc.count();
  return SEGVLAD_OK;
}

// ---- segment VLAD: the plan --------------------------------------------------------------------------
// How a batch's descriptors are computed (segvlad_images: always Descriptor; segvlad_images_pca: one of the other three)
enum class DescribeForm {
  Descriptor,        // aggregate into the K*D-wide descriptor
  Planes,            // fused projection: the aggregation also writes the descriptor's fp16 planes, planes x W on the 16-bit pipe
  Project,           // fused projection: project every covered token with its cluster's slice of W, aggregate in P dimensions
  PlainProjection,   // no fp16 split of the model (option pca_arith=fp32, K*D % 32 != 0): descriptor to HBM, then segvlad_pca_apply
};
enum class Passes { All, AssignOnly, FromPrep };   // a whole call | segvlad_describe_begin, k-means | segvlad_describe_end
// A call's arguments as the caller gave them, in segvlad_images' order (+ y, l2norm), and where stage_pointers put them on the device
struct DescribeIO {
  const float* tokens; int B, N; const uint64_t* inc_bits; const int32_t* seg_offsets; const uint8_t* adj;
  float* out;   // the descriptor (PlainProjection without one: reserve_scratch points it at s_desc)
  uint8_t* labels_out; float *gap_out, *block_norms_out, *y; int l2norm;
  const void *d_tok = nullptr, *d_inc = nullptr, *d_adj = nullptr;
  void *d_out = nullptr, *d_lab = nullptr, *d_gap = nullptr, *d_bn = nullptr, *d_y = nullptr;
};
struct DescribePlan {
  int code = SEGVLAD_OK;   // != OK: the call is refused with `why`, nothing else below is set
  char why[192] = {0};
  Passes passes = Passes::All;
  DescribeForm form = DescribeForm::Descriptor;
  int B = 0, N = 0, K = 0, D = 0, P = 0, S_tot = 0, S_max = 0, SC = 1, nw = 0, l2norm = 0;
  std::vector<int64_t> adj_off;   // [B + 1]: where image b's S_b x S_b adjacency block starts
  float xscale = 1.f;      // power-of-two scale of the fp16 planes (Planes: descriptor - mean; Project: token residuals)
  float zscale = 0.f;      // Project: scale of the projected residuals on the 16-bit pipe (0: fp32 MFMA)
  float soft_temp = 0.f;   // option vlad_assign: 0 = hard; > 0 = soft assignment at this temperature (soft_vlad_kernels.hip)
  bool soft_pooled = false;   // ... soft_pooled:<T>: residuals against all centres
  bool burst = false;         // option vlad_burst: every assignment weight times u[n] = g[n]^-p (burst_kernels.hip) ...
  float burst_a = 0.f, burst_b = 0.f, burst_p = 0.f;   // ... g[n] = sum_m sigmoid(a (2 cos(x_n, x_m) - 2) + b)
  bool burst_segment = false;   // ... option vlad_burst_scope=segment (set only with burst): the sum runs over U(s), a weight per
                                // (segment, token) in s_bseg (burst_seg_kernels.hip)
  bool weighted() const { return soft_temp > 0.f || burst; }   // the descriptor is the weight buffer's aggregation (soft_aggregate_kernel)
  int64_t rows_pad = 0;    // Project: grouped token rows, every cluster's rows padded to whole 256-row GEMM tiles
  bool want_desc = false, want_y = false, want_labels = false, want_gap = false, want_block_norms = false;   // the optional outputs
  bool upload_offsets = false;   // this call puts the segment / adjacency offsets on the device (else: the mask branch of its begin did)
};

// The project form gives every token the slice of ONE cluster, unweighted: auto takes the planes form under soft assignment or the burst
// discount, an explicit pca_path=project is refused (SEGVLAD_ERR_LIMIT).  True, with the message under the caller's name in `why`, when
// the options ask for that.
static bool refuses_project(const segvlad_ctx* ctx, const char* who, char* why, size_t n) {
  if (ctx->opt.pca_path != 2) return false;
  if (ctx->opt.vlad_soft_temp > 0.f)
    snprintf(why, n, "%s: pca_path=project presupposes one cluster per token, vlad_assign=%s:%g has none "
                     "(set pca_path to auto or planes, or vlad_assign to hard)",
             who, ctx->opt.vlad_soft_pooled ? "soft_pooled" : "soft", (double)ctx->opt.vlad_soft_temp);
  else if (ctx->opt.vlad_burst)
    snprintf(why, n, "%s: pca_path=project presupposes unweighted tokens, vlad_burst=%g:%g:%g weights them "
                     "(set pca_path to auto or planes, or vlad_burst to off)",
             who, (double)ctx->opt.burst_a, (double)ctx->opt.burst_b, (double)ctx->opt.burst_p);
  else
    return false;
  return true;
}

// Every check and every decision of a call, before anything is enqueued: arithmetic on the arguments, the options and the context's scalars.
static DescribePlan plan_describe(const segvlad_ctx* ctx, const DescribeIO& io, bool pca, Passes passes) {
  DescribePlan p;
#define PLAN_REFUSE(code_, ...) (p.code = (code_), snprintf(p.why, sizeof(p.why), __VA_ARGS__), p)
  const int B = io.B, N = io.N, K = ctx->K, D = ctx->D;
  const bool x3 = ctx->pca_w_scale > 0.f && !ctx->opt.pca_fp32;
  if (pca) {
    if (ctx->P == 0) return PLAN_REFUSE(SEGVLAD_ERR_STATE, "images_pca: call segvlad_pca_set first");
    if (K == 0) return PLAN_REFUSE(SEGVLAD_ERR_STATE, "images_pca: call segvlad_set_vocab first");
    if (ctx->KD != K * D)
      return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images_pca: the PCA model expects %d-d rows, the vocabulary gives %d", ctx->KD, K * D);
    if (B > 0 && io.seg_offsets && !sv_is_device_ptr(io.seg_offsets) && io.seg_offsets[B] > 0 && !io.y)
      return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images_pca: null y");
    if (!x3 && passes != Passes::All) return PLAN_REFUSE(SEGVLAD_ERR_STATE, "describe: the split call needs the fp16x3 projection (pca_arith)");
    if (refuses_project(ctx, "images_pca", p.why, sizeof(p.why))) return (p.code = SEGVLAD_ERR_LIMIT, p);
  }
  if (K == 0) return PLAN_REFUSE(SEGVLAD_ERR_STATE, "images: call segvlad_set_vocab first");
  p.passes = passes, p.B = B, p.N = N, p.K = K, p.D = D, p.P = ctx->P, p.nw = (N + 63) / 64, p.l2norm = io.l2norm;
  p.soft_pooled = ctx->opt.vlad_soft_pooled != 0;
  p.soft_temp = ctx->opt.vlad_soft_temp;   // (read by the passes behind prep alone: an assign-only plan is the hard assignment)
  p.burst = ctx->opt.vlad_burst != 0, p.burst_a = ctx->opt.burst_a, p.burst_b = ctx->opt.burst_b, p.burst_p = ctx->opt.burst_p;
  p.burst_segment = p.burst && ctx->opt.burst_segment != 0;
  if (passes == Passes::AssignOnly)   // tokens -> token-major copy, norms, labels in the context's scratch; no segments yet
    return (B <= 0 || N <= 0 || !io.tokens) ? PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: B=%d N=%d", B, N) : p;
  if (B < 0 || N <= 0) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: B=%d N=%d", B, N);
  if (B == 0) return p;   // nothing to do
  if (!io.tokens || !io.seg_offsets) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: null pointer");
  if (sv_is_device_ptr(io.seg_offsets)) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: seg_offsets must be host memory");
  if (io.seg_offsets[0] != 0) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: seg_offsets[0] must be 0");
  SegWalk w = walk_seg_offsets(io.seg_offsets, B);
  if (!w.monotone) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: seg_offsets must be non-decreasing");
  p.S_tot = io.seg_offsets[B], p.S_max = w.S_max, p.SC = w.S_max > 0 ? (w.S_max + 63) / 64 : 1;
  p.adj_off = std::move(w.adj_off);
  const bool plain = pca && !x3;
  const float* y = plain ? nullptr : io.y;   // (the plain projection is a call of its own behind the descriptor)
  if (p.S_tot > 0 && (!io.inc_bits || (!io.out && !y && !plain))) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images: null inc_bits/out");
  p.upload_offsets = passes == Passes::All;
  p.want_desc = p.S_tot > 0 && (io.out || plain), p.want_block_norms = io.block_norms_out && p.S_tot > 0;
  p.want_labels = io.labels_out != nullptr, p.want_gap = io.gap_out != nullptr;
  // fused projection: the descriptor entries are <= 1 in magnitude by construction, so the fp16 split scale is known before the data
  // exists (pca_apply has to measure max|x| first)
  p.want_y = y != nullptr && p.S_tot > 0;
  if (plain) p.form = DescribeForm::PlainProjection;
  if (!p.want_y) return p;
  // "project then aggregate" (project_kernels.hip) when the descriptor itself is not asked for.  auto: when it is the smaller product
  // (N D P per image against S K D P) and the batch holds >= 128 tokens per cluster on average -- every cluster's rows are padded to
  // whole 256-row GEMM tiles, below that the split-K descriptor GEMM is quicker ("The fused VLAD -> PCA call", has the numbers)
  const bool project = !p.weighted() && io.out == nullptr && D % 32 == 0 && ctx->P % 4 == 0 && ctx->opt.pca_path != 1 &&
                       (ctx->opt.pca_path == 2 || ((double)p.S_tot * K >= 1.25 * (double)B * N && (double)B * N >= 128.0 * K));
  p.form = project ? DescribeForm::Project : DescribeForm::Planes;
  p.xscale = sv_fp16_scale(1.f + ctx->pca_mean_maxabs);
  if (!project) return p;
  // residuals of unit tokens against the centres: |r| <= 1 + max|C|.  Centres that are means of unit tokens (every k-means vocabulary)
  // give 2^13, like the planes form's data-derived scale; arbitrary centres (segvlad_set_vocab takes any) get the scale their
  // magnitude needs instead of overflowing fp16 silently
  const float bound = 1.f + ctx->vocab_maxabs;
  if (!std::isfinite(bound)) return PLAN_REFUSE(SEGVLAD_ERR_ARG, "images_pca: the vocabulary holds a non-finite centre");
  p.xscale = sv_fp16_scale(bound);
  p.rows_pad = (((int64_t)B * N + 255) & ~255ll) + 256ll * K;
  // |z_tp| = |W_k[p, :] . r_t| <= sqrt(D) max|W| (1 + max ||C_k||): a power-of-two scale that keeps z * zscale inside fp16.  Both premises
  // hold BY CONSTRUCTION: x^_t is normalised by the kernels themselves, vocab_norm_max is set by segvlad_set_vocab, the elementwise bound of
  // W is the one pca_set left in pca_w_scale.  A bound that is not finite and positive switches the 16-bit form off (zscale = 0: fp32 MFMA)
  if (ctx->pca_w_scale > 0.f) {
    const float zb = std::sqrt((float)D) * (16384.f / ctx->pca_w_scale) * (1.f + ctx->vocab_norm_max);
    if (std::isfinite(zb) && zb > 0.f) p.zscale = sv_fp16_scale(zb);
  }
  return p;
#undef PLAN_REFUSE
}

// ---- segment VLAD: the staged passes ------------------------------------------------------------------
// The call's scratch, sized before the first launch (guard mode places the fences by these byte counts)
static int reserve_scratch(segvlad_ctx* ctx, const DescribePlan& p, DescribeIO& io) {
  const size_t B = p.B, N = p.N, D = p.D, K = p.K, P = p.P, S = p.S_tot;
  if (p.form == DescribeForm::Project) {
    SV_HIP(ctx->s_xh1.reserve((size_t)(p.rows_pad + 256) * D * 2));   // + one tile: the dummy row of sv_launch_token_norms
    SV_HIP(ctx->s_xh2.reserve((size_t)(p.rows_pad + 256) * D * 2));
    SV_HIP(ctx->s_pz.reserve((size_t)(p.rows_pad + 1) * P * sizeof(float)));   // + the zero row of the pj_planes aggregation
    SV_HIP(ctx->s_rowbase.reserve(B * K * sizeof(int32_t)));
    SV_HIP(ctx->s_tilegrp.reserve((size_t)(p.rows_pad >> 8) * sizeof(int32_t)));
    SV_HIP(ctx->s_phys.reserve(B * N * sizeof(int32_t)));
    SV_HIP(ctx->s_covcnt.reserve(B * K * sizeof(int32_t)));
    SV_HIP(ctx->s_bn.reserve(S * K * sizeof(float)));
  } else if (p.form == DescribeForm::Planes) {
    SV_HIP(ctx->s_xh1.reserve((size_t)sv_x3_rows(p.S_tot) * ctx->KD * 2));   // blocked planes, rows padded to whole tiles
    SV_HIP(ctx->s_xh2.reserve((size_t)sv_x3_rows(p.S_tot) * ctx->KD * 2));
  } else if (p.form == DescribeForm::PlainProjection && !io.out && S > 0) {
    SV_HIP(ctx->s_desc.reserve(S * ctx->KD * sizeof(float)));
    io.out = ctx->s_desc.as<float>();
  }
  SV_HIP(ctx->s_xt.reserve(B * N * D * sizeof(float)));
  SV_HIP(ctx->s_rnorm.reserve(B * N * sizeof(float)));
  if (!p.want_labels) SV_HIP(ctx->s_labels.reserve(B * N));
  if (p.passes == Passes::AssignOnly) return SEGVLAD_OK;
  if (p.weighted() && S > 0) {   // the weights, the block norms the row scale is made of, the descriptor the planes are split from
    // (segment scope under hard assignment has no weight buffer: label k's positions carry weight 1)
    if (!(p.burst_segment && p.soft_temp == 0.f)) SV_HIP(ctx->s_softw.reserve(B * N * K * sizeof(float)));
    if (p.soft_pooled) SV_HIP(ctx->s_softc.reserve(D * sizeof(float)));
    if (!p.want_block_norms) SV_HIP(ctx->s_bn.reserve(S * K * sizeof(float)));
    if (p.form == DescribeForm::Planes && !p.want_desc) SV_HIP(ctx->s_desc.reserve(S * K * D * sizeof(float)));
    if (p.burst_segment) SV_HIP(ctx->s_bseg.reserve(B * N * 64 * (size_t)p.SC * sizeof(float)));
    else if (p.burst) SV_HIP(ctx->s_burst.reserve(B * (size_t)sv_burst_tiles(p.N) * N * sizeof(float)));
  }
  SV_HIP(ctx->s_colmask.reserve(B * N * p.SC * 8));
  SV_HIP(ctx->s_gscale.reserve((S + 1) * sizeof(float)));
  SV_HIP(ctx->s_segoff.reserve((B + 1) * sizeof(int32_t)));
  SV_HIP(ctx->s_adjoff.reserve((B + 1) * sizeof(int64_t)));
  return SEGVLAD_OK;
}

// Host pointers to the device (inputs copied now, outputs flushed by sv_finish), and the offsets where this call uploads them
static int stage_pointers(segvlad_ctx* ctx, const DescribePlan& p, DescribeIO& io) {
  const size_t B = p.B, N = p.N, S = p.S_tot;
  if (p.want_y) SV_TRY(sv_out(ctx, io.y, S * p.P * sizeof(float), &io.d_y));
  SV_TRY(sv_in(ctx, io.tokens, B * p.D * N * sizeof(float), &io.d_tok));
  if (S > 0) SV_TRY(sv_in(ctx, io.inc_bits, S * p.nw * 8, &io.d_inc));
  if (io.adj && S > 0) SV_TRY(sv_in(ctx, io.adj, (size_t)p.adj_off[B], &io.d_adj));
  if (p.want_desc) SV_TRY(sv_out(ctx, io.out, S * p.K * p.D * sizeof(float), &io.d_out));
  if (p.want_labels) SV_TRY(sv_out(ctx, io.labels_out, B * N, &io.d_lab));
  else io.d_lab = ctx->s_labels.p;
  if (p.want_gap) SV_TRY(sv_out(ctx, io.gap_out, B * N * sizeof(float), &io.d_gap));
  if (p.want_block_norms) SV_TRY(sv_out(ctx, io.block_norms_out, S * p.K * sizeof(float), &io.d_bn));
  if (p.upload_offsets) {
    SV_HIP(hipMemcpyAsync(ctx->s_segoff.p, io.seg_offsets, (B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SV_HIP(hipMemcpyAsync(ctx->s_adjoff.p, p.adj_off.data(), (B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  }
  return SEGVLAD_OK;
}

// labels (cosine arg-max against the normalised centres, first maximum), the token-major copy Xt, 1 / ||x||
static int pass_assign(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io) {
  StageScope sc(ctx, "assign");
  SV_TRY(sv_launch_assign(ctx, (const float*)io.d_tok, p.B, p.N, ctx->s_xt.as<float>(), (uint8_t*)io.d_lab, ctx->s_rnorm.as<float>(),
                          (float*)io.d_gap));
  sc.count();
  return SEGVLAD_OK;
}
static int pass_prep(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io) {
  const bool project = p.form == DescribeForm::Project;
  StageScope sc(ctx, "prep");
  SV_TRY(sv_launch_prep(ctx, (const uint8_t*)io.d_lab, (const uint64_t*)io.d_inc, ctx->s_segoff.as<int32_t>(), ctx->s_adjoff.as<int64_t>(),
                        (const uint8_t*)io.d_adj, p.B, p.N, p.K, p.S_max, p.SC, ctx->s_colmask.as<uint64_t>(), ctx->s_gscale.as<float>(),
                        project ? ctx->s_phys.as<int32_t>() : nullptr, project ? ctx->s_covcnt.as<int32_t>() : nullptr,
                        ctx->opt.cover_rows != 0 ? 1 : 0));
  sc.count();
  return SEGVLAD_OK;
}
// the tail of both fused forms, inside their "pca" stage
static int pass_normalize(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io, StageScope& sc) {
  if (!p.l2norm) return SEGVLAD_OK;
  SV_TRY(sv_launch_normalize_rows(ctx, (const float*)io.d_y, p.S_tot, p.P, (float*)io.d_y));
  sc.count();
  return SEGVLAD_OK;
}

// Soft assignment and / or burst discount: the weights ("assign"; "burst": g from the self-similarity tiles, then the weights times
// g^-p -- under hard assignment the one-hot of the labels times g^-p, so that path too aggregates from the weight buffer, at K times
// the hard aggregation's MFMA work), then intra-normalised blocks + block norms, the rows' scale, and for the planes form the
// split of the finished fp32 descriptor that segvlad_pca_apply uses, at the scale known in advance ("aggregate").
// vlad_burst_scope=segment: "burst" is one kernel, the weights u[s][n] of every (segment, covered token) from the tiles of the
// self-similarity times the column masks; the aggregation takes them as its A operand and, under hard assignment, walks label k's
// positions for cluster k -- the hard aggregation's matrix work, no weight buffer
static int pass_soft_descriptor(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io, uint16_t* h1, uint16_t* h2) {
  float* desc = io.d_out ? (float*)io.d_out : ctx->s_desc.as<float>();
  float* bn = io.d_bn ? (float*)io.d_bn : ctx->s_bn.as<float>();
  if (p.soft_temp > 0.f) {
    StageScope sc(ctx, "assign");
    SV_TRY(sv_launch_soft_weights(ctx, (const float*)io.d_tok, p.B, p.N, p.soft_temp, ctx->s_softw.as<float>()));
    sc.count();
  }
  if (p.burst_segment) {
    StageScope sc(ctx, "burst");
    SV_TRY(sv_launch_burst_seg_gram(ctx, ctx->s_xt.as<float>(), ctx->s_colmask.as<uint64_t>(), ctx->s_segoff.as<int32_t>(), p.B, p.N, p.D,
                                    p.SC, p.burst_a, p.burst_b, p.burst_p, ctx->s_bseg.as<float>()));
    sc.count();
  } else if (p.burst) {
    StageScope sc(ctx, "burst");
    SV_TRY(sv_launch_burst_gram(ctx, ctx->s_xt.as<float>(), ctx->s_rnorm.as<float>(), p.B, p.N, p.D, p.burst_a, p.burst_b,
                                ctx->s_burst.as<float>()));
    SV_TRY(sv_launch_burst_finish(ctx, ctx->s_burst.as<float>(), (const uint8_t*)io.d_lab, p.B, p.N, p.K, p.burst_p, p.soft_temp == 0.f,
                                  ctx->s_softw.as<float>()));
    sc.count(2);
  }
  StageScope sc(ctx, "aggregate");
  const float* cmean = nullptr;
  if (p.soft_pooled) {
    SV_TRY(sv_launch_soft_centre_mean(ctx, ctx->vocab.as<float>(), p.K, p.D, ctx->s_softc.as<float>()));
    sc.count();
    cmean = ctx->s_softc.as<float>();
  }
  if (p.burst_segment)
    SV_TRY(sv_launch_burst_seg_aggregate(ctx, ctx->s_xt.as<float>(), p.soft_temp > 0.f ? ctx->s_softw.as<float>() : nullptr,
                                         ctx->s_bseg.as<float>(), ctx->s_colmask.as<uint64_t>(), ctx->vocab.as<float>(), p.K, p.D,
                                         ctx->s_segoff.as<int32_t>(), p.B, p.N, p.SC, desc, bn, cmean));
  else
    SV_TRY(sv_launch_soft_aggregate(ctx, ctx->s_xt.as<float>(), ctx->s_softw.as<float>(), ctx->s_colmask.as<uint64_t>(), ctx->vocab.as<float>(),
                                    p.K, p.D, ctx->s_segoff.as<int32_t>(), p.B, p.N, p.SC, desc, bn, cmean));
  SV_TRY(sv_launch_soft_finalize(ctx, bn, p.S_tot, p.K, p.D, desc));
  sc.count(2);
  if (h1) {
    SV_TRY(sv_launch_split_f16x2(ctx, desc, p.S_tot, ctx->KD, ctx->pca_mean.as<float>(), p.xscale, h1, h2));
    sc.count();
  }
  return SEGVLAD_OK;
}

// aggregate (Planes: the descriptor's fp16 planes beside or instead of the descriptor), then planes x W
static int pass_descriptor(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io) {
  const bool fused = p.form == DescribeForm::Planes;
  uint16_t *h1 = fused ? ctx->s_xh1.as<uint16_t>() : nullptr, *h2 = fused ? ctx->s_xh2.as<uint16_t>() : nullptr;
  if (p.weighted()) {
    SV_TRY(pass_soft_descriptor(ctx, p, io, h1, h2));
  } else {
    StageScope sc(ctx, "aggregate");
    SV_TRY(sv_launch_aggregate(ctx, ctx->s_xt.as<float>(), ctx->s_colmask.as<uint64_t>(), ctx->vocab.as<float>(), p.K, p.D,
                               ctx->s_segoff.as<int32_t>(), ctx->s_gscale.as<float>(), p.B, p.N, p.SC, (float*)io.d_out,
                               (float*)io.d_bn, fused ? ctx->pca_mean.as<float>() : nullptr, p.xscale, h1, h2));
    sc.count();
  }
  if (!fused) return SEGVLAD_OK;
  StageScope sc(ctx, "pca");
  SV_TRY(sv_launch_gemm_f16x3(ctx, h1, h2, ctx->pca_w1.as<uint16_t>(), ctx->pca_w2.as<uint16_t>(), p.S_tot, p.P, ctx->KD,
                              1.f / (p.xscale * ctx->pca_w_scale), ctx->pca_scale.as<float>(), (float*)io.d_y));
  sc.count(2);
  return pass_normalize(ctx, p, io, sc);
}

// group plan + token norms (block norms and the token residuals' fp16 planes, grouped by cluster), grouped GEMM, P-space aggregate
static int pass_project(segvlad_ctx* ctx, const DescribePlan& p, const DescribeIO& io) {
  float* bn = io.d_bn ? (float*)io.d_bn : ctx->s_bn.as<float>();
  uint16_t *h1 = ctx->s_xh1.as<uint16_t>(), *h2 = ctx->s_xh2.as<uint16_t>();
  {
    StageScope sc(ctx, "aggregate");
    SV_TRY(sv_launch_group_plan(ctx, ctx->s_covcnt.as<int32_t>(), p.B, p.K, ctx->s_rowbase.as<int32_t>(), ctx->s_tilegrp.as<int32_t>(),
                                (int)(p.rows_pad >> 8)));
    SV_TRY(sv_launch_token_norms(ctx, ctx->s_xt.as<float>(), ctx->s_colmask.as<uint64_t>(), ctx->vocab.as<float>(), p.K, p.D,
                                 ctx->s_segoff.as<int32_t>(), p.B, p.N, p.SC, bn, p.xscale, h1, h2, ctx->s_rowbase.as<int32_t>(),
                                 ctx->opt.debug_search == 7 ? -p.rows_pad : p.rows_pad, ctx->s_phys.as<int32_t>()));
    sc.count(2);
  }
  StageScope sc(ctx, "pca");
  // pj_planes: Z leaves the GEMM as the fp16 pairs of z * zscale, the aggregation's MFMA operands (same bytes, same bits of y)
  const bool z_pairs = sv_project_z_pairs(ctx, p.zscale, p.rows_pad + 1, p.P);
  if (z_pairs)   // the row behind the GEMM's last: what the aggregation reads for a position without a row (its loads are unconditional)
    SV_HIP(hipMemsetAsync(ctx->s_pz.as<float>() + (size_t)p.rows_pad * p.P, 0, (size_t)p.P * sizeof(float), ctx->stream));
  SV_TRY(sv_launch_gemm_f16x3_grouped(ctx, h1, h2, ctx->pca_w1.as<uint16_t>(), ctx->pca_w2.as<uint16_t>(), (int)p.rows_pad, p.P, p.D, p.K,
                                      ctx->s_tilegrp.as<int32_t>(), 1.f / (p.xscale * ctx->pca_w_scale), ctx->s_pz.as<float>(),
                                      z_pairs ? p.zscale : 0.f));
  SV_TRY(sv_launch_project_aggregate(ctx, ctx->s_pz.as<float>(), ctx->pca_cproj.as<float>(), bn, ctx->s_gscale.as<float>(),
                                     ctx->s_colmask.as<uint64_t>(), ctx->s_laboff.as<int32_t>(), ctx->s_rowbase.as<int32_t>(),
                                     ctx->s_phys.as<int32_t>(), ctx->s_segoff.as<int32_t>(), p.B, p.N, p.K, p.P, p.SC, p.S_max,
                                     ctx->pca_scale.as<float>(), (float*)io.d_y, p.zscale, z_pairs ? 1 : 0, p.rows_pad));
  sc.count(2);
  return pass_normalize(ctx, p, io, sc);
}

// An open describe's mask branch joins the main stream once: here, in front of the first consumer of its outputs
static int join_mask_branch(segvlad_ctx* ctx) {
  if (!ctx->desc.side_pending) return SEGVLAD_OK;
  ctx->desc.side_pending = false;
  return sv_join_side(ctx);
}
// The passes of a planned call, from the one its plan starts at; the caller finishes (sv_finish)
static int run_describe(segvlad_ctx* ctx, const DescribePlan& p, DescribeIO& io) {
  SV_TRY(reserve_scratch(ctx, p, io));
  if (p.form == DescribeForm::Project && !ctx->pca_cproj_valid) {   // W mean: rebuilt when segvlad_pca_set has made it stale
    SV_HIP(ctx->pca_cproj.reserve((size_t)ctx->P * sizeof(float)));
    SV_TRY(sv_launch_project_consts(ctx, ctx->pca_comps.as<float>(), ctx->pca_mean.as<float>(), ctx->P, ctx->KD, ctx->pca_cproj.as<float>()));
    ctx->pca_cproj_valid = true;
  }
  SV_TRY(stage_pointers(ctx, p, io));
  if (p.passes != Passes::FromPrep) SV_TRY(pass_assign(ctx, p, io));
  if (p.passes == Passes::AssignOnly) return SEGVLAD_OK;
  SV_TRY(join_mask_branch(ctx));   // (segvlad_describe_end: incidence + centroids + adjacency ran beside the assignment pass)
  if (p.S_tot == 0) return SEGVLAD_OK;
  SV_TRY(pass_prep(ctx, p, io));
  return p.form == DescribeForm::Project ? pass_project(ctx, p, io) : pass_descriptor(ctx, p, io);
}

// segvlad_images / segvlad_images_pca: plan, every pass, finish
static int describe_whole(segvlad_ctx* ctx, DescribeIO& io, bool pca) {
  const DescribePlan p = plan_describe(ctx, io, pca, Passes::All);
  if (p.code != SEGVLAD_OK) return ctx->fail(p.code, "%s", p.why);
  if (p.B == 0) return SEGVLAD_OK;
  SV_TRY(run_describe(ctx, p, io));
  if (p.form != DescribeForm::PlainProjection || p.S_tot == 0) return sv_finish(ctx);
  SV_TRY(sv_finish(ctx));   // ends in ANOTHER entry point: host outputs are flushed before segvlad_pca_apply starts its own staging
  return segvlad_pca_apply(ctx, io.out, p.S_tot, io.y, p.l2norm);
}

// ---- the whole describe stage of a batch in ONE call: masks + tokens -> (projected) segment descriptors ----------------------
// place_rec_main.py:244-270 per image (masks -> adjacency -> seg_vlad_gpu_single) and per batch (apply_pca_transform_from_pkl).  The mask
// branch does not depend on the tokens, the assignment pass does not depend on the masks: the former runs on the context's side stream
// BESIDE the latter and is joined in front of `prep`, the first kernel that needs both ("The describe stage as one call").
struct MaskBranch {   // segvlad_describe_begin's mask-side arguments, in its order (bulk pointers: device memory)
  const uint8_t* masks; int Hm, Wm, H, W, patch; const int32_t* seg_offsets; int B, order;
  uint64_t* inc_bits; double* centroids; uint8_t *adj, *flags;
};
// the side stream forked; on it: incidence + centroids, adjacency, the flags' and the centroids' copies to the pinned landing zone, the event
static int pass_mask_branch(segvlad_ctx* ctx, const MaskBranch& m, int S_tot) {
  SV_TRY(sv_fork_side(ctx));
  ctx->desc.side_pending = true;
  StreamSwitch on_side(ctx, ctx->side);
  SV_TRY(incidence_run(ctx, m.masks, S_tot, m.Hm, m.Wm, m.H, m.W, m.patch, m.inc_bits, m.centroids, true));
  SV_TRY(adjacency_run(ctx, m.centroids, m.seg_offsets, m.B, m.order, m.adj, m.flags));
  hipError_t e = hipMemcpyAsync(ctx->h_desc, m.flags, (size_t)m.B, hipMemcpyDeviceToHost, ctx->side);
  if (e == hipSuccess)
    e = hipMemcpyAsync(ctx->h_desc + (((size_t)m.B + 63) & ~(size_t)63), m.centroids, (size_t)S_tot * 16, hipMemcpyDeviceToHost, ctx->side);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev_desc, ctx->side);
  if (e != hipSuccess) return ctx->fail(SEGVLAD_ERR_HIP, "describe: flags read-back: %s", hipGetErrorString(e));
  return SEGVLAD_OK;
}

// The one way out of an open describe (every exit of begin, end and cancel): nothing of the mask branch stays behind on the side stream
// unobserved, the "describe" stage's event pair is closed, the context takes other batches again; returns rc
static int close_describe(segvlad_ctx* ctx, bool ran, int rc) {
  (void)join_mask_branch(ctx);
  OpenDescribe& d = ctx->desc;
  if (d.timer) {
    (void)hipEventRecord(d.timer->ev[2 * d.slot + 1], ctx->stream);
    if (ran) d.timer->launches += 1;
  }
  d = OpenDescribe{};
  return rc;
}

// segvlad_describe_begin but its finish (segvlad_describe goes on into segvlad_describe_end, which finishes)
static int describe_begin(segvlad_ctx* ctx, const MaskBranch& m, const float* tokens, int N, bool pca) {
  const int B = m.B;
  if (ctx->desc.open) return ctx->fail(SEGVLAD_ERR_STATE, "describe_begin: the previous describe_begin has no describe_end yet");
  if (B < 0 || m.order < 1) return ctx->fail(SEGVLAD_ERR_ARG, "describe: need B >= 0 and order >= 1");
  if (!m.masks || !tokens || !m.seg_offsets || !m.inc_bits || !m.centroids || !m.adj || !m.flags)
    return ctx->fail(SEGVLAD_ERR_ARG, "describe: null pointer");
  if (sv_is_device_ptr(m.seg_offsets)) return ctx->fail(SEGVLAD_ERR_ARG, "describe: seg_offsets must be host memory");
  const void* bulk[] = {m.masks, tokens, m.inc_bits, m.centroids, m.adj, m.flags};
  for (const void* p : bulk)
    if (!sv_is_device_ptr(p))
      return ctx->fail(SEGVLAD_ERR_ARG, "describe: bulk pointers must be device memory (the separate entry points stage host data)");
  if (m.patch <= 0 || N != (m.H / m.patch) * (m.W / m.patch))
    return ctx->fail(SEGVLAD_ERR_ARG, "describe: N=%d tokens do not match the %dx%d image at patch %d", N, m.H, m.W, m.patch);
  const int S_tot = B > 0 ? m.seg_offsets[B] : 0;
  // Configurations the split call does not take are reported as SEGVLAD_ERR_LIMIT -- the code of "this entry point cannot, the separate
  // ones (incidence_centroids -> adjacency -> images[_pca]) can", which a caller can tell from misuse: an empty batch, and a
  // PCA model without the fp16x3 form (option pca_arith=fp32, or K*D not a multiple of 32: images_pca takes its PlainProjection form)
  char why[256];
  if (pca && refuses_project(ctx, "describe", why, sizeof(why)))   // (plan_describe's refusal, before the mask branch is forked)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "%s", why);
  if (B == 0 || S_tot <= 0) return ctx->fail(SEGVLAD_ERR_LIMIT, "describe: no images / no segments (use the separate entry points)");
  // ... and an image that sv_launch_adjacency would refuse: the same bound, asked before the mask branch is forked
  const SegWalk w = walk_seg_offsets(m.seg_offsets, B);
  if (w.monotone && !sv_adjacency_fits(w.S_max))
    return ctx->fail(SEGVLAD_ERR_LIMIT, "describe: %d segments in one image exceed the in-LDS Delaunay (use the separate entry points)",
                     w.S_max);
  if (pca && ctx->P == 0) return ctx->fail(SEGVLAD_ERR_STATE, "describe: call segvlad_pca_set first");
  if (pca && (ctx->pca_w_scale <= 0.f || ctx->opt.pca_fp32))
    return ctx->fail(SEGVLAD_ERR_LIMIT,
                     "describe: the split call needs the fp16x3 projection (pca_arith; K*D %% 32 == 0): use the separate entry points");
  DescribeIO io{tokens, B, N};
  const DescribePlan p = plan_describe(ctx, io, false, Passes::AssignOnly);
  if (p.code != SEGVLAD_OK) return ctx->fail(p.code, "%s", p.why);
  // pinned landing zone of the flags and the centroids (read by segvlad_describe_flags while the assignment pass runs)
  const size_t need = (size_t)B + (size_t)S_tot * 16 + 64;
  if (need > ctx->h_desc_cap) {
    if (ctx->h_desc) SV_HIP(hipHostFree(ctx->h_desc));
    ctx->h_desc = nullptr, ctx->h_desc_cap = 0;
    SV_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_desc), need + need / 2, hipHostMallocDefault));
    ctx->h_desc_cap = need + need / 2;
  }
  if (!ctx->ev_desc) SV_HIP(hipEventCreateWithFlags(&ctx->ev_desc, hipEventDisableTiming));
  // stage "describe": from here to the end of segvlad_describe_end, as the context's stream sees it (the parts overlap)
  OpenDescribe& d = ctx->desc;
  d.open = true, d.B = B, d.S_tot = S_tot;
  d.timer = sv_stage_open(ctx, "describe", &d.slot);
  int rc = pass_mask_branch(ctx, m, S_tot);
  if (rc == SEGVLAD_OK) rc = run_describe(ctx, p, io);   // main stream: the assignment pass
  return rc == SEGVLAD_OK ? rc : close_describe(ctx, false, rc);
}

extern "C" {
int segvlad_incidence(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch, uint64_t* inc_bits) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("incidence");
  SV_TRY(incidence_run(ctx, masks, S, Hm, Wm, H, W, patch, inc_bits, nullptr, false));
  return S == 0 ? SEGVLAD_OK : sv_finish(ctx);
}
int segvlad_incidence_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch, uint64_t* inc_bits,
                                double* centroids) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("incidence_centroids");
  SV_TRY(incidence_run(ctx, masks, S, Hm, Wm, H, W, patch, inc_bits, centroids, true));
  return S == 0 ? SEGVLAD_OK : sv_finish(ctx);
}

int segvlad_mask_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, double* centroids) {
  CHECK_CTX();
  if (S < 0 || Hm <= 0 || Wm <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "mask_centroids: bad geometry");
  if (S == 0) return SEGVLAD_OK;
  if (!masks || !centroids) return ctx->fail(SEGVLAD_ERR_ARG, "mask_centroids: null pointer");
  const void* dm;
  void* dout;
  SV_TRY(sv_in(ctx, masks, (size_t)S * Hm * Wm, &dm));
  SV_TRY(sv_out(ctx, centroids, (size_t)S * 2 * sizeof(double), &dout));
  SV_TRY(sv_launch_centroids(ctx, (const uint8_t*)dm, S, Hm, Wm, (double*)dout));
  return sv_finish(ctx);
}

int segvlad_adjacency(segvlad_ctx* ctx, const double* centroids, const int32_t* seg_offsets, int B, int order, uint8_t* adj_out,
                      uint32_t* n_empty_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("adjacency");
  SV_TRY(adjacency_run(ctx, centroids, seg_offsets, B, order, adj_out, nullptr));
  if (B == 0 || seg_offsets[B] == 0) return SEGVLAD_OK;   // nothing was enqueued
  if (n_empty_out) SV_HIP(hipMemcpyAsync(n_empty_out, ctx->s_flag.as<uint32_t>() + 4, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (n_empty_out) SV_HIP(hipStreamSynchronize(ctx->stream));
  return sv_finish(ctx);
}
int segvlad_adjacency_flagged(segvlad_ctx* ctx, const double* centroids, const int32_t* seg_offsets, int B, int order,
                              uint8_t* adj_out, uint8_t* img_flags_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("adjacency_flagged");
  if (B > 0 && !img_flags_out) return ctx->fail(SEGVLAD_ERR_ARG, "adjacency_flagged: null img_flags_out");
  SV_TRY(adjacency_run(ctx, centroids, seg_offsets, B, order, adj_out, img_flags_out));
  return (B == 0 || seg_offsets[B] == 0) ? SEGVLAD_OK : sv_finish(ctx);
}

int segvlad_images(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits, const int32_t* seg_offsets,
                   const uint8_t* adj, float* out, uint8_t* labels_out, float* gap_out, float* block_norms_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("images");
  DescribeIO io{tokens, B, N, inc_bits, seg_offsets, adj, out, labels_out, gap_out, block_norms_out, nullptr, 0};
  return describe_whole(ctx, io, false);
}
// y: the projected rows; desc_out may be NULL (the K*D-wide descriptor then never reaches HBM in the fused forms)
int segvlad_images_pca(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits, const int32_t* seg_offsets,
                       const uint8_t* adj, float* y, int l2norm, float* desc_out, uint8_t* labels_out, float* gap_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("images_pca");
  DescribeIO io{tokens, B, N, inc_bits, seg_offsets, adj, desc_out, labels_out, gap_out, nullptr, y, l2norm};
  return describe_whole(ctx, io, true);
}

int segvlad_describe_begin(segvlad_ctx* ctx, const uint8_t* masks, int Hm, int Wm, int H, int W, int patch, const float* tokens, int B,
                           int N, const int32_t* seg_offsets, int order, uint64_t* inc_bits_out, double* centroids_out, uint8_t* adj_out,
                           uint8_t* img_flags_out, int pca) {
  CHECK_CTX();
  const MaskBranch m{masks, Hm, Wm, H, W, patch, seg_offsets, B, order, inc_bits_out, centroids_out, adj_out, img_flags_out};
  SV_TRY(describe_begin(ctx, m, tokens, N, pca != 0));
  const int rc = sv_finish(ctx);
  return rc == SEGVLAD_OK ? rc : close_describe(ctx, false, rc);
}

int segvlad_describe_flags(segvlad_ctx* ctx, uint8_t* flags_host, double* centroids_host) {
  CHECK_CTX();
  if (!ctx->desc.open) return ctx->fail(SEGVLAD_ERR_STATE, "describe_flags: call segvlad_describe_begin first");
  if (!flags_host) return ctx->fail(SEGVLAD_ERR_ARG, "describe_flags: null pointer");
  SV_HIP(hipEventSynchronize(ctx->ev_desc));   // the MASK BRANCH only: the assignment pass on the main stream keeps running
  memcpy(flags_host, ctx->h_desc, (size_t)ctx->desc.B);
  if (centroids_host) memcpy(centroids_host, ctx->h_desc + (((size_t)ctx->desc.B + 63) & ~(size_t)63), (size_t)ctx->desc.S_tot * 16);
  return SEGVLAD_OK;
}

int segvlad_describe_end(segvlad_ctx* ctx, const float* tokens, int B, int N, const uint64_t* inc_bits, const int32_t* seg_offsets,
                         uint8_t* adj, int n_patch, const int32_t* patch_images, const uint8_t* patch_blocks, float* desc_out, float* y,
                         int l2norm) {
  CHECK_CTX();
  if (!ctx->desc.open) return ctx->fail(SEGVLAD_ERR_STATE, "describe_end: call segvlad_describe_begin first");
  auto bail = [&](int rc) { return close_describe(ctx, false, rc); };   // the context stays usable: the split call is over
  if (!tokens || !inc_bits || !seg_offsets || !adj || (!desc_out && !y) || B != ctx->desc.B || seg_offsets[B] != ctx->desc.S_tot ||
      n_patch < 0 || (n_patch > 0 && (!patch_images || !patch_blocks)))
    return bail(ctx->fail(SEGVLAD_ERR_ARG, "describe_end: arguments do not match segvlad_describe_begin's"));
  DescribeIO io{tokens, B, N, inc_bits, seg_offsets, adj, desc_out, nullptr, nullptr, nullptr, y, l2norm};
  const DescribePlan p = plan_describe(ctx, io, y != nullptr, Passes::FromPrep);
  if (p.code != SEGVLAD_OK) return bail(ctx->fail(p.code, "%s", p.why));
  if (n_patch > 0) {
    // adjacency blocks the caller recomputed on the host (Qhull, for images whose centroids are in a non-generic configuration):
    // written over the device kernel's behind the mask branch, in front of prep
    if (join_mask_branch(ctx) != SEGVLAD_OK) return bail(SEGVLAD_ERR_HIP);
    size_t src = 0;
    for (int j = 0; j < n_patch; ++j) {
      const int b = patch_images[j];
      if (b < 0 || b >= B) return bail(ctx->fail(SEGVLAD_ERR_ARG, "describe_end: patch image %d out of range", b));
      const size_t bytes = (size_t)(p.adj_off[(size_t)b + 1] - p.adj_off[(size_t)b]);
      const hipError_t e = hipMemcpyAsync(adj + p.adj_off[(size_t)b], patch_blocks + src, bytes, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) return bail(ctx->fail(SEGVLAD_ERR_HIP, "describe_end: adjacency patch: %s", hipGetErrorString(e)));
      src += bytes;
    }
  }
  SV_TRY(close_describe(ctx, true, run_describe(ctx, p, io)));
  return sv_finish(ctx);
}

int segvlad_describe(segvlad_ctx* ctx, const uint8_t* masks, int Hm, int Wm, int H, int W, int patch, const float* tokens, int B, int N,
                     const int32_t* seg_offsets, int order, uint64_t* inc_bits_out, double* centroids_out, uint8_t* adj_out,
                     uint8_t* img_flags_out, float* desc_out, float* y, int l2norm) {
  CHECK_CTX();
  if (!desc_out && !y) return ctx->fail(SEGVLAD_ERR_ARG, "describe: null pointer");
  if ((desc_out && !sv_is_device_ptr(desc_out)) || (y && !sv_is_device_ptr(y)))
    return ctx->fail(SEGVLAD_ERR_ARG, "describe: bulk pointers must be device memory (the separate entry points stage host data)");
  const MaskBranch m{masks, Hm, Wm, H, W, patch, seg_offsets, B, order, inc_bits_out, centroids_out, adj_out, img_flags_out};
  SV_TRY(describe_begin(ctx, m, tokens, N, y != nullptr));
  return segvlad_describe_end(ctx, tokens, B, N, inc_bits_out, seg_offsets, adj_out, 0, nullptr, nullptr, desc_out, y, l2norm);
}

// ---- vocabulary k-means: one Lloyd half-step over a batch of images (utilities.py:749-791, vlad_c_centers_pt_gen.py:86-158) -------
int segvlad_kmeans_step(segvlad_ctx* ctx, const float* tokens, int B, int N, double* sums, int64_t* counts, uint8_t* labels_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("kmeans_step");
  if (ctx->K == 0) return ctx->fail(SEGVLAD_ERR_STATE, "kmeans_step: call segvlad_set_vocab with the current centres first");
  if (B < 0 || N <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "kmeans_step: B=%d N=%d", B, N);
  if (B == 0) return SEGVLAD_OK;
  if (!tokens || !sums || !counts) return ctx->fail(SEGVLAD_ERR_ARG, "kmeans_step: null pointer");
  if (!sv_is_device_ptr(sums) || !sv_is_device_ptr(counts))
    return ctx->fail(SEGVLAD_ERR_ARG, "kmeans_step: sums / counts are accumulated into and must be device memory");
  DescribeIO io{tokens, B, N};
  const DescribePlan p = plan_describe(ctx, io, false, Passes::AssignOnly);
  if (p.code != SEGVLAD_OK) return ctx->fail(p.code, "%s", p.why);
  SV_TRY(run_describe(ctx, p, io));   // the assignment pass: labels, Xt, 1 / ||x|| in the context's scratch
  {
    StageScope sc(ctx, "kmeans");
    SV_TRY(sv_launch_centroid_sums(ctx, ctx->s_xt.as<float>(), ctx->s_rnorm.as<float>(), ctx->s_labels.as<uint8_t>(), B, N, p.D, p.K, sums, counts));
    sc.count(2);
  }
  if (labels_out) {
    void* d_lab = nullptr;
    SV_TRY(sv_out(ctx, labels_out, (size_t)B * N, &d_lab));
    SV_HIP(hipMemcpyAsync(d_lab, ctx->s_labels.p, (size_t)B * N, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return sv_finish(ctx);
}

}  // extern "C"

// ---- K-parametric aggregation of given residuals + labels (vlad_matmuls_per_cluster) --------------------
__global__ void fill_ones_kernel(float* p, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) p[j] = 1.f;
}

extern "C" int segvlad_cluster_aggregate(segvlad_ctx* ctx, int num_c, const float* res, const uint8_t* labels, int N, int D,
                                         const uint64_t* inc_bits, int S, const uint8_t* adj, float* out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("cluster_aggregate");
  if (num_c <= 0 || num_c > 256 || N <= 0 || D <= 0 || (D % 4) || S < 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "cluster_aggregate: bad shape num_c=%d N=%d D=%d S=%d", num_c, N, D, S);
  if (S == 0) return SEGVLAD_OK;
  if (!res || !labels || !inc_bits || !out) return ctx->fail(SEGVLAD_ERR_ARG, "cluster_aggregate: null pointer");
  const int nw = (N + 63) / 64, SC = (S + 63) / 64;
  const void *d_res, *d_lab, *d_inc, *d_adj = nullptr;
  void* d_out;
  SV_TRY(sv_in(ctx, res, (size_t)N * D * 4, &d_res));
  SV_TRY(sv_in(ctx, labels, (size_t)N, &d_lab));
  SV_TRY(sv_in(ctx, inc_bits, (size_t)S * nw * 8, &d_inc));
  if (adj) SV_TRY(sv_in(ctx, adj, (size_t)S * S, &d_adj));
  SV_TRY(sv_out(ctx, out, (size_t)S * num_c * D * 4, &d_out));
  SV_HIP(ctx->s_rnorm.reserve((size_t)N * 4));
  SV_HIP(ctx->s_colmask.reserve((size_t)N * SC * 8));
  SV_HIP(ctx->s_gscale.reserve((size_t)(S + 1) * 4));
  SV_HIP(ctx->s_segoff.reserve(2 * sizeof(int32_t)));
  SV_HIP(ctx->s_adjoff.reserve(2 * sizeof(int64_t)));
  const int32_t so[2] = {0, S};
  const int64_t ao[2] = {0, (int64_t)S * S};
  SV_HIP(hipMemcpyAsync(ctx->s_segoff.p, so, sizeof(so), hipMemcpyHostToDevice, ctx->stream));
  SV_HIP(hipMemcpyAsync(ctx->s_adjoff.p, ao, sizeof(ao), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(fill_ones_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, ctx->s_rnorm.as<float>(), N);
  SV_TRY(sv_launch_prep(ctx, (const uint8_t*)d_lab, (const uint64_t*)d_inc, ctx->s_segoff.as<int32_t>(), ctx->s_adjoff.as<int64_t>(),
                        (const uint8_t*)d_adj, 1, N, num_c, S, SC, ctx->s_colmask.as<uint64_t>(), ctx->s_gscale.as<float>(), nullptr, nullptr, 0));
  SV_TRY(sv_launch_aggregate(ctx, (const float*)d_res, ctx->s_colmask.as<uint64_t>(), nullptr, num_c, D, ctx->s_segoff.as<int32_t>(),
                             ctx->s_gscale.as<float>(), 1, N, SC, (float*)d_out, nullptr));
  SV_HIP(hipStreamSynchronize(ctx->stream));  // so[] / ao[] live on this frame
  return sv_finish(ctx);
}
