// Grouped search (segvlad_search_grouped): per query row the nearest index rows such that no reference image appears more than
// per_image times -- the group_by / collapse of retrieval engines.  No reference counterpart: the reference's vote adds one
// similarity per HIT (get_matches, func_vpr.py:207-224), so on a redundant map one query segment gives one image dozens of votes.
//
// The rule, on the unbounded (squared L2, lower id) ordered list L(q) of segvlad_search: an entry is KEPT when fewer than per_image
// EARLIER entries of L(q) carry its image id (db_img); a row with a negative image id is a group of its own.  The result is the
// first k kept entries in their order -- a subsequence of an ordered list is ordered -- and (+inf, -1) behind them.  An entry with
// per_image or more earlier entries of its image has per_image earlier KEPT ones, so the decision is a function of the list alone.
//
//   inner search         segvlad_search's body, unchanged, at depth k_fetch = min(1024, 4 k) into scratch (option group_fetch, tests)
//   group_collapse_kernel  one wave per row walks (list_walk_dev.h) the k_fetch entries in chunks of 64.  Earlier entries of an entry's image =
//                        the count the earlier chunks left in the wave's LDS table + the lower lanes of this chunk with the same
//                        id.  Both depend on list positions only; the one atomic (claiming a table slot) decides WHERE an id's
//                        count lives, never its value.  Kept entries are placed by ballot + mbcnt, the walk stops at k kept.
//                        A row that kept k, or whose list reached the index's end (a -1 slot, or k_fetch >= the index), is
//                        COMPLETE; any other row with a finite squared norm is OPEN: flagged and counted
//   exact tail           (the correctness backstop.)  The open rows, gathered, in batches: the range search's exact sweep
//                        (sv_range_exact_sweep, search.hip) under an infinite radius emits every index row's (distance bits << 32
//                        | id) word -- the search's own arithmetic, no second distance kernel --, sv_range_sort_segments orders
//                        each row's n words, group_tail_kernel applies the same rule with one byte per image in global scratch and
//                        writes the first k kept into the open row's output slots.  A batch holds as many rows as keep its two
//                        word buffers and its counts (2 x 8 n + db_img_max + 1 bytes per row) within GR_TAIL_BYTES = 1 GiB, at
//                        least one.
//
// LDS: a wave's table is 2048 slots (a list of <= 1024 entries holds <= 1024 ids: load <= 1/2) of a 4-byte key + a 2-byte count,
// 12 KiB; four waves per workgroup, 48 KiB of the CU's 160: three workgroups per CU.  The slot of an id is the top 11 bits of
// id x 0x9E3779B1: consecutive image ids -- neighbours in time, what crowds a list -- land a golden-ratio step apart, spread over
// the 32 banks of the 4-byte reads; lanes of one image read one address, which broadcasts.
// The entry points (segvlad_search_grouped, segvlad_group_stats) are at the end of this file.
#include <algorithm>
#include <vector>

#include "ctx.h"
#include "list_walk_dev.h"

namespace {

constexpr int GR_SLOTS = 2048;
constexpr int GR_WAVES = 4;
constexpr size_t GR_TAIL_BYTES = (size_t)1 << 30;

// among the lanes of a wave: how many LOWER lanes carry this lane's g (rank), how many lanes in all (tot).  Lanes with g < 0 take
// no part (their results are unused).
__device__ __forceinline__ void gr_chunk_counts(int g, int lane, int& rank, int& tot) {
  rank = 0;
  tot = 0;
#pragma unroll
  for (int l = 0; l < 64; ++l) {
    const int same = (__builtin_amdgcn_readlane(g, l) == g) ? 1 : 0;
    tot += same;
    rank += (l < lane) ? same : 0;
  }
}

__device__ __forceinline__ uint32_t gr_slot(int g) { return ((uint32_t)g * 0x9E3779B1u) >> 21; }   // 0 .. GR_SLOTS - 1

// head: [0] open rows, [1] the most entries a complete row read.  whole: k_fetch covers the index (no row can be open)
__global__ __launch_bounds__(64 * GR_WAVES) void group_collapse_kernel(const float* __restrict__ d2f, const int64_t* __restrict__ idxf,
                                                                      int nq, int kf, int k, int per_image, int whole,
                                                                      const int32_t* __restrict__ db_img, const float* __restrict__ qn,
                                                                      float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                                      uint32_t* __restrict__ head, uint32_t* __restrict__ flags) {
  __shared__ int32_t s_key[GR_WAVES][GR_SLOTS];
  __shared__ uint16_t s_cnt[GR_WAVES][GR_SLOTS];
  const int w = (int)(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int q = (int)blockIdx.x * GR_WAVES + w;
  if (q >= nq) return;
  int32_t* key = s_key[w];
  uint16_t* cnt = s_cnt[w];
  for (int j = l; j < GR_SLOTS; j += 64) key[j] = -1;
  __threadfence_block();
  const SvListArrays list = {d2f + (size_t)q * kf, idxf + (size_t)q * kf, kf};
  const auto wk = sv_list_walk(list, [&](int64_t id, bool real) {
    const int g = real ? db_img[id] : -1;
    // the count the earlier chunks left for this image
    int prior = 0;
    uint32_t h = 0;
    if (g >= 0) {
      h = gr_slot(g);
      int32_t kk;
      while ((kk = key[h]) != -1 && kk != g) h = (h + 1) & (GR_SLOTS - 1);
      if (kk == g) prior = cnt[h];
    }
    int rank, tot;
    gr_chunk_counts(g, l, rank, tot);
    // the image's first lane of the chunk leaves the new count (h: the first slot that was free or the image's own at the lookup;
    // another image's leader may take a free one first -- then this one moves on, and only the place differs)
    if (g >= 0 && rank == 0) {
      for (;;) {
        const int32_t old = atomicCAS(&key[h], -1, g);
        if (old == -1 || old == g) break;
        h = (h + 1) & (GR_SLOTS - 1);
      }
      cnt[h] = (uint16_t)(prior + tot);
    }
    __threadfence_block();
    return real && (g < 0 || prior + rank < per_image);
  }, k, l, d2_out + (size_t)q * k, idx_out + (size_t)q * k);
  if (l == 0) {
    const bool complete = wk.kept >= k || wk.ended || whole != 0;
    const bool open = !complete && fabsf(qn[q]) < INFINITY;   // (false for a NaN norm, too)
    flags[q] = open ? 1u : 0u;
    if (open) atomicAdd(&head[0], 1u);
    if (complete) atomicMax(&head[1], (uint32_t)wk.read);
  }
}

// a batch's slots 0 .. nb - 1 and where each one's n words start
__global__ __launch_bounds__(256) void group_plan_kernel(int nb, int64_t n, int64_t* __restrict__ woff, int32_t* __restrict__ slot) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t <= nb) woff[t] = (int64_t)t * n;
  if (t < nb) slot[t] = t;
}

// One wave per open row of a batch: the rule over the row's n ordered words (all-ones words: slots the sweep did not fill -- a
// distance that is NaN or +inf --, ordered behind every entry).  tab: per row nimg bytes, zero on entry, an image's count so far
// (held at 255).  The first k kept go to the row's output slots, (+inf, -1) behind them.
__global__ __launch_bounds__(64) void group_tail_kernel(const unsigned long long* __restrict__ sorted, int64_t n, int k, int per_image,
                                                        const int32_t* __restrict__ db_img, uint8_t* __restrict__ tab, int64_t nimg,
                                                        const int32_t* __restrict__ rows, float* __restrict__ d2_out,
                                                        int64_t* __restrict__ idx_out) {
  const int l = threadIdx.x;
  const SvListWords list = {sorted + (size_t)blockIdx.x * (size_t)n, n};
  uint8_t* tb = tab + (size_t)blockIdx.x * (size_t)nimg;
  const int64_t q = rows[blockIdx.x];
  sv_list_walk(list, [&](int64_t id, bool real) {
    const int g = real ? db_img[id] : -1;
    const int prior = g >= 0 ? (int)tb[g] : 0;
    int rank, tot;
    gr_chunk_counts(g, l, rank, tot);
    if (g >= 0 && rank == 0) tb[g] = (uint8_t)min(prior + tot, 255);
    __threadfence_block();   // (the next chunk's lanes read what this chunk's leaders wrote: one wave, one L1)
    return real && (g < 0 || prior + rank < per_image);
  }, k, l, d2_out + (size_t)q * k, idx_out + (size_t)q * k);
}

}   // namespace

// segvlad_search_grouped after the argument checks: Q / outputs on the device, nq >= 1, the index holds rows and an img_of_seg map;
// fills ctx->gr_stats; synchronises
static int search_grouped(segvlad_ctx* ctx, const float* Q, int nq, int k, int per_image, float* d2_out, int64_t* idx_out) {
  const int d = ctx->db_d;
  const int64_t n = ctx->db_n;
  const int gf = ctx->opt.group_fetch;
  const int kf = gf > 0 ? std::min(1024, std::max(k, gf)) : std::min(1024, 4 * k);
  ctx->gr_stats[0] = kf;   // ([1], [2]: cleared by the entry point)

  SV_HIP(ctx->s_deep_d2.reserve((size_t)nq * kf * 4));
  SV_HIP(ctx->s_deep_idx.reserve((size_t)nq * kf * 8));
  SV_TRY(sv_search_dev(ctx, Q, nq, kf, ctx->s_deep_d2.as<float>(), ctx->s_deep_idx.as<int64_t>()));

  // words 0 .. 3: the open-row counter and the longest read (segvlad_group_stats); words 4 ..: the rows' flags
  SV_HIP(ctx->s_gr_flag.reserve(((size_t)nq + 4) * 4));
  SV_HIP(ctx->s_deep_qn.reserve((size_t)nq * 4));
  uint32_t* head = ctx->s_gr_flag.as<uint32_t>();
  float* qn = ctx->s_deep_qn.as<float>();
  std::vector<uint32_t> hf((size_t)nq + 4);
  StageScope sc(ctx, "knn_group");
  SV_HIP(hipMemsetAsync(head, 0, 16, ctx->stream));
  // (from Q itself: the norms of a view that is not 16-byte aligned are summed in another order, and the tail's rows must carry
  //  the values segvlad_search gives the same pointer)
  SV_TRY(sv_launch_row_sumsq(ctx, Q, nq, d, qn));
  hipLaunchKernelGGL(group_collapse_kernel, dim3((unsigned)((nq + GR_WAVES - 1) / GR_WAVES)), dim3(64 * GR_WAVES), 0, ctx->stream,
                     ctx->s_deep_d2.as<float>(), ctx->s_deep_idx.as<int64_t>(), nq, kf, k, per_image, (int64_t)kf >= n ? 1 : 0,
                     ctx->db_img.as<int32_t>(), qn, d2_out, idx_out, head, head + 4);
  SV_HIP(hipGetLastError());
  sc.count(2);
  SV_HIP(hipMemcpyAsync(hf.data(), head, hf.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  ctx->gr_stats[2] = hf[1];
  if (hf[0] == 0) return SEGVLAD_OK;

  // ---- the exact tail ----
  std::vector<int32_t> rows;
  for (int r = 0; r < nq; ++r)
    if (hf[(size_t)r + 4]) rows.push_back(r);
  const size_t nf = rows.size();
  ctx->gr_stats[1] = (int64_t)nf;
  const size_t nimg = (size_t)std::max<int64_t>((int64_t)ctx->db_img_max + 1, 1);
  // rows of a batch: both word buffers and the per-image counts within GR_TAIL_BYTES, the segmented sort's 32-bit word count, at
  // least one
  const size_t nb = std::max<size_t>(1, std::min({nf, GR_TAIL_BYTES / ((size_t)n * 16 + nimg), (size_t)(0xffffffffLL / n)}));
  SV_HIP(ctx->s_gr_rows.reserve(nf * 4));
  SV_HIP(ctx->s_gr_q.reserve(nf * ((size_t)d + 2) * 4));
  SV_HIP(ctx->s_gr_plan.reserve((nb + 1) * 8 + nb * 4));
  SV_HIP(ctx->s_gr_cur.reserve(nb * 4));
  SV_HIP(ctx->s_gr_words.reserve(nb * (size_t)n * 8));
  SV_HIP(ctx->s_gr_sorted.reserve(nb * (size_t)n * 8));
  SV_HIP(ctx->s_gr_tab.reserve(nb * nimg));
  int32_t* drows = ctx->s_gr_rows.as<int32_t>();
  float* qx = ctx->s_gr_q.as<float>();
  float* qnx = qx + nf * d;
  float* effx = qnx + nf;
  int64_t* woff = ctx->s_gr_plan.as<int64_t>();
  int32_t* slot = reinterpret_cast<int32_t*>(woff + nb + 1);
  uint64_t* words = ctx->s_gr_words.as<uint64_t>();
  uint64_t* sorted = ctx->s_gr_sorted.as<uint64_t>();
  SV_HIP(hipMemcpyAsync(drows, rows.data(), nf * 4, hipMemcpyHostToDevice, ctx->stream));
  SV_TRY(sv_launch_range_gather(ctx, Q, qn, /*eff=*/nullptr, drows, (int)nf, d, qx, qnx, effx));   // every open row: an infinite radius
  hipLaunchKernelGGL(group_plan_kernel, dim3((unsigned)(nb / 256 + 1)), dim3(256), 0, ctx->stream, (int)nb, n, woff, slot);
  SV_HIP(hipGetLastError());
  sc.count(2);
  for (size_t t0 = 0; t0 < nf; t0 += nb) {
    const size_t m = std::min(nb, nf - t0);
    SV_HIP(hipMemsetAsync(words, 0xff, m * (size_t)n * 8, ctx->stream));
    SV_HIP(hipMemsetAsync(ctx->s_gr_cur.p, 0, m * 4, ctx->stream));
    SV_HIP(hipMemsetAsync(ctx->s_gr_tab.p, 0, m * nimg, ctx->stream));
    int launches = 0;
    SV_TRY(sv_range_exact_sweep(ctx, qx + t0 * d, qnx + t0, effx + t0, slot, (int)m, nullptr, woff, ctx->s_gr_cur.as<uint32_t>(), words,
                                &launches));
    SV_TRY(sv_range_sort_segments(ctx, words, sorted, (int64_t)m * n, (int)m, woff));
    hipLaunchKernelGGL(group_tail_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream,
                       reinterpret_cast<const unsigned long long*>(sorted), n, k, per_image, ctx->db_img.as<int32_t>(),
                       ctx->s_gr_tab.as<uint8_t>(), (int64_t)nimg, drows + t0, d2_out, idx_out);
    SV_HIP(hipGetLastError());
    sc.count(launches + 2);
  }
  SV_HIP(hipStreamSynchronize(ctx->stream));   // rows[] lives on this frame
  return SEGVLAD_OK;
}

extern "C" int segvlad_search_grouped(segvlad_ctx* ctx, const float* Q, int nq, int k, int per_image, float* d2_out,
                                      int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || k < 1 || k > 1024 || per_image < 1 || per_image > 16)
    return ctx->fail(SEGVLAD_ERR_ARG, "search_grouped: need nq >= 0, 1<=k<=1024, 1<=per_image<=16 (k=%d, per_image=%d)", k, per_image);
  SV_TRY(sv_check_img_index(ctx, "search_grouped"));
  if (ctx->db_n > 0xffffffffLL) return ctx->fail(SEGVLAD_ERR_LIMIT, "search_grouped: %lld index rows (candidate ids are 32-bit)", (long long)ctx->db_n);
  ctx->gr_stats[0] = ctx->gr_stats[1] = ctx->gr_stats[2] = 0;
  if (nq == 0) return SEGVLAD_OK;
  if (!Q || !d2_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "search_grouped: null pointer");
  const void* dq;
  void *dd2, *didx;
  SV_TRY(sv_in(ctx, Q, (size_t)nq * ctx->db_d * 4, &dq));
  SV_TRY(sv_out(ctx, d2_out, (size_t)nq * k * 4, &dd2));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k * 8, &didx));
  if (ctx->db_n == 0) {   // emptied by segvlad_db_remove: no row anywhere
    SV_HIP(sv_fill_none(ctx, (float*)dd2, (int64_t*)didx, (size_t)nq * k));
    return sv_finish(ctx);
  }
  SV_TRY(search_grouped(ctx, (const float*)dq, nq, k, per_image, (float*)dd2, (int64_t*)didx));
  return sv_finish(ctx);
}

extern "C" int segvlad_group_stats(segvlad_ctx* ctx, int64_t* stats_out, int n) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  if (!stats_out || n < 0) return ctx->fail(SEGVLAD_ERR_ARG, "group_stats: bad arguments");
  for (int i = 0; i < n && i < 3; ++i) stats_out[i] = ctx->gr_stats[i];
  return SEGVLAD_OK;
}
