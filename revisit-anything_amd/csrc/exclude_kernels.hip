// Search excluding image-id windows per query image (segvlad_search_excluding).  No reference counterpart: the reference searches
// the whole index (place_rec_main.py:53-60); this is the self-query of a live map -- loop closure, leave-one-out checks -- where a
// query image's own rows and those of its neighbours in time are in the index and must not be matched.  Every query IMAGE names
// up to 8 inclusive intervals of reference image ids; the result is what a fresh index without those images returns.
//
//   host            per query image: its intervals clamped to the ids the index holds, sorted and merged; X_b = the index rows they
//                   cover, from the host copy of the image -> row map's offsets (shortlist_kernels.hip; copied once per index
//                   change).  k_fetch = min(1024, k + max_b X_b).  No read-back per call
//   inner search    segvlad_search's body, unchanged, at depth k_fetch into scratch.  A list of k_fetch entries holds at most X_b
//                   excluded ones: where k + X_b <= k_fetch the first k allowed entries of the list ARE the answer
//   ex_compact_kernel   one wave per row walks (list_walk_dev.h) the k_fetch entries in order, drops those whose image (db_img) lies in
//                   one of the image's merged intervals, writes the first k kept in their order -- a subsequence of a (distance, id)
//                   ordered list is ordered -- and (+inf, -1) behind them.  A row that kept k, or whose list ran into the index's
//                   end (a -1 slot), or whose image has k + X_b <= k_fetch is complete; any other row is SHORT: flagged and counted
//   exact tail      (only images with k + X_b > 1024 can flag a row: a window of more than 1024 - k rows -- 21 images of 50 rows at
//                   k = 50 -- that also crowds the allowed rows out of the row's nearest 1024.)  The shortlist search's exact fp32
//                   MFMA GEMM (sl_gemm_kernel<., true>) over the ALLOWED rows -- the complement of <= 8 intervals is <= 9 ranges of
//                   the map's positions -- for the groups (<= 64 rows of one image) of those images only; a group without a flagged
//                   row leaves at once, nothing is read back.  sl_final_kernel orders the lists, ex_scatter_kernel moves the flagged
//                   rows' results into place.  This is the correctness backstop, not the fast path: a group that runs streams the
//                   allowed part of the index in fp32 once (4 GB at 1 M x 1024).
// The entry points (segvlad_search_excluding, segvlad_exclude_stats) are at the end of this file.
#include <algorithm>
#include <utility>
#include <vector>

#include "ctx.h"
#include "list_walk_dev.h"

namespace {

// per query image: its merged intervals (unused ones empty: lo 1, hi 0), and whether k + X_b <= k_fetch
struct ExImg {
  int32_t safe;
  int32_t pad;
  int32_t lo[SV_EX_MAX_E], hi[SV_EX_MAX_E];
};

// flags == nullptr: no image can leave a row short (k + X_b <= k_fetch for all of them)
__global__ __launch_bounds__(256) void ex_compact_kernel(const float* __restrict__ d2f, const int64_t* __restrict__ idxf, int nq, int kf,
                                                         int k, const int32_t* __restrict__ qoff, int n_img,
                                                         const ExImg* __restrict__ imgs, const int32_t* __restrict__ db_img,
                                                         float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                         uint32_t* __restrict__ flags, uint32_t* __restrict__ n_short) {
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), l = threadIdx.x & 63;
  if (q >= nq) return;
  int a = 1, b = n_img;   // the first j with qoff[j] > q: the row belongs to image j - 1
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (qoff[mid] > q) b = mid;
    else a = mid + 1;
  }
  const ExImg im = imgs[a - 1];
  const SvListArrays list = {d2f + (size_t)q * kf, idxf + (size_t)q * kf, kf};
  // the rule: an entry is kept unless its image lies in one of the merged intervals
  const auto w = sv_list_walk(list, [&](int64_t id, bool real) {
    bool keep = false;
    if (real) {
      const int g = db_img[id];
      keep = true;
#pragma unroll
      for (int e = 0; e < SV_EX_MAX_E; ++e) keep = keep && !(g >= im.lo[e] && g <= im.hi[e]);
    }
    return keep;
  }, k, l, d2_out + (size_t)q * k, idx_out + (size_t)q * k);
  if (flags && l == 0) {
    const bool is_short = w.kept < k && !w.ended && !im.safe;
    flags[q] = is_short ? 1u : 0u;
    if (is_short) atomicAdd(n_short, 1u);
  }
}

// the tail's slot t holds query row slot_q[t]: a flagged row takes its k results from there
__global__ __launch_bounds__(64) void ex_scatter_kernel(const int32_t* __restrict__ slot_q, const uint32_t* __restrict__ flags, int k,
                                                        const float* __restrict__ d2_tmp, const int64_t* __restrict__ idx_tmp,
                                                        float* __restrict__ d2_out, int64_t* __restrict__ idx_out) {
  const size_t t = blockIdx.x;
  const int q = slot_q[t];
  if (!flags[q]) return;
  for (int j = threadIdx.x; j < k; j += 64) {
    d2_out[(size_t)q * k + j] = d2_tmp[t * k + j];
    idx_out[(size_t)q * k + j] = idx_tmp[t * k + j];
  }
}

// the intervals of one query image, clamped to 0 .. nimg - 1, sorted and merged (adjacent ones too); returns how many
int merge_intervals(const int32_t* iv, int E, int nimg, std::pair<int, int>* out) {
  std::pair<int, int> a[SV_EX_MAX_E];
  int n = 0;
  for (int e = 0; e < E; ++e) {
    const int lo = std::max(iv[2 * e], 0), hi = std::min(iv[2 * e + 1], nimg - 1);
    if (lo <= hi) a[n++] = {lo, hi};
  }
  std::sort(a, a + n);
  int m = 0;
  for (int e = 0; e < n; ++e) {
    if (m > 0 && a[e].first <= out[m - 1].second + 1) out[m - 1].second = std::max(out[m - 1].second, a[e].second);
    else out[m++] = a[e];
  }
  return m;
}

}   // namespace

// segvlad_search_excluding after the argument checks: Q on the device, qoff / excl host, outputs on the device, the index holds rows
static int search_excluding(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qoff, int n_img, const int32_t* excl, int E, int k,
                            float* d2_out, int64_t* idx_out) {
  const int d = ctx->db_d;
  SV_TRY(sv_sl_map_host(ctx));
  const int nimg = ctx->db_img_max + 1;
  const uint32_t* off = ctx->sl_off_host.data();
  // per query image: merged intervals and X_b (images without query rows do not count)
  std::vector<std::pair<int, int>> merged((size_t)n_img * SV_EX_MAX_E);
  std::vector<int> nm(n_img);
  std::vector<int64_t> X(n_img);
  int64_t xmax = 0, n_excl = 0;
  for (int b = 0; b < n_img; ++b) {
    std::pair<int, int>* mb = merged.data() + (size_t)b * SV_EX_MAX_E;
    nm[b] = merge_intervals(excl + (size_t)b * E * 2, E, nimg, mb);
    int64_t x = 0;
    for (int e = 0; e < nm[b]; ++e) x += (int64_t)off[mb[e].second + 1] - (int64_t)off[mb[e].first];
    X[b] = x;
    if (qoff[b + 1] > qoff[b]) {
      xmax = std::max(xmax, x);
      n_excl += x > 0;
    }
  }
  const int kf = (int)std::min<int64_t>(1024, k + xmax);
  ctx->ex_stats[0] = kf;   // ([2] and ctx->ex_short_dev: cleared by the entry point)
  ctx->ex_stats[1] = xmax;
  ctx->ex_stats[3] = n_excl;
  if (xmax == 0) return sv_search_dev(ctx, Q, nq, k, d2_out, idx_out);   // nothing is excluded anywhere: the plain search

  // images that can leave a row short, their groups (as segvlad_search_shortlist's) and allowed ranges of map positions
  std::vector<int32_t> groups, slot_q;
  std::vector<uint32_t> unum, uoff, ustart;
  int gmax = 0, n_slots = 0;
  for (int b = 0; b < n_img; ++b) {
    const int rws = qoff[b + 1] - qoff[b];
    if (rws <= 0 || k + X[b] <= kf) continue;
    const int tab = (int)unum.size();
    const std::pair<int, int>* mb = merged.data() + (size_t)b * SV_EX_MAX_E;
    uint32_t nr = 0, run = 0;
    uoff.resize((size_t)(tab + 1) * (SV_EX_RANGES + 1), 0u);
    ustart.resize((size_t)(tab + 1) * SV_EX_RANGES, 0u);
    uint32_t* uo = uoff.data() + (size_t)tab * (SV_EX_RANGES + 1);
    uint32_t* us = ustart.data() + (size_t)tab * SV_EX_RANGES;
    int next = 0;   // first image id not yet covered
    for (int e = 0; e <= nm[b]; ++e) {
      const int end = e < nm[b] ? mb[e].first : nimg;   // allowed ids next .. end - 1
      if (end > next && off[end] > off[next]) {
        us[nr] = off[next];
        uo[nr] = run;
        run += off[end] - off[next];
        ++nr;
      }
      if (e < nm[b]) next = mb[e].second + 1;
    }
    uo[nr] = run;
    unum.push_back(nr);
    const int ng = (rws + 63) / 64;
    for (int j = 0; j < ng; ++j) {
      const int a0 = qoff[b] + (int)((int64_t)rws * j / ng), a1 = qoff[b] + (int)((int64_t)rws * (j + 1) / ng);
      groups.insert(groups.end(), {a0, a1 - a0, tab, n_slots});
      for (int q = a0; q < a1; ++q) slot_q.push_back(q);
      n_slots += a1 - a0;
      gmax = std::max(gmax, a1 - a0);
    }
  }
  const bool tail = !groups.empty();
  if (tail && (int64_t)off[nimg] != ctx->db_n)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "search_excluding: the index holds rows with negative image ids, which the exact tail's "
                     "image -> row map does not cover (a window of %lld rows at k=%d needs the tail)", (long long)xmax, k);

  SV_HIP(ctx->s_deep_d2.reserve((size_t)nq * kf * 4));
  SV_HIP(ctx->s_deep_idx.reserve((size_t)nq * kf * 8));
  SV_TRY(sv_search_dev(ctx, Q, nq, kf, ctx->s_deep_d2.as<float>(), ctx->s_deep_idx.as<int64_t>()));

  // launch metadata in one copy: qoff [n_img + 1], then the images' records
  static_assert(sizeof(ExImg) % 4 == 0, "records follow the offsets as int32 words");
  const size_t img_w0 = ((size_t)n_img + 1 + 1) & ~(size_t)1;
  std::vector<int32_t> meta(img_w0 + (size_t)n_img * (sizeof(ExImg) / 4));
  std::copy(qoff, qoff + n_img + 1, meta.begin());
  ExImg* him = reinterpret_cast<ExImg*>(meta.data() + img_w0);
  for (int b = 0; b < n_img; ++b) {
    him[b].safe = k + X[b] <= kf;
    him[b].pad = 0;
    for (int e = 0; e < SV_EX_MAX_E; ++e) {
      him[b].lo[e] = e < nm[b] ? merged[(size_t)b * SV_EX_MAX_E + e].first : 1;
      him[b].hi[e] = e < nm[b] ? merged[(size_t)b * SV_EX_MAX_E + e].second : 0;
    }
  }
  const void* dmeta;
  SV_TRY(sv_in(ctx, meta.data(), meta.size() * 4, &dmeta));
  const int32_t* dqoff = (const int32_t*)dmeta;
  const ExImg* dimgs = reinterpret_cast<const ExImg*>(dqoff + img_w0);
  uint32_t *flags = nullptr, *n_short = nullptr;
  if (tail) {   // word 0: the short-row counter (segvlad_exclude_stats), words 4 ..: the rows' flags
    SV_HIP(ctx->s_ex_flag.reserve(((size_t)nq + 4) * 4));
    SV_HIP(ctx->s_deep_qn.reserve((size_t)nq * 4));
    SV_HIP(ctx->s_ex_td2.reserve((size_t)n_slots * k * 4));
    SV_HIP(ctx->s_ex_tidx.reserve((size_t)n_slots * k * 8));
    n_short = ctx->s_ex_flag.as<uint32_t>();
    flags = n_short + 4;
  }
  const float* Qt = Q;   // the tail's GEMM loads 16-byte pieces: a row-offset view of a device tensor is copied for it
  if (tail) SV_TRY(sv_aligned_queries(ctx, Q, nq, &Qt));
  {
    StageScope sc(ctx, "knn_exclude");
    if (tail) {
      SV_HIP(hipMemsetAsync(n_short, 0, 4, ctx->stream));
      // (from Q itself, not the copy: the norms of a view that is not 16-byte aligned are summed in another order, and the tail's
      //  rows must carry the values segvlad_search gives the same pointer)
      SV_TRY(sv_launch_row_sumsq(ctx, Q, nq, d, ctx->s_deep_qn.as<float>()));
      sc.count();
    }
    hipLaunchKernelGGL(ex_compact_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, ctx->s_deep_d2.as<float>(),
                       ctx->s_deep_idx.as<int64_t>(), nq, kf, k, dqoff, n_img, dimgs, ctx->db_img.as<int32_t>(), d2_out, idx_out, flags,
                       n_short);
    SV_HIP(hipGetLastError());
    sc.count();
    if (tail) {
      const void* dslot;
      SV_TRY(sv_in(ctx, slot_q.data(), (size_t)n_slots * 4, &dslot));
      SV_TRY(sv_launch_exclude_tail(ctx, Qt, ctx->s_deep_qn.as<float>(), groups.data(), (int)(groups.size() / 4), gmax, n_slots,
                                    unum.data(), uoff.data(), ustart.data(), (int)unum.size(), flags, k, ctx->s_ex_td2.as<float>(),
                                    ctx->s_ex_tidx.as<int64_t>()));
      hipLaunchKernelGGL(ex_scatter_kernel, dim3((unsigned)n_slots), dim3(64), 0, ctx->stream, (const int32_t*)dslot, flags, k,
                         ctx->s_ex_td2.as<float>(), ctx->s_ex_tidx.as<int64_t>(), d2_out, idx_out);
      SV_HIP(hipGetLastError());
      sc.count(3);
      ctx->ex_short_dev = n_short;
    }
  }
  return SEGVLAD_OK;
}

extern "C" int segvlad_search_excluding(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img,
                                        const int32_t* excl, int E, int k, float* d2_out, int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || n_img < 0 || k < 1 || k > 1024 || E < 1 || E > SV_EX_MAX_E)
    return ctx->fail(SEGVLAD_ERR_ARG, "search_excluding: need nq, n_img >= 0, 1<=k<=1024, 1<=E<=%d (k=%d, E=%d)", SV_EX_MAX_E, k, E);
  SV_TRY(sv_check_qseg_offsets(ctx, "search_excluding", qseg_offsets, n_img, nq));
  if (n_img > 0 && !excl) return ctx->fail(SEGVLAD_ERR_ARG, "search_excluding: null excl");
  if (excl && sv_is_device_ptr(excl)) return ctx->fail(SEGVLAD_ERR_ARG, "search_excluding: excl must be host memory");
  SV_TRY(sv_check_img_index(ctx, "search_excluding"));
  const int d = ctx->db_d;
  if (d % 32 != 0) return ctx->fail(SEGVLAD_ERR_LIMIT, "search_excluding: d=%d (the exact GEMM of the tail takes d %% 32 == 0)", d);
  if (ctx->db_n > 0x7fffffffll) return ctx->fail(SEGVLAD_ERR_LIMIT, "search_excluding: more than 2^31 - 1 rows");
  if (ctx->opt.debug_fail_search == 1) return ctx->fail(SEGVLAD_ERR_STATE, "search_excluding: failing on request (option debug_fail_search)");
  ctx->ex_stats[0] = ctx->ex_stats[1] = ctx->ex_stats[2] = ctx->ex_stats[3] = 0;
  ctx->ex_short_dev = nullptr;
  if (nq == 0) return SEGVLAD_OK;
  if (!Q || !d2_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "search_excluding: null pointer");
  const void* dq;
  void *dd2, *didx;
  SV_TRY(sv_in(ctx, Q, (size_t)nq * d * 4, &dq));
  SV_TRY(sv_out(ctx, d2_out, (size_t)nq * k * 4, &dd2));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k * 8, &didx));
  if (ctx->db_n == 0) {   // emptied by segvlad_db_remove: no row is allowed anywhere
    ctx->ex_stats[0] = k;
    SV_HIP(sv_fill_none(ctx, (float*)dd2, (int64_t*)didx, (size_t)nq * k));
    return sv_finish(ctx);
  }
  SV_TRY(search_excluding(ctx, (const float*)dq, nq, qseg_offsets, n_img, excl, E, k, (float*)dd2, (int64_t*)didx));
  return sv_finish(ctx);
}

extern "C" int segvlad_exclude_stats(segvlad_ctx* ctx, int64_t* stats_out, int n) {
  CHECK_CTX();
  if (!stats_out || n < 0) return ctx->fail(SEGVLAD_ERR_ARG, "exclude_stats: bad arguments");
  if (ctx->ex_short_dev) {   // the rows the last call's tail finished: fetched once
    uint32_t w = 0;
    SV_HIP(hipMemcpyAsync(&w, ctx->ex_short_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->ex_stats[2] = w;
    ctx->ex_short_dev = nullptr;
  } else {
    SV_HIP(hipStreamSynchronize(ctx->stream));
  }
  for (int i = 0; i < n && i < 4; ++i) stats_out[i] = ctx->ex_stats[i];
  return SEGVLAD_OK;
}
