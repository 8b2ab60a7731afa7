// Shortlist-restricted exact search (segvlad_search_shortlist).  No reference counterpart: the reference searches the whole
// index (place_rec_main.py:53-60); this is the re-ranking / location-prior form of deployed place recognition, where every
// query IMAGE comes with the reference images its segments may match (a global-descriptor top-M, a GNSS radius).
//
//   image -> row map   (built lazily on the first shortlist search after segvlad_db_add / segvlad_db_reset)
//     sl_hist_kernel      rows per reference image (atomics over db_img)
//     sl_scan_kernel      exclusive scan -> offsets [n_img_ref + 1], and a copy as scatter cursors
//     sl_scatter_kernel   row ids into their image's segment (atomic cursor: order not yet defined)
//     sl_sort_kernel      one workgroup per image: its segment sorted ascending in LDS (<= SL_SORT_CAP rows), or -- a larger image --
//                         rebuilt in row order by an ordered scan of db_img (ballot compaction); rows are thus ascending per image
//                         whether an image's rows are contiguous or not (several db_add calls, interleaved ids)
//   per call
//     sl_union_kernel     per query image: its shortlist sorted, duplicates / -1 padding / ids without rows dropped, and the
//                         prefix sums of the kept images' row counts: union position p -> (image j, row off[j] + p - uoff[j]).
//                         The union is never materialised (a shortlist may cover the whole index)
//     sl_gemm_kernel      1-D grid of (group, slice) workgroups: a group is <= 64 consecutive query rows of one image (the group
//                         bound of the tile, group_tile_dev.h), slice s takes the union's 128-row tiles s, s + S, s + 2S, ...  Per tile
//                         the exact fp32 distances of all group x 128 pairs -- the gathered-row tile of group_tile_dev.h: per pair the
//                         sequential chain acc = fma(q[k], r[k], acc) from 0 on v_mfma_f32_32x32x2_f32 in k order, then sv_d2 with
//                         the stored norms: bit for bit segvlad_search's value -- then every key (distance bits,
//                         row id) below the row's threshold is appended to the row's candidate buffer in global memory.  A buffer
//                         that could not take another tile is cut to its k best by a workgroup sort, which also sets the threshold
//                         (the k-th key); at the end every buffer is cut to <= k
//     sl_final_kernel     per query row: its S slices' lists, (distance, id) sort, top k; (+inf, -1) beyond the allowed rows
// Nothing is read back during a call: the grid sizes come from qseg_offsets, n_img, M and k (host), the union sizes stay on the device.
// sl_gemm_kernel and sl_final_kernel also are the exact tail of segvlad_search_excluding (exclude_kernels.hip), whose "union" is the
// complement of a few intervals of image ids: sv_launch_exclude_tail, at the end of this file, behind the entry point.  Both launch the
// pair through sl_launch_gemm.
#include <algorithm>

#include "ctx.h"
#include "group_tile_dev.h"
#include "knn_dev.h"

namespace {

constexpr int SL_GMAX = 64;        // query rows per group, at most
constexpr int SL_SORT_CAP = 4096;  // rows of an image sorted in LDS by the map build (larger images: ordered scan)
constexpr int SL_SLICES_MAX = 8;

// ---- image -> row map -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sl_imax_kernel(const int32_t* __restrict__ img, int64_t n, int* __restrict__ out) {
  int m = -1;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) m = max(m, img[r]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

__global__ __launch_bounds__(256) void sl_hist_kernel(const int32_t* __restrict__ img, int64_t n, int nimg, uint32_t* __restrict__ cnt) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int g = img[r];
  if (g >= 0 && g < nimg) atomicAdd(&cnt[g], 1u);
}

constexpr int SL_SCAN_T = 1024;
__global__ __launch_bounds__(SL_SCAN_T) void sl_scan_kernel(const uint32_t* __restrict__ cnt, int nimg, uint32_t* __restrict__ off,
                                                            uint32_t* __restrict__ cur) {
  __shared__ uint32_t part[SL_SCAN_T];
  const int tid = threadIdx.x;
  const int per = (nimg + SL_SCAN_T - 1) / SL_SCAN_T;
  const int b0 = min(nimg, tid * per), b1 = min(nimg, b0 + per);
  uint32_t s = 0;
  for (int i = b0; i < b1; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int t = 0; t < SL_SCAN_T; ++t) {
      const uint32_t v = part[t];
      part[t] = run;
      run += v;
    }
    off[nimg] = run;
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (int i = b0; i < b1; ++i) {
    off[i] = run;
    cur[i] = run;
    run += cnt[i];
  }
}

__global__ __launch_bounds__(256) void sl_scatter_kernel(const int32_t* __restrict__ img, int64_t n, int nimg, uint32_t* __restrict__ cur,
                                                         uint32_t* __restrict__ rows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int g = img[r];
  if (g >= 0 && g < nimg) rows[atomicAdd(&cur[g], 1u)] = (uint32_t)r;
}

__global__ __launch_bounds__(256) void sl_sort_kernel(const int32_t* __restrict__ img, int64_t n, const uint32_t* __restrict__ off,
                                                      uint32_t* __restrict__ rows) {
  __shared__ uint32_t a[SL_SORT_CAP];
  __shared__ uint32_t wtot[4];
  const int g = blockIdx.x, tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const uint32_t o = off[g];
  const int c = (int)(off[g + 1] - o);
  if (c <= 1) return;
  if (c <= SL_SORT_CAP) {
    const int np2 = sv_np2(c);
    for (int j = tid; j < np2; j += 256) a[j] = j < c ? rows[o + j] : 0xffffffffu;
    sv_bitonic<uint32_t>(a, np2, tid);
    for (int j = tid; j < c; j += 256) rows[o + j] = a[j];
    return;
  }
  // a large image: its rows in row order, by a scan of the whole map (at most n / SL_SORT_CAP such images)
  uint32_t base = 0;
  for (int64_t r0 = 0; r0 < n; r0 += 256) {
    const int64_t r = r0 + tid;
    const bool have = r < n && img[r] == g;
    const uint64_t mk = __builtin_amdgcn_ballot_w64(have);
    if (l == 0) wtot[w] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t before = base, all = 0;
    for (int x = 0; x < 4; ++x) {
      if (x < w) before += wtot[x];
      all += wtot[x];
    }
    if (have) rows[o + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u))] = (uint32_t)r;
    base += all;
    __syncthreads();
  }
}

// ---- per query image: the deduplicated shortlist and the prefix sums of its images' row counts ---------------------------
__global__ __launch_bounds__(256) void sl_union_kernel(const int32_t* __restrict__ shortlist, int M, int np2, int nimg_ref,
                                                       const uint32_t* __restrict__ off, uint32_t* __restrict__ uids,
                                                       uint32_t* __restrict__ uoff, uint32_t* __restrict__ unum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* a = reinterpret_cast<uint32_t*>(smem);   // [np2]
  __shared__ uint32_t pk[256], ps[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < np2; j += 256) {
    uint32_t v = 0xffffffffu;
    if (j < M) {
      const int id = shortlist[(size_t)b * M + j];
      if (id >= 0 && id < nimg_ref) v = (uint32_t)id;
    }
    a[j] = v;
  }
  sv_bitonic<uint32_t>(a, np2, tid);
  const int per = np2 / 256 > 0 ? np2 / 256 : 1;
  const int j0 = tid * per, j1 = min(np2, j0 + per);
  uint32_t nk = 0, rs = 0;
  for (int j = j0; j < j1; ++j) {
    const uint32_t v = a[j];
    if (v != 0xffffffffu && (j == 0 || a[j - 1] != v)) {
      ++nk;
      rs += off[v + 1] - off[v];
    }
  }
  pk[tid] = nk;
  ps[tid] = rs;
  __syncthreads();
  if (tid == 0) {
    uint32_t rk = 0, rr = 0;
    for (int t = 0; t < 256; ++t) {
      const uint32_t x = pk[t], y = ps[t];
      pk[t] = rk;
      ps[t] = rr;
      rk += x;
      rr += y;
    }
    unum[b] = rk;
    uoff[(size_t)b * (M + 1) + rk] = rr;
  }
  __syncthreads();
  nk = pk[tid];
  rs = ps[tid];
  for (int j = j0; j < j1; ++j) {
    const uint32_t v = a[j];
    if (v != 0xffffffffu && (j == 0 || a[j - 1] != v)) {
      uids[(size_t)b * M + nk] = v;
      uoff[(size_t)b * (M + 1) + nk] = rs;
      ++nk;
      rs += off[v + 1] - off[v];
    }
  }
}

// ---- group x union tiles: exact fp32 distances, candidates below the running threshold ----------------------------------
struct SlGroup {
  int q0, nrows, img, pad;   // (pad: the group's first list slot in the exclusion's tail, unused by the shortlist search)
};

// EX (the exact tail of segvlad_search_excluding, exclude_kernels.hip): the "union" of group image b is the complement of its merged
// exclusion intervals -- nu <= 9 contiguous ranges of sl_img_rows POSITIONS, uids[j] the first position of range j (not an image id)
// and uoff the prefix sums of the ranges' lengths; a group none of whose rows is marked in ex_flags writes empty lists and leaves;
// a group's lists go to cand / lens at its slot base (SlGroup::pad) instead of its query rows.  Everything else -- the tile
// (group_tile_dev.h), sv_d2, the candidate buffers -- is the one code for both.
template <int MT, bool EX>
__global__ __launch_bounds__(256) void sl_gemm_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                      const float* __restrict__ qn, const float* __restrict__ rn,
                                                      const SlGroup* __restrict__ groups, int S, int M,
                                                      const uint32_t* __restrict__ off, const uint32_t* __restrict__ rows,
                                                      const uint32_t* __restrict__ uids, const uint32_t* __restrict__ uoff,
                                                      const uint32_t* __restrict__ unum, int k, int cap,
                                                      uint64_t* __restrict__ cand, uint32_t* __restrict__ lens,
                                                      const uint32_t* __restrict__ ex_flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [max(staging image, compaction scratch)] [dk: 32 MT x 128 distance keys]
  const size_t stage_bytes = max(sv_group_tile_bytes(MT), (size_t)cap * 8);
  float* tile = reinterpret_cast<float*>(smem);
  uint64_t* scratch = reinterpret_cast<uint64_t*>(smem);
  uint32_t* dk = reinterpret_cast<uint32_t*>(smem + stage_bytes);
  __shared__ uint32_t ids[128];
  __shared__ uint64_t s_thr[32 * MT];
  __shared__ uint32_t s_cnt[32 * MT];
  const int g = (int)(blockIdx.x / (unsigned)S), s = (int)(blockIdx.x % (unsigned)S);
  const SlGroup gr = groups[g];
  const int q0 = gr.q0, nrows = gr.nrows, b = gr.img;
  const int q_end = q0 + nrows;
  const int o0 = EX ? gr.pad : q0;   // first list of the group in cand / lens
  if constexpr (EX) {
    if (!__syncthreads_or(threadIdx.x < nrows && ex_flags[q0 + threadIdx.x] != 0u)) {
      if ((int)threadIdx.x < nrows) lens[(size_t)(o0 + threadIdx.x) * S + s] = 0u;
      return;
    }
  }
  const int nu = (int)unum[b];
  const uint32_t* uo = uoff + (size_t)b * (M + 1);
  const uint32_t* ui = uids + (size_t)b * M;
  const int U = (int)uo[nu];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  if (tid < 32 * MT) {
    s_thr[tid] = SV_WORD_NONE;
    s_cnt[tid] = 0u;
  }
  __syncthreads();
  // the k best keys of row r's buffer stay, the threshold becomes the k-th (a sort of the whole buffer by the workgroup)
  auto compact = [&](int r, int keep) {
    uint64_t* buf = cand + ((size_t)(o0 + r) * S + s) * cap;
    const int n = (int)s_cnt[r];
    const int np2 = sv_np2(n);
    for (int j = tid; j < np2; j += 256) scratch[j] = j < n ? buf[j] : SV_WORD_NONE;
    sv_bitonic<uint64_t>(scratch, np2, tid);
    const int nn = min(n, keep);
    for (int j = tid; j < nn; j += 256) buf[j] = scratch[j];
    if (tid == 0) {
      s_cnt[r] = (uint32_t)nn;
      if (nn == k) s_thr[r] = scratch[k - 1];
    }
    __syncthreads();
  };
  const SvGroupTileQ<MT> qrows = sv_group_tile_query_rows<MT>(Q, d, q0, q_end);   // (the same for every tile)
  const int ntile = (U + 127) >> 7;
  for (int t = s; t < ntile; t += S) {
    const int c0 = t * 128;
    if (tid < 128) {
      uint32_t id = 0;
      const int p = c0 + tid;
      if (p < U) {
        int lo = 0, hi = nu - 1;   // the last j with uoff[j] <= p
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if ((int)uo[mid] <= p) lo = mid;
          else hi = mid - 1;
        }
        id = rows[(EX ? ui[lo] : off[ui[lo]]) + (uint32_t)(p - (int)uo[lo])];
      }
      ids[tid] = id;   // (columns beyond U: row 0, computed and never used)
    }
    __syncthreads();
    f32x16 acc[MT];
    sv_group_tile_dots<MT>(tile, ids, qrows, R, d, acc);   // (on return `tile` is free: compact() below sorts in it)
    {
      const int col = 32 * w + i;
      const float r2 = rn[ids[col]];
#pragma unroll
      for (int u = 0; u < MT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr2 = 32 * u + sv_frag_row(r, kk);
          if (q0 + lr2 < q_end) dk[lr2 * 128 + col] = f2key_(sv_d2(qn[q0 + lr2], r2, acc[u][r]));
        }
    }
    __syncthreads();
    // candidates: a wave per row, two columns per lane, appended in ballot order
    for (int r = w; r < nrows; r += 4) {
      uint64_t* buf = cand + ((size_t)(o0 + r) * S + s) * cap;
      const uint64_t thr = s_thr[r];
      uint32_t cnt = s_cnt[r];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = l + 64 * h;
        const uint64_t key = sv_word_key(dk[r * 128 + col], ids[col]);
        const bool pass = c0 + col < U && key < thr;
        const uint64_t mk = __builtin_amdgcn_ballot_w64(pass);
        if (pass) buf[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u))] = key;
        cnt += (uint32_t)__popcll(mk);
      }
      if (l == 0) s_cnt[r] = cnt;
    }
    __syncthreads();
    // a buffer that could not take the next tile is cut to its k best
    for (int r = 0; r < nrows; ++r)
      if ((int)s_cnt[r] > cap - 128) compact(r, k);
  }
  for (int r = 0; r < nrows; ++r)
    if ((int)s_cnt[r] > k) compact(r, k);
  if (tid < nrows) lens[(size_t)(o0 + tid) * S + s] = s_cnt[tid];
}

// ---- per query row: the slices' lists, (distance, id) order, top k -------------------------------------------------------
__global__ __launch_bounds__(256) void sl_final_kernel(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ lens, int S,
                                                       int cap, int k, int np2, float* __restrict__ d2_out, int64_t* __restrict__ idx_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* a = reinterpret_cast<uint64_t*>(smem);   // [np2 >= S k]
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  int total = 0;
  for (int s = 0; s < S; ++s) {
    const int n = (int)lens[q * S + s];
    const uint64_t* buf = cand + ((size_t)q * S + s) * cap;
    for (int j = tid; j < n; j += 256) a[total + j] = buf[j];
    total += n;
  }
  for (int j = total + tid; j < np2; j += 256) a[j] = SV_WORD_NONE;
  if (S > 1 || total > 1) sv_bitonic<uint64_t>(a, np2, tid);
  for (int j = tid; j < k; j += 256) {
    float dd = INFINITY;
    int64_t id = -1;
    if (j < total) {
      dd = sv_word_d2(a[j]);
      id = sv_word_id(a[j]);
      if (!(dd < INFINITY)) id = -1;   // (never listed: segvlad.h, "Non-finite rows"; sv_d2 has made a NaN +inf)
    }
    d2_out[q * k + j] = dd;
    idx_out[q * k + j] = id;
  }
}

}   // namespace

// largest image id of db_img[from, n) (synchronises; segvlad_db_add)
int sv_img_max(segvlad_ctx* ctx, const int32_t* img_dev, int64_t n, int* out) {
  *out = -1;
  if (n <= 0) return SEGVLAD_OK;
  SV_HIP(ctx->s_sl_misc.reserve(4));
  int* dm = ctx->s_sl_misc.as<int>();
  SV_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dm), -1, 1, ctx->stream));
  const int64_t nb = std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(sl_imax_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, img_dev, n, dm);
  SV_HIP(hipGetLastError());
  SV_HIP(hipMemcpyAsync(out, dm, 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  return SEGVLAD_OK;
}

// the image -> row map of the current index (rebuilt when db_add / db_reset cleared sl_map_valid)
static int sl_build_map(segvlad_ctx* ctx) {
  if (ctx->sl_map_valid) return SEGVLAD_OK;
  const int nimg = ctx->db_img_max + 1;
  const int64_t n = ctx->db_n;
  SV_HIP(ctx->sl_img_off.reserve((size_t)(nimg + 1) * 4));
  SV_HIP(ctx->sl_img_rows.reserve((size_t)(n > 0 ? n : 1) * 4));
  SV_HIP(ctx->s_sl_cur.reserve((size_t)(nimg + 1) * 4 * 2));
  uint32_t* cnt = ctx->s_sl_cur.as<uint32_t>();
  uint32_t* cur = cnt + nimg + 1;
  uint32_t* off = ctx->sl_img_off.as<uint32_t>();
  const int32_t* img = ctx->db_img.as<int32_t>();
  SV_HIP(hipMemsetAsync(cnt, 0, (size_t)(nimg + 1) * 4, ctx->stream));
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (nimg > 0 && n > 0) {
    hipLaunchKernelGGL(sl_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, img, n, nimg, cnt);
    SV_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(sl_scan_kernel, dim3(1), dim3(SL_SCAN_T), 0, ctx->stream, cnt, nimg, off, cur);
  SV_HIP(hipGetLastError());
  if (nimg > 0 && n > 0) {
    hipLaunchKernelGGL(sl_scatter_kernel, dim3(nb), dim3(256), 0, ctx->stream, img, n, nimg, cur, ctx->sl_img_rows.as<uint32_t>());
    SV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sl_sort_kernel, dim3((unsigned)nimg), dim3(256), 0, ctx->stream, img, n, off, ctx->sl_img_rows.as<uint32_t>());
    SV_HIP(hipGetLastError());
  }
  ctx->sl_map_valid = true;
  ctx->sl_off_host_valid = false;
  return SEGVLAD_OK;
}

// the map, and ctx->sl_off_host = the host copy of sl_img_off [n_img_ref + 1] (segvlad_search_excluding counts an interval's rows
// with it): copied when the map was rebuilt -- one synchronisation per index change, none per call
int sv_sl_map_host(segvlad_ctx* ctx) {
  SV_TRY(sl_build_map(ctx));
  if (ctx->sl_off_host_valid) return SEGVLAD_OK;
  ctx->sl_off_host.resize((size_t)ctx->db_img_max + 2);
  SV_HIP(hipMemcpyAsync(ctx->sl_off_host.data(), ctx->sl_img_off.p, ctx->sl_off_host.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  ctx->sl_off_host_valid = true;
  return SEGVLAD_OK;
}

// The exact GEMM and the final sort, for both searches: sl_gemm_kernel<., EX> over the groups [ng] (HOST; gmax = the longest), then
// sl_final_kernel over the n_lists candidate lists (the query rows; EX: the list slots).  uids / uoff [.][M], [.][M + 1] / unum are
// the device tables the kernel reads in its mode, flags the EX row flags (else null).  Two launches, nothing read back.
static int sl_launch_gemm(segvlad_ctx* ctx, bool ex, const float* Q, const float* qn, const SlGroup* groups, int ng, int gmax,
                          int n_lists, int M, const uint32_t* uids, const uint32_t* uoff, const uint32_t* unum, const uint32_t* flags,
                          int k, float* d2_out, int64_t* idx_out) {
  // slices per group: ~1536 workgroups (256 CUs x 2 resident x 3: the GEMM is latency-bound at one or two waves per SIMD),
  // the lists of a row bounded by 8 k keys (the final sort) and the candidate buffers by ~512 MB
  const int cap = k <= 256 ? 1024 : 2048;
  int S = std::max(1, std::min(SL_SLICES_MAX, (1536 + ng - 1) / std::max(ng, 1)));
  while (S > 1 && (S * k > 8192 || (size_t)n_lists * S * cap * 8 > ((size_t)512 << 20))) --S;
  const void* dgrp;
  SV_TRY(sv_in(ctx, groups, (size_t)ng * sizeof(SlGroup), &dgrp));
  SV_HIP(ctx->s_sl_cand.reserve((size_t)n_lists * S * cap * 8));
  SV_HIP(ctx->s_sl_lens.reserve((size_t)n_lists * S * 4));
  uint64_t* cand = ctx->s_sl_cand.as<uint64_t>();
  uint32_t* lens = ctx->s_sl_lens.as<uint32_t>();
  const int mt = gmax > 32 ? 2 : 1;
  const size_t glds = std::max(sv_group_tile_bytes(mt), (size_t)cap * 8) + (size_t)32 * mt * 128 * 4;
  auto gk = ex ? (mt == 2 ? sl_gemm_kernel<2, true> : sl_gemm_kernel<1, true>) : (mt == 2 ? sl_gemm_kernel<2, false> : sl_gemm_kernel<1, false>);
  SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(gk), glds));
  hipLaunchKernelGGL(gk, dim3((unsigned)(ng * S)), dim3(256), glds, ctx->stream, Q, ctx->db_rows.as<float>(), ctx->db_d, qn,
                     ctx->db_norms.as<float>(), (const SlGroup*)dgrp, S, M, ctx->sl_img_off.as<uint32_t>(),
                     ctx->sl_img_rows.as<uint32_t>(), uids, uoff, unum, k, cap, cand, lens, flags);
  SV_HIP(hipGetLastError());
  const int np2 = sv_np2(S * k);
  const size_t flds = (size_t)np2 * 8;
  if (flds > 48 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(sl_final_kernel), flds));
  hipLaunchKernelGGL(sl_final_kernel, dim3((unsigned)n_lists), dim3(256), flds, ctx->stream, cand, lens, S, cap, k, np2, d2_out, idx_out);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// segvlad_search_shortlist after the argument checks: Q on the device, 16-byte aligned, qn its squared norms; qoff host; shortlist /
// outputs on the device
static int search_shortlist(segvlad_ctx* ctx, const float* Q, int nq, const float* qn, const int32_t* qoff, int n_img,
                            const int32_t* shortlist, int M, int k, float* d2_out, int64_t* idx_out) {
  {
    StageScope sc(ctx, "knn_shortlist");
    const bool rebuilt = !ctx->sl_map_valid;
    SV_TRY(sl_build_map(ctx));
    // groups: an image's rows in ceil(rows / 64) near-equal runs
    std::vector<SlGroup> grp;
    int gmax = 0;
    for (int b = 0; b < n_img; ++b) {
      const int rws = qoff[b + 1] - qoff[b];
      if (rws <= 0) continue;
      const int ng = (rws + SL_GMAX - 1) / SL_GMAX;
      for (int j = 0; j < ng; ++j) {
        const int a0 = qoff[b] + (int)((int64_t)rws * j / ng), a1 = qoff[b] + (int)((int64_t)rws * (j + 1) / ng);
        grp.push_back({a0, a1 - a0, b, 0});
        gmax = std::max(gmax, a1 - a0);
      }
    }
    const int ng = (int)grp.size();
    int np2m = 64;
    while (np2m < M) np2m <<= 1;
    SV_HIP(ctx->s_sl_uids.reserve((size_t)n_img * M * 4));
    SV_HIP(ctx->s_sl_uoff.reserve((size_t)n_img * (M + 1) * 4));
    SV_HIP(ctx->s_sl_unum.reserve((size_t)n_img * 4));
    const size_t ulds = (size_t)np2m * 4;
    if (ulds > 48 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(sl_union_kernel), ulds));
    hipLaunchKernelGGL(sl_union_kernel, dim3((unsigned)n_img), dim3(256), ulds, ctx->stream, shortlist, M, np2m, ctx->db_img_max + 1,
                       ctx->sl_img_off.as<uint32_t>(), ctx->s_sl_uids.as<uint32_t>(), ctx->s_sl_uoff.as<uint32_t>(),
                       ctx->s_sl_unum.as<uint32_t>());
    SV_HIP(hipGetLastError());
    SV_TRY(sl_launch_gemm(ctx, false, Q, qn, grp.data(), ng, gmax, nq, M, ctx->s_sl_uids.as<uint32_t>(), ctx->s_sl_uoff.as<uint32_t>(),
                          ctx->s_sl_unum.as<uint32_t>(), nullptr, k, d2_out, idx_out));
    sc.count(rebuilt ? 8 : 3);
  }
  return SEGVLAD_OK;
}

extern "C" int segvlad_search_shortlist(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img,
                                        const int32_t* shortlist, int M, int k, float* d2_out, int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || n_img < 0 || k < 1 || k > 1024 || M < 1 || M > 4096)
    return ctx->fail(SEGVLAD_ERR_ARG, "search_shortlist: need nq, n_img >= 0, 1<=k<=1024, 1<=M<=4096 (k=%d, M=%d)", k, M);
  SV_TRY(sv_check_qseg_offsets(ctx, "search_shortlist", qseg_offsets, n_img, nq));
  SV_TRY(sv_check_img_index(ctx, "search_shortlist"));
  if (nq == 0) return SEGVLAD_OK;
  if (!Q || !shortlist || !d2_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "search_shortlist: null pointer");
  const int d = ctx->db_d;
  if (d % 32 != 0) return ctx->fail(SEGVLAD_ERR_LIMIT, "search_shortlist: d=%d (the exact GEMM takes d %% 32 == 0)", d);
  if (ctx->db_n > 0x7fffffffll) return ctx->fail(SEGVLAD_ERR_LIMIT, "search_shortlist: more than 2^31 - 1 rows");
  const void *dq, *dsl;
  const float* q;
  void *dd2, *didx;
  SV_TRY(sv_in(ctx, Q, (size_t)nq * d * 4, &dq));
  SV_TRY(sv_aligned_queries(ctx, (const float*)dq, nq, &q));
  SV_TRY(sv_in(ctx, shortlist, (size_t)n_img * M * 4, &dsl));
  SV_TRY(sv_out(ctx, d2_out, (size_t)nq * k * 4, &dd2));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k * 8, &didx));
  if (ctx->db_n == 0) {   // emptied by segvlad_db_remove: no row is allowed anywhere
    SV_HIP(sv_fill_none(ctx, (float*)dd2, (int64_t*)didx, (size_t)nq * k));
    return sv_finish(ctx);
  }
  SV_HIP(ctx->s_qnorm.reserve((size_t)nq * 4));
  SV_TRY(sv_launch_row_sumsq(ctx, q, nq, d, ctx->s_qnorm.as<float>()));
  SV_TRY(search_shortlist(ctx, q, nq, ctx->s_qnorm.as<float>(), qseg_offsets, n_img, (const int32_t*)dsl, M, k, (float*)dd2,
                          (int64_t*)didx));
  return sv_finish(ctx);
}

// The exact tail of segvlad_search_excluding: sl_gemm_kernel<., true> over the allowed rows of every group that holds a flagged
// query row, sl_final_kernel over the groups' n_slots list slots.  groups [ng] = {q0, nrows, table index, slot base} (HOST);
// unum [n_tab], uoff [n_tab][10], ustart [n_tab][9] (HOST): the allowed position ranges of sl_img_rows per table entry;
// flags [nq] device words; d2_tmp / idx_tmp [n_slots][k] device.  Two launches, nothing read back.
int sv_launch_exclude_tail(segvlad_ctx* ctx, const float* Q, const float* qn, const int32_t* groups, int ng, int gmax, int n_slots,
                           const uint32_t* unum, const uint32_t* uoff, const uint32_t* ustart, int n_tab, const uint32_t* flags,
                           int k, float* d2_tmp, int64_t* idx_tmp) {
  static_assert(sizeof(SlGroup) == 16, "groups are handed over as int32 quadruples");
  constexpr int M = SV_EX_RANGES;
  const void *dnum, *doff, *dst;
  SV_TRY(sv_in(ctx, unum, (size_t)n_tab * 4, &dnum));
  SV_TRY(sv_in(ctx, uoff, (size_t)n_tab * (M + 1) * 4, &doff));
  SV_TRY(sv_in(ctx, ustart, (size_t)n_tab * M * 4, &dst));
  return sl_launch_gemm(ctx, true, Q, qn, reinterpret_cast<const SlGroup*>(groups), ng, gmax, n_slots, M, (const uint32_t*)dst,
                        (const uint32_t*)doff, (const uint32_t*)dnum, flags, k, d2_tmp, idx_tmp);
}
