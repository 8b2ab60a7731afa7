// Removal from the index (segvlad_db_remove): a stream compaction of the index's planes, out of place, on the device.
//
//   rm_mark_rows_kernel   listed row ids -> a per-row byte (duplicates harmless, ids outside 0 .. n-1 ignored)
//   rm_mark_imgs_kernel   listed image ids -> a per-image byte of db_img_max + 1 entries (negative / larger ids ignored)
//   rm_count_kernel       per block of RM_ROWS rows: the row's final removal byte (row byte | its image's byte), and the block's
//                         number of kept rows from ballot popcounts
//   rm_scan_kernel        one workgroup: exclusive scan of the block totals (64-bit), n' behind them (the sl_scan_kernel pattern)
//   rm_pos_kernel         per block again: each kept row's new position -> src_of_dst[pos] = row, new_id[row] = pos or -1
//   rm_prefix_kernel      survivors below the old fp16 / bf16-plane row counts (binary searches of the ascending src_of_dst)
//   rm_gather_kernel      dst row j <- src row src_of_dst[j], for every plane: fp32 rows, norms, image ids, the fp16 image and the
//                         bf16 hi / lo planes (their existing prefixes).  16-byte accesses when the row pitch allows it, 8- or 4-byte
//                         ones otherwise (db_add takes any d: d % 4 == 2 and odd d); all offsets 64-bit (a raw K*D descriptor index
//                         passes 2^31 elements)
// Survivors keep their order, so dst row j's source is ascending in j: the gather streams both buffers.
#include <algorithm>

#include "ctx.h"

namespace {

constexpr int RM_T = 256;
constexpr int RM_ROWS = 4 * RM_T;   // rows per block of the count / position kernels

__global__ __launch_bounds__(RM_T) void rm_mark_rows_kernel(const int64_t* __restrict__ ids, int64_t n_ids, int64_t n,
                                                            uint8_t* __restrict__ row_rm) {
  for (int64_t i = (int64_t)blockIdx.x * RM_T + threadIdx.x; i < n_ids; i += (int64_t)gridDim.x * RM_T) {
    const int64_t r = ids[i];
    if (r >= 0 && r < n) row_rm[r] = 1;
  }
}

__global__ __launch_bounds__(RM_T) void rm_mark_imgs_kernel(const int32_t* __restrict__ ids, int64_t n_ids, int img_max,
                                                            uint8_t* __restrict__ img_rm) {
  for (int64_t i = (int64_t)blockIdx.x * RM_T + threadIdx.x; i < n_ids; i += (int64_t)gridDim.x * RM_T) {
    const int g = ids[i];
    if (g >= 0 && g <= img_max) img_rm[g] = 1;
  }
}

__global__ __launch_bounds__(RM_T) void rm_count_kernel(uint8_t* __restrict__ row_rm, const uint8_t* __restrict__ img_rm,
                                                        const int32_t* __restrict__ img, int img_max, int64_t n,
                                                        uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t wcnt[RM_T / 64];
  const int tid = threadIdx.x, w = tid >> 6;
  uint32_t kept = 0;
  for (int it = 0; it < RM_ROWS / RM_T; ++it) {
    const int64_t r = (int64_t)blockIdx.x * RM_ROWS + it * RM_T + tid;
    bool keep = false;
    if (r < n) {
      bool rm = row_rm[r] != 0;
      if (img_rm && !rm) {
        const int g = img[r];
        rm = g >= 0 && g <= img_max && img_rm[g] != 0;
        if (rm) row_rm[r] = 1;
      }
      keep = !rm;
    }
    kept += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(keep));
  }
  if ((tid & 63) == 0) wcnt[w] = kept;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
    for (int x = 0; x < RM_T / 64; ++x) s += wcnt[x];
    blk_cnt[blockIdx.x] = s;
  }
}

constexpr int RM_SCAN_T = 1024;
__global__ __launch_bounds__(RM_SCAN_T) void rm_scan_kernel(const uint32_t* __restrict__ cnt, int64_t nb, int64_t* __restrict__ off,
                                                            int64_t* __restrict__ total) {
  __shared__ int64_t part[RM_SCAN_T];
  const int tid = threadIdx.x;
  const int64_t per = (nb + RM_SCAN_T - 1) / RM_SCAN_T;
  const int64_t b0 = min(nb, (int64_t)tid * per), b1 = min(nb, b0 + per);
  int64_t s = 0;
  for (int64_t i = b0; i < b1; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < RM_SCAN_T; ++t) {
      const int64_t v = part[t];
      part[t] = run;
      run += v;
    }
    off[nb] = run;
    total[0] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int64_t i = b0; i < b1; ++i) {
    off[i] = run;
    run += cnt[i];
  }
}

__global__ __launch_bounds__(RM_T) void rm_pos_kernel(const uint8_t* __restrict__ row_rm, int64_t n, const int64_t* __restrict__ off,
                                                      int64_t* __restrict__ src_of_dst, int64_t* __restrict__ new_id) {
  __shared__ uint32_t wtot[RM_T / 64];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  int64_t base = off[blockIdx.x];
  for (int it = 0; it < RM_ROWS / RM_T; ++it) {
    const int64_t r = (int64_t)blockIdx.x * RM_ROWS + it * RM_T + tid;
    const bool keep = r < n && row_rm[r] == 0;
    const uint64_t mk = __builtin_amdgcn_ballot_w64(keep);
    if (l == 0) wtot[w] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int x = 0; x < RM_T / 64; ++x) {
      if (x < w) before += wtot[x];
      all += wtot[x];
    }
    if (r < n) {
      const int64_t pos = base + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      if (keep) src_of_dst[pos] = r;
      if (new_id) new_id[r] = keep ? pos : -1;
    }
    base += all;
    __syncthreads();
  }
}

// out[j] = survivors below bound[j] (= the first position whose source row is >= bound[j]), j < 2; total = n'
__global__ void rm_prefix_kernel(const int64_t* __restrict__ src_of_dst, const int64_t* __restrict__ total, int64_t b0, int64_t b1,
                                 int64_t* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= 2) return;
  const int64_t bound = j == 0 ? b0 : b1;
  int64_t lo = 0, hi = total[0];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (src_of_dst[mid] < bound) lo = mid + 1;
    else hi = mid;
  }
  out[j] = lo;
}

// dst row j <- src row src_of_dst[j]; a row is `units` elements of V.  WAVE: one wave per row (4 units per lane in flight), else
// one thread per unit over the flat [n_dst][units] range (short rows: the norms, the image ids, d = 96)
template <class V, bool WAVE>
__global__ __launch_bounds__(RM_T) void rm_gather_kernel(const V* __restrict__ src, V* __restrict__ dst, int64_t units,
                                                         const int64_t* __restrict__ src_of_dst, int64_t n_dst) {
  if (WAVE) {
    const int l = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (RM_T / 64);
    for (int64_t j = (int64_t)blockIdx.x * (RM_T / 64) + (threadIdx.x >> 6); j < n_dst; j += waves) {
      const V* s = src + src_of_dst[j] * units;
      V* o = dst + j * units;
      for (int64_t u = l; u < units; u += 4 * 64) {
        V v[4];
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (u + x * 64 < units) v[x] = s[u + x * 64];
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (u + x * 64 < units) o[u + x * 64] = v[x];
      }
    }
  } else {
    const int64_t tot = n_dst * units;
    for (int64_t t = (int64_t)blockIdx.x * RM_T + threadIdx.x; t < tot; t += (int64_t)gridDim.x * RM_T) {
      const int64_t j = t / units, u = t - j * units;
      dst[t] = src[src_of_dst[j] * units + u];
    }
  }
}

template <class V>
int launch_gather_as(segvlad_ctx* ctx, const void* src, void* dst, int64_t units, const int64_t* src_of_dst, int64_t n_dst) {
  if (units >= 64) {
    const int64_t nb = std::min<int64_t>((n_dst + RM_T / 64 - 1) / (RM_T / 64), 8192);
    hipLaunchKernelGGL((rm_gather_kernel<V, true>), dim3((unsigned)nb), dim3(RM_T), 0, ctx->stream, (const V*)src, (V*)dst, units,
                       src_of_dst, n_dst);
  } else {
    const int64_t nb = std::min<int64_t>((n_dst * units + RM_T - 1) / RM_T, 8192);
    hipLaunchKernelGGL((rm_gather_kernel<V, false>), dim3((unsigned)nb), dim3(RM_T), 0, ctx->stream, (const V*)src, (V*)dst, units,
                       src_of_dst, n_dst);
  }
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

}  // namespace

int sv_remove_positions(segvlad_ctx* ctx, const int64_t* row_ids, int64_t n_row_ids, const int32_t* img_ids, int64_t n_img_ids,
                        int64_t* new_id, int64_t plane_rows_a, int64_t plane_rows_b, int64_t* counts_host, int* launches) {
  *launches = 0;
  const int64_t n = ctx->db_n;
  const int64_t nb = (n + RM_ROWS - 1) / RM_ROWS;
  const bool by_img = n_img_ids > 0 && ctx->db_img_max >= 0;
  const int64_t nimg = by_img ? (int64_t)ctx->db_img_max + 1 : 0;
  SV_HIP(ctx->s_rm_row.reserve((size_t)n));
  if (by_img) SV_HIP(ctx->s_rm_img.reserve((size_t)nimg));
  SV_HIP(ctx->s_rm_blk.reserve((size_t)nb * 4 + (size_t)(nb + 1) * 8 + 8));
  SV_HIP(ctx->s_rm_src.reserve((size_t)n * 8));
  SV_HIP(ctx->s_rm_misc.reserve(4 * 8));
  uint8_t* row_rm = ctx->s_rm_row.as<uint8_t>();
  uint8_t* img_rm = by_img ? ctx->s_rm_img.as<uint8_t>() : nullptr;
  int64_t* off = reinterpret_cast<int64_t*>(ctx->s_rm_blk.as<char>() + (((size_t)nb * 4 + 7) & ~(size_t)7));
  uint32_t* blk_cnt = ctx->s_rm_blk.as<uint32_t>();
  int64_t* misc = ctx->s_rm_misc.as<int64_t>();
  SV_HIP(hipMemsetAsync(row_rm, 0, (size_t)n, ctx->stream));
  if (by_img) SV_HIP(hipMemsetAsync(img_rm, 0, (size_t)nimg, ctx->stream));
  if (n_row_ids > 0) {
    const int64_t g = std::min<int64_t>((n_row_ids + RM_T - 1) / RM_T, 4096);
    hipLaunchKernelGGL(rm_mark_rows_kernel, dim3((unsigned)g), dim3(RM_T), 0, ctx->stream, row_ids, n_row_ids, n, row_rm);
    SV_HIP(hipGetLastError());
    ++*launches;
  }
  if (by_img) {
    const int64_t g = std::min<int64_t>((n_img_ids + RM_T - 1) / RM_T, 4096);
    hipLaunchKernelGGL(rm_mark_imgs_kernel, dim3((unsigned)g), dim3(RM_T), 0, ctx->stream, img_ids, n_img_ids, ctx->db_img_max, img_rm);
    SV_HIP(hipGetLastError());
    ++*launches;
  }
  hipLaunchKernelGGL(rm_count_kernel, dim3((unsigned)nb), dim3(RM_T), 0, ctx->stream, row_rm, img_rm, ctx->db_img.as<int32_t>(),
                     ctx->db_img_max, n, blk_cnt);
  SV_HIP(hipGetLastError());
  hipLaunchKernelGGL(rm_scan_kernel, dim3(1), dim3(RM_SCAN_T), 0, ctx->stream, blk_cnt, nb, off, misc);
  SV_HIP(hipGetLastError());
  hipLaunchKernelGGL(rm_pos_kernel, dim3((unsigned)nb), dim3(RM_T), 0, ctx->stream, row_rm, n, off, ctx->s_rm_src.as<int64_t>(), new_id);
  SV_HIP(hipGetLastError());
  hipLaunchKernelGGL(rm_prefix_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->s_rm_src.as<int64_t>(), misc, plane_rows_a, plane_rows_b,
                     misc + 1);
  SV_HIP(hipGetLastError());
  *launches += 4;   // count, scan, positions, prefix
  // n' and the planes' surviving prefixes: the host plans every later search from them
  SV_HIP(hipMemcpyAsync(counts_host, misc, 3 * 8, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  return SEGVLAD_OK;
}

int sv_launch_remove_gather(segvlad_ctx* ctx, const void* src, void* dst, size_t pitch, int64_t n_dst) {
  if (n_dst <= 0 || pitch == 0) return SEGVLAD_OK;
  const int64_t* s = ctx->s_rm_src.as<int64_t>();
  if (pitch % 16 == 0) return launch_gather_as<uint4>(ctx, src, dst, (int64_t)(pitch / 16), s, n_dst);
  if (pitch % 8 == 0) return launch_gather_as<uint2>(ctx, src, dst, (int64_t)(pitch / 8), s, n_dst);
  // (every plane's pitch is a multiple of 4: fp32 rows, 4-byte norms / ids, 16-bit planes of d % 32 == 0)
  if (pitch % 4 == 0) return launch_gather_as<uint32_t>(ctx, src, dst, (int64_t)(pitch / 4), s, n_dst);
  return ctx->fail(SEGVLAD_ERR_ARG, "db_remove: row pitch of %zu bytes", pitch);
}
