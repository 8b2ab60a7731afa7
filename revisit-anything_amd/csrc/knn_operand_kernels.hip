// Exact kNN, large-database path: operand preparation for the 16-bit filters and the scalars a search reads back (gfx950).
//
//   maxabs_kernel            max |x| of a block (optionally over the finite entries alone, with a non-finite flag)   sv_maxabs
//   max_kernel, min_kernel   largest / smallest of a list of row norms, by ordered keys                  sv_row_norm_max, sv_row_norm_min
//                            all three behind ONE read-back without a wait in between:            sv_maxabs_and_norm_min_begin / _end
//                            (the pinned words and the event of that read-back: sv_ensure_pinned_words)
//   to_f16_kernel            fp32 -> fp16 plane, scale from the host                                       sv_launch_to_f16
//   to_f16_devscale_kernel   the same, scale read from the device                                          sv_launch_to_f16_devscale
//   query_f16_small_kernel   a single image's query rows: scale, fp16 plane, norms and the zeroed flag block
//                            in one workgroup and one launch                                              sv_launch_query_f16_small
// (the filters that read these planes: knn_filter_kernels.hip, knn_bf16_filter_kernels.hip)
#include <string.h>

#include "ctx.h"
#include "knn_dev.h"

// max |x| of a block of floats.  16-byte loads where the pointer allows, ONE atomic per workgroup: the first version's 4-byte
// loads and one atomicMax per WAVE (16 384 of them on one word for a 10 000 x 1024 query batch) took 190 us in front of every
// batch search (round 5 kernel trace) for 41 MB -- 10 us of reading.
// FINITE_ONLY: NaN and Inf entries do not count (their |x| bit patterns sort above every finite value's): the maximum a
// power-of-two scale is derived from must not be taken over by one bad row (segvlad_pca_apply, the index and the queries of
// segvlad_search).  FLAG (with FINITE_ONLY): out[2] is raised when such an entry was seen.
template <bool FINITE_ONLY, bool FLAG = false>
__global__ __launch_bounds__(256) void maxabs_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t wmax[4];
  uint32_t m = 0, bad = 0;
  auto mag = [&bad](uint32_t u) -> uint32_t {
    u &= 0x7fffffffu;
    if (FLAG) bad |= (uint32_t)(u >= 0x7f800000u);
    return (FINITE_ONLY && u >= 0x7f800000u) ? 0u : u;
  };
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  int64_t head = 0;   // elements in front of the first 16-byte boundary
  if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) head = min<int64_t>(n, (int64_t)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) >> 2));
  const int64_t n4 = (n - head) >> 2;
  const uint4* x4 = reinterpret_cast<const uint4*>(x + head);
  for (int64_t j = tid; j < n4; j += nth) {
    const uint4 v = x4[j];
    m = max(max(m, mag(v.x)), max(max(mag(v.y), mag(v.z)), mag(v.w)));  // |x| bit pattern orders like the value
  }
  if (tid < head) m = max(m, mag(__float_as_uint(x[tid])));
  const int64_t tail0 = head + 4 * n4;
  if (tid < n - tail0) m = max(m, mag(__float_as_uint(x[tail0 + tid])));
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
  if (FLAG && __ballot(bad != 0u) != 0ull && (threadIdx.x & 63) == 0) atomicOr(out + 2, 1u);
}

// nonfinite_host != null (finite_only): set when the block holds a NaN or an Inf
int sv_maxabs(segvlad_ctx* ctx, const float* x, int64_t n, float* out_host, bool finite_only, bool* nonfinite_host) {
  SV_HIP(ctx->s_minmax.reserve(32));
  uint32_t* mm = ctx->s_minmax.as<uint32_t>() + 4;   // [4] = max |x| bits, [6] = the non-finite flag
  SV_HIP(hipMemsetAsync(mm, 0, 12, ctx->stream));
  int64_t blocks = (n + 1023) / 1024;
  if (blocks > 1024) blocks = 1024;
  if (n > 0 && finite_only && nonfinite_host)
    hipLaunchKernelGGL((maxabs_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, x, n, mm);
  else if (n > 0 && finite_only)
    hipLaunchKernelGGL(maxabs_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, x, n, mm);
  else if (n > 0)
    hipLaunchKernelGGL(maxabs_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, x, n, mm);
  uint32_t u[3] = {0, 0, 0};
  SV_HIP(hipMemcpyAsync(u, mm, 12, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  float f;
  memcpy(&f, &u[0], 4);
  *out_host = f;
  if (nonfinite_host) *nonfinite_host = u[2] != 0u;
  return SEGVLAD_OK;
}

__global__ __launch_bounds__(256) void to_f16_kernel(const float* __restrict__ X, int64_t n4, float scale,
                                                     _Float16* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(X)[j];
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 h;
    h[0] = (_Float16)(v.x * scale);  // round-to-nearest-even conversion
    h[1] = (_Float16)(v.y * scale);
    h[2] = (_Float16)(v.z * scale);
    h[3] = (_Float16)(v.w * scale);
    reinterpret_cast<h4*>(out)[j] = h;
  }
}

// A handful of query rows (<= 128 x d floats): largest magnitude, the power-of-two scale that puts it in [8192, 16384) --
// the host's pow2_scale, bit for bit -- and the fp16 plane, in ONE workgroup and one launch; the scales stay on the device
// (scales[0] = query scale, scales[1] = 1 / (query scale x db_scale)): no memset, no atomics, no host round trip.
// qn_out != null: the rows' squared norms as well (one wave per row, 16 rows in flight: the arithmetic of row_sumsq_kernel,
// gemm_kernels.hip, operation for operation -- lane j sums the squares of float4 j, j + 64, ... with fmaf, then the xor
// butterfly -- so that the single-image pass sees the very bits the batch path computes), instead of a launch of its own in
// front of this one.
__global__ __launch_bounds__(1024) void query_f16_small_kernel(const float* __restrict__ X, int64_t n4, float db_scale,
                                                               _Float16* __restrict__ out, float* __restrict__ scales,
                                                               float* __restrict__ qn_out, int nq, int d,
                                                               uint32_t* __restrict__ zero, int zero_words) {
  __shared__ uint32_t wmax[16];
  __shared__ uint32_t badrow[128];   // (nq <= 128)
  __shared__ float s_scale;
  const int tid = threadIdx.x;
  // the search's flag block, zeroed here instead of by a fill launch of its own in front of the pass's dependent chain
  for (int j = tid; j < zero_words; j += 1024) zero[j] = 0u;
  if (qn_out) {
    const int lane = tid & 63;
    for (int row = tid >> 6; row < nq; row += 16) {
      const float4* x4 = reinterpret_cast<const float4*>(X + (int64_t)row * d);
      float s = 0.f;
      for (int j = lane; j < (d >> 2); j += 64) {
        const float4 v = x4[j];
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) qn_out[row] = s;
    }
  }
  uint32_t m = 0;
  for (int64_t j = tid; j < n4; j += 1024) {
    const float4 v = reinterpret_cast<const float4*>(X)[j];
    m = max(m, mag4_(v));
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  for (int w = 0; w < 16; ++w) m = max(m, wmax[w]);
  if (m >= SV_BIG_BITS) {   // (uniform) a NaN, an Inf or a huge value: the maximum again, over the rows with a finite norm (knn_dev.h)
    const int d4 = d >> 2;
    for (int row = tid >> 6; row < nq; row += 16) {
      const bool bad = row_norm_bad_(X + (int64_t)row * d, d4, tid & 63);
      if ((tid & 63) == 0) badrow[row] = bad ? 1u : 0u;
    }
    __syncthreads();
    m = 0;
    for (int64_t j = tid; j < n4; j += 1024)
      if (!badrow[j / d4]) m = max(m, mag4_(reinterpret_cast<const float4*>(X)[j]));
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
  }
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) m = max(m, wmax[w]);
    const float maxabs = __uint_as_float(m);
    float scale = 1.f;
    if (maxabs > 0.f && isfinite(maxabs)) {
      int e;
      frexpf(maxabs, &e);
      scale = ldexpf(1.f, 14 - e);
    }
    s_scale = scale;
    scales[0] = scale;
    scales[1] = 1.f / (scale * db_scale);
  }
  __syncthreads();
  const float scale = s_scale;
  for (int64_t j = tid; j < n4; j += 1024) {
    const float4 v = reinterpret_cast<const float4*>(X)[j];
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 h;
    h[0] = (_Float16)(v.x * scale);
    h[1] = (_Float16)(v.y * scale);
    h[2] = (_Float16)(v.z * scale);
    h[3] = (_Float16)(v.w * scale);
    reinterpret_cast<h4*>(out)[j] = h;
  }
}

int sv_launch_query_f16_small(segvlad_ctx* ctx, const float* X, int64_t n_elems, float db_scale, uint16_t* out, float* scales_dev,
                              float* qn_out, int nq, int d, uint32_t* zero, int zero_words) {
  hipLaunchKernelGGL(query_f16_small_kernel, dim3(1), dim3(1024), 0, ctx->stream, X, n_elems / 4, db_scale,
                     reinterpret_cast<_Float16*>(out), scales_dev, qn_out, nq, d, zero, zero_words);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

__global__ __launch_bounds__(256) void to_f16_devscale_kernel(const float* __restrict__ X, int64_t n4, const float* __restrict__ scales,
                                                              _Float16* __restrict__ out) {
  const float scale = scales[0];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(X)[j];
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 h;
    h[0] = (_Float16)(v.x * scale);
    h[1] = (_Float16)(v.y * scale);
    h[2] = (_Float16)(v.z * scale);
    h[3] = (_Float16)(v.w * scale);
    reinterpret_cast<h4*>(out)[j] = h;
  }
}

int sv_launch_to_f16_devscale(segvlad_ctx* ctx, const float* X, int64_t n_elems, const float* scales_dev, uint16_t* out) {
  if (n_elems <= 0) return SEGVLAD_OK;
  const int64_t n4 = n_elems / 4;
  int64_t blocks = (n4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(to_f16_devscale_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, X, n4, scales_dev,
                     reinterpret_cast<_Float16*>(out));
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

int sv_launch_to_f16(segvlad_ctx* ctx, const float* X, int64_t n_elems, float scale, uint16_t* out) {
  if (n_elems <= 0) return SEGVLAD_OK;
  const int64_t n4 = n_elems / 4;
  int64_t blocks = (n4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(to_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, X, n4, scale,
                     reinterpret_cast<_Float16*>(out));
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ---- max of the database row norms (margin scale) -------------------------------------------------------------
// Both reductions order the values by their keys, where a NaN sorts above +inf or -- sign bit set -- below 0.0.  For the search
// (FINITE_ONLY; min_kernel always) NaN and Inf norms -- rows that are never listed -- do not count, or one such row would take the
// margin's scale from every other row; segvlad_set_vocab keeps the plain maximum.
__device__ __forceinline__ bool norm_counts_(float v) { return (__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u; }
template <bool FINITE_ONLY>
__global__ __launch_bounds__(256) void max_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ out) {
  uint32_t m = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const float v = x[j];
    if (!FINITE_ONLY || norm_counts_(v)) m = max(m, f2key_(v));
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

__global__ __launch_bounds__(256) void min_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ out) {
  uint32_t m = 0xffffffffu;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const float v = x[j];
    if (norm_counts_(v)) m = min(m, f2key_(v));
  }
  for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) atomicMin(out, m);
}

// smallest of n non-negative values (the query batch's smallest squared norm), read back to the host (synchronises)
int sv_row_norm_min(segvlad_ctx* ctx, const float* norms, int64_t n, float* out_host) {
  SV_HIP(ctx->s_minmax.reserve(32));
  uint32_t* mm = ctx->s_minmax.as<uint32_t>() + 6;
  SV_HIP(hipMemsetAsync(mm, 0xff, 4, ctx->stream));
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (n > 0) hipLaunchKernelGGL(min_kernel, dim3(blocks), dim3(256), 0, ctx->stream, norms, n, mm);
  uint32_t key = 0;
  SV_HIP(hipMemcpyAsync(&key, mm, 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  float f;
  memcpy(&f, &u, 4);
  *out_host = (n > 0 && key != 0xffffffffu) ? f : 0.f;
  return SEGVLAD_OK;
}

int sv_ensure_pinned_words(segvlad_ctx* ctx) {
  if (!ctx->h_pin) {
    SV_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pin), 64, hipHostMallocDefault));
    for (int j = 0; j < 16; ++j) ctx->h_pin[j] = 0u;
    SV_HIP(hipEventCreateWithFlags(&ctx->ev_scalars, hipEventDisableTiming));
  }
  return SEGVLAD_OK;
}

// max |x| of a block (finite values), the smallest and the largest finite of a list of row norms and the block's non-finite flag
// behind ONE read-back, WITHOUT a wait in between: _begin enqueues the reductions and the copy into pinned words of the
// context and records an event behind them; _end blocks on that event only.  What the caller enqueues between the two runs on
// the device while the host waits.
int sv_maxabs_and_norm_min_begin(segvlad_ctx* ctx, const float* x, int64_t n, const float* norms, int64_t n_norms) {
  SV_HIP(ctx->s_minmax.reserve(32));
  SV_TRY(sv_ensure_pinned_words(ctx));
  uint32_t* mm = ctx->s_minmax.as<uint32_t>() + 4;   // [4] = finite max |x| bits (init 0), [5] = min key (init all ones), [6] = non-finite flag
  static const uint32_t init[4] = {0u, 0xffffffffu, 0u, 0u};   // ..., [7] = max finite norm key
  SV_HIP(hipMemcpyAsync(mm, init, 16, hipMemcpyHostToDevice, ctx->stream));
  int64_t blocks = (n + 1023) / 1024;
  if (blocks > 1024) blocks = 1024;
  if (n > 0) hipLaunchKernelGGL((maxabs_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, x, n, mm);
  int nb = (int)((n_norms + 255) / 256);
  if (nb > 1024) nb = 1024;
  if (n_norms > 0) hipLaunchKernelGGL(min_kernel, dim3(nb), dim3(256), 0, ctx->stream, norms, n_norms, mm + 1);
  if (n_norms > 0) hipLaunchKernelGGL(max_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, norms, n_norms, mm + 3);
  SV_HIP(hipGetLastError());
  SV_HIP(hipMemcpyAsync(ctx->h_pin, mm, 16, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipEventRecord(ctx->ev_scalars, ctx->stream));
  return SEGVLAD_OK;
}

static float key_to_float(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int sv_maxabs_and_norm_min_end(segvlad_ctx* ctx, int64_t n, int64_t n_norms, float* maxabs_host, float* norm_min_host, bool* nonfinite_host,
                               float* norm_max_host) {
  SV_HIP(hipEventSynchronize(ctx->ev_scalars));
  const uint32_t h0 = ctx->h_pin[0], h1 = ctx->h_pin[1];
  memcpy(maxabs_host, &h0, 4);
  if (n <= 0) *maxabs_host = 0.f;
  *nonfinite_host = n > 0 && ctx->h_pin[2] != 0u;
  *norm_max_host = (n_norms > 0 && ctx->h_pin[3] != 0u) ? key_to_float(ctx->h_pin[3]) : 0.f;
  const uint32_t u = (h1 & 0x80000000u) ? (h1 & 0x7fffffffu) : ~h1;
  float f;
  memcpy(&f, &u, 4);
  *norm_min_host = (n_norms > 0 && h1 != 0xffffffffu) ? f : 0.f;
  return SEGVLAD_OK;
}

int sv_row_norm_max(segvlad_ctx* ctx, const float* norms, int64_t n, float* out_host, bool finite_only) {
  SV_HIP(ctx->s_minmax.reserve(16));
  uint32_t* mm = ctx->s_minmax.as<uint32_t>() + 2;
  SV_HIP(hipMemsetAsync(mm, 0, 4, ctx->stream));
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (n > 0 && finite_only) hipLaunchKernelGGL(max_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, norms, n, mm);
  else if (n > 0) hipLaunchKernelGGL(max_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, norms, n, mm);
  uint32_t key = 0;
  SV_HIP(hipMemcpyAsync(&key, mm, 4, hipMemcpyDeviceToHost, ctx->stream));
  SV_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  float f;
  memcpy(&f, &u, 4);
  *out_host = (n > 0 && key != 0) ? f : 0.f;
  return SEGVLAD_OK;
}
