// Kernels of segvlad_range_search (host side: search.hip): the thresholds of the one full-level filter pass, the exact
// evaluation and LDS ordering of whole candidate lists, the counts -> lims scan, the count / emit sweeps of the exact distance
// blocks (long rows and the exact path), the ordering of those rows' segments and the unpacking of the ordered words.
//
// Every distance is the chain of segvlad_search: the sequential fp32 fma dot product in k order (sv_dot_seq_, knn_dev.h: what
// refine_exact_kernel evaluates, and bit for bit what the fp32 distance GEMM's matrix pipe produces), the stored row norms,
// sv_d2.  A hit is `d2 < radius2`, strictly; its word is (f2key(d2) << 32 | id), so ascending words are ascending
// (d2, lower id) -- a total order, which makes every result independent of the order the words were collected in.
#include <algorithm>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "ctx.h"
#include "knn_dev.h"

extern "C" {

// radius2 -> eff[q] (what a distance is compared with: -inf for a NaN, zero or negative radius, so nothing is below it) and
// thr[q] (what the filter collects under: eff, but -inf for +inf -- such a row takes every finite distance, it is flagged
// long here and the filter appends nothing for it).
__global__ __launch_bounds__(256) void range_thr_kernel(const float* __restrict__ radius2, int nq, float* __restrict__ eff,
                                                        float* __restrict__ thr, uint32_t* __restrict__ flags, int all_long) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const float r = radius2[q];
  const float e = (r > 0.f) ? r : -INFINITY;   // (false for NaN)
  const bool inf = e == INFINITY;
  eff[q] = e;
  thr[q] = inf ? -INFINITY : e;
  flags[q] = (inf || all_long) ? 1u : 0u;
}

// One chunk's candidate-list lengths: a list longer than cap flags its row long; out = {words the short rows may stage (u64),
// sum of the lengths (u64), the longest list, long rows of the chunk}.  One workgroup.
__global__ __launch_bounds__(1024) void range_cand_stats_kernel(const uint32_t* __restrict__ cand_cnt, int m, int cap,
                                                                uint32_t* __restrict__ flags, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_bound, s_sum;
  __shared__ uint32_t s_max, s_long;
  if (threadIdx.x == 0) {
    s_bound = 0ull;
    s_sum = 0ull;
    s_max = 0u;
    s_long = 0u;
  }
  __syncthreads();
  unsigned long long bound = 0ull, sum = 0ull;
  uint32_t mx = 0u, nl = 0u;
  for (int r = threadIdx.x; r < m; r += 1024) {
    const uint32_t c = cand_cnt[r];
    uint32_t f = flags[r];
    if (!f && c > (uint32_t)cap) flags[r] = f = 1u;
    sum += c;
    mx = max(mx, c);
    nl += f;
    if (!f) bound += c;
  }
  atomicAdd(&s_bound, bound);
  atomicAdd(&s_sum, sum);
  atomicMax(&s_max, mx);
  atomicAdd(&s_long, nl);
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = s_bound;
    out[1] = s_sum;
    out[2] = s_max;
    out[3] = s_long;
  }
}

// A short row's candidate list, evaluated exactly and ordered: one workgroup per query row, one candidate per thread and
// sweep (its row walked with U 16-byte loads in flight, as refine_exact_kernel's), the words of the hits ordered in LDS
// (sv_bitonic over the smallest power of two that holds the list), then written to `stage` behind a reservation on *cursor:
// soff[row] = where, cnt[row] = how many.  Where a row's words sit in `stage` depends on the order the workgroups finish in;
// nothing that leaves the call does (the unpack reads them through soff).  Flagged (long) rows: cnt = 0, soff = -1.
// Dynamic LDS: [d] floats, then [np2 of the chunk's longest short list] words.
}  // extern "C"

template <int U>
__global__ __launch_bounds__(256) void range_refine_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                           const float* __restrict__ qn, const float* __restrict__ rn,
                                                           const float* __restrict__ eff, const uint32_t* __restrict__ cand_cnt,
                                                           const uint32_t* __restrict__ cand_id, int cap,
                                                           const uint32_t* __restrict__ flags, uint32_t* __restrict__ cnt,
                                                           int64_t* __restrict__ soff, unsigned long long* __restrict__ stage,
                                                           unsigned long long* __restrict__ cursor) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t s_hits;
  __shared__ unsigned long long s_off;
  float* qs = reinterpret_cast<float*>(smem);
  uint64_t* a = reinterpret_cast<uint64_t*>(smem + (size_t)d * 4);
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (flags[row]) {
    if (tid == 0) {
      cnt[row] = 0u;
      soff[row] = -1;
    }
    return;
  }
  const int n = (int)cand_cnt[row];   // <= cap: a longer list flagged its row
  const int np2 = sv_np2(n);
  for (int j = tid; j < (d >> 2); j += 256) reinterpret_cast<float4*>(qs)[j] = reinterpret_cast<const float4*>(Q + row * d)[j];
  for (int j = tid; j < np2; j += 256) a[j] = SV_WORD_NONE;
  if (tid == 0) s_hits = 0u;
  __syncthreads();
  const float q2 = qn[row], rad = eff[row];
  const float4* qp = reinterpret_cast<const float4*>(qs);
  for (int j = tid; j < n; j += 256) {
    const uint32_t id = cand_id[row * cap + j];
    const float acc = sv_dot_seq_<U>(qp, reinterpret_cast<const float4*>(R + (size_t)id * d), d >> 2);
    const float v = sv_d2(q2, rn[id], acc);
    if (v < rad) {
      a[j] = sv_word(v, id);
      atomicAdd(&s_hits, 1u);
    }
  }
  sv_bitonic(a, np2, tid);   // (the empty slots, all ones, sort behind every hit: a NaN is never a hit)
  const uint32_t hits = s_hits;
  if (tid == 0) {
    s_off = hits ? atomicAdd(cursor, (unsigned long long)hits) : 0ull;
    cnt[row] = hits;
    soff[row] = (int64_t)s_off;
  }
  __syncthreads();
  const unsigned long long off = s_off;
  for (uint32_t j = tid; j < hits; j += 256) stage[off + j] = a[j];
}

extern "C" {

// lims[0] = 0, lims[q + 1] = lims[q] + (flags == null || flags[q] ? cnt[q] : 0): one workgroup walks the counts in tiles of
// 1024, the running total carried from tile to tile.
__global__ __launch_bounds__(1024) void range_scan_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ flags, int nq,
                                                          int64_t* __restrict__ lims) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t carry;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    carry = 0;
    lims[0] = 0;
  }
  __syncthreads();
  for (int q0 = 0; q0 < nq; q0 += 1024) {
    const int q = q0 + tid;
    int64_t v = (q < nq && (!flags || flags[q])) ? (int64_t)cnt[q] : 0;
    for (int o = 1; o < 64; o <<= 1) {   // inclusive scan of the wave
      const int64_t u = __shfl_up(v, o);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int64_t base = carry;
    for (int j = 0; j < w; ++j) base += wsum[j];
    if (q < nq) lims[q + 1] = base + v;
    __syncthreads();
    if (tid == 1023) carry = base + v;
    __syncthreads();
  }
}

// the listed rows of (Q, qn, eff), dense: the query block of the exact distance sweeps.  eff == null: every row gets an infinite
// radius (the exact tail of segvlad_search_grouped)
__global__ __launch_bounds__(256) void range_gather_kernel(const float* __restrict__ Q, const float* __restrict__ qn,
                                                           const float* __restrict__ eff, const int32_t* __restrict__ rows, int d,
                                                           float* __restrict__ Y, float* __restrict__ yn, float* __restrict__ yeff) {
  const int r = blockIdx.x;
  const int64_t src = rows[r];
  for (int j = threadIdx.x; j < d; j += 256) Y[(int64_t)r * d + j] = Q[src * d + j];
  if (threadIdx.x == 0) {
    yn[r] = qn[src];
    yeff[r] = eff ? eff[src] : INFINITY;
  }
}

// One exact distance block dist [mq][ld] (query rows rows[0, mq) against index rows col0 .. col0 + ns - 1).
// words == null: cnt[rows[r]] += the entries below eff[r] (the slabs of a row run one after the other on the stream).
// words != null: those entries' words appended at words[woff[rows[r]] + cur[rows[r]]++] (wave-aggregated reservations).
__global__ __launch_bounds__(256) void range_block_kernel(const float* __restrict__ dist, int64_t ld, int ns, int64_t col0,
                                                          const float* __restrict__ eff, const int32_t* __restrict__ rows,
                                                          uint32_t* __restrict__ cnt, const int64_t* __restrict__ woff,
                                                          uint32_t* __restrict__ cur, unsigned long long* __restrict__ words) {
  __shared__ uint32_t s_cnt;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float rad = eff[r];
  const int64_t q = rows[r];
  const float* x = dist + (int64_t)r * ld;
  if (!words) {
    if (tid == 0) s_cnt = 0u;
    __syncthreads();
    uint32_t c = 0u;
    for (int j = tid; j < ns; j += 256) c += (x[j] < rad) ? 1u : 0u;
    c = wave_sum_u32_(c);
    if (lane == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0 && s_cnt) cnt[q] += s_cnt;
    return;
  }
  const int64_t base = woff[q];
  for (int j0 = 0; j0 < ns; j0 += 256) {
    const int j = j0 + tid;
    const float v = j < ns ? x[j] : 0.f;
    const bool hit = j < ns && v < rad;
    const uint64_t mask = __ballot(hit);
    if (!mask) continue;
    uint32_t slot0 = 0u;
    if (lane == 0) slot0 = atomicAdd(&cur[q], (uint32_t)__popcll(mask));
    slot0 = (uint32_t)__shfl((int)slot0, 0);
    if (hit) {
      const uint32_t pos = slot0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      words[base + pos] = sv_word_key(f2key_(v), (uint32_t)(col0 + j));
    }
  }
}

// the ordered words of the rows with flags[q] == want, from src[srcoff[q] ..), to (d2_out, idx_out)[lims[q] ..)
__global__ __launch_bounds__(256) void range_unpack_kernel(const unsigned long long* __restrict__ src, const int64_t* __restrict__ srcoff,
                                                           const uint32_t* __restrict__ flags, uint32_t want,
                                                           const int64_t* __restrict__ lims, float* __restrict__ d2_out,
                                                           int64_t* __restrict__ idx_out) {
  const int64_t q = blockIdx.x;
  if (flags[q] != want) return;
  const int64_t lo = lims[q], n = lims[q + 1] - lo, so = srcoff[q];
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    const unsigned long long w = src[so + j];
    d2_out[lo + j] = sv_word_d2(w);
    idx_out[lo + j] = sv_word_id(w);
  }
}

}  // extern "C"

// ---- launchers -----------------------------------------------------------------------------------------------------
int sv_launch_range_thr(segvlad_ctx* ctx, const float* radius2, int nq, float* eff, float* thr, uint32_t* flags, bool all_long) {
  hipLaunchKernelGGL(range_thr_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, radius2, nq, eff, thr, flags, all_long ? 1 : 0);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

int sv_launch_range_cand_stats(segvlad_ctx* ctx, const uint32_t* cand_cnt, int m, int cap, uint32_t* flags, uint64_t* out_dev) {
  hipLaunchKernelGGL(range_cand_stats_kernel, dim3(1), dim3(1024), 0, ctx->stream, cand_cnt, m, cap, flags,
                     reinterpret_cast<unsigned long long*>(out_dev));
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

int sv_launch_range_refine(segvlad_ctx* ctx, const float* Q, const float* R, int m, int d, const float* qn, const float* rn,
                           const float* eff, const uint32_t* cand_cnt, const uint32_t* cand_id, int cap, uint32_t list_max,
                           const uint32_t* flags, uint32_t* cnt, int64_t* soff, uint64_t* stage, uint64_t* cursor) {
  if (m <= 0) return SEGVLAD_OK;
  if (d % 64 != 0) return ctx->fail(SEGVLAD_ERR_STATE, "range refine: d=%d is not a multiple of 64", d);
  const size_t np2 = (size_t)sv_np2((int)std::min<size_t>(list_max, (size_t)cap));
  const size_t lds = (size_t)d * 4 + np2 * 8;
  if (lds > 160 * 1024 - 64) return ctx->fail(SEGVLAD_ERR_LIMIT, "range refine: a %zu-entry list of %d-d rows exceeds the LDS", np2, d);
  auto go = [&](auto kern) -> int {
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(m), dim3(256), lds, ctx->stream, Q, R, d, qn, rn, eff, cand_cnt, cand_id, cap, flags, cnt, soff,
                       reinterpret_cast<unsigned long long*>(stage), reinterpret_cast<unsigned long long*>(cursor));
    SV_HIP(hipGetLastError());
    return SEGVLAD_OK;
  };
  return (d % 128 == 0) ? go(range_refine_kernel<32>) : go(range_refine_kernel<16>);
}

int sv_launch_range_scan(segvlad_ctx* ctx, const uint32_t* cnt, const uint32_t* flags, int nq, int64_t* lims) {
  hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, flags, nq, lims);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

int sv_launch_range_gather(segvlad_ctx* ctx, const float* Q, const float* qn, const float* eff, const int32_t* rows, int nr, int d,
                           float* Y, float* yn, float* yeff) {
  if (nr <= 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(range_gather_kernel, dim3(nr), dim3(256), 0, ctx->stream, Q, qn, eff, rows, d, Y, yn, yeff);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

int sv_launch_range_block(segvlad_ctx* ctx, const float* dist, int64_t ld, int mq, int ns, int64_t col0, const float* eff,
                          const int32_t* rows, uint32_t* cnt, const int64_t* woff, uint32_t* cur, uint64_t* words) {
  if (mq <= 0 || ns <= 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(range_block_kernel, dim3(mq), dim3(256), 0, ctx->stream, dist, ld, ns, col0, eff, rows, cnt, woff, cur,
                     reinterpret_cast<unsigned long long*>(words));
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// Orders every segment [off[q], off[q + 1]) of `words` (n_words in all) ascending into `sorted` (rocPRIM's segmented radix sort
// over all 64 bits; its temporary storage is ctx->s_rs_tmp).
int sv_range_sort_segments(segvlad_ctx* ctx, const uint64_t* words, uint64_t* sorted, int64_t n_words, int nq, const int64_t* off) {
  if (n_words <= 0 || nq <= 0) return SEGVLAD_OK;
  if (n_words > 0xffffffffLL) return ctx->fail(SEGVLAD_ERR_LIMIT, "range search: %lld hits in rows beyond the filter's lists", (long long)n_words);
  size_t tmp = 0;
  SV_HIP(rocprim::segmented_radix_sort_keys(nullptr, tmp, words, sorted, (unsigned)n_words, (unsigned)nq, off, off + 1, 0u, 64u, ctx->stream));
  SV_HIP(ctx->s_rs_tmp.reserve(tmp ? tmp : 4));
  SV_HIP(rocprim::segmented_radix_sort_keys(ctx->s_rs_tmp.p, tmp, words, sorted, (unsigned)n_words, (unsigned)nq, off, off + 1, 0u, 64u,
                                            ctx->stream));
  return SEGVLAD_OK;
}

int sv_launch_range_unpack(segvlad_ctx* ctx, const uint64_t* src, const int64_t* srcoff, const uint32_t* flags, uint32_t want, int nq,
                           const int64_t* lims, float* d2_out, int64_t* idx_out) {
  if (nq <= 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(range_unpack_kernel, dim3(nq), dim3(256), 0, ctx->stream, reinterpret_cast<const unsigned long long*>(src), srcoff,
                     flags, want, lims, d2_out, idx_out);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
