// Dense masks -> SAM's uncompressed RLE on the device (mask_to_rle_pytorch, sam/segment_anything/utils/amg.py:107-135; the areas are
// area_from_rle's): segvlad_rle_encode writes the batch layout that segvlad_incidence_rle and segvlad_rle_decode read
// (rle_kernels.hip) -- counts uint32, the runs of all masks one after the other, and run_offsets int64 [S + 1].
//
// A transpose plus a compaction: the bytes are row-major, the runs follow the columns (pixel p = col * Hm + row).  A CHANGE is a
// pixel whose value differs from the pixel before it, pixel 0 being compared with a clear pixel: a mask with n changes at
// p_0 < p_1 < ... has the n + 1 runs p_0, p_1 - p_0, ..., P - p_(n-1) (a mask without changes: [P]).  A set pixel 0 is a change at 0
// and so gives the leading run of length 0 without a special case.
//
// One UNIT is one (mask, column, block of RLE_ENCODE_ROWS rows); a mask's units are numbered column-major, u = col * nrb + block.
// The lanes of a wave take adjacent columns of one row block (four columns each, one 4-byte load per row, where Wm % 4 == 0 and the
// masks start on a 4-byte boundary; else one column each by byte loads), so a wave reads a contiguous piece of every row.  A lane
// shifts each byte's `!= 0` into its column's current 32-row word w, and t = (w ^ ((w << 1) | prev)) & valid marks the changes;
// prev, the bit of the pixel before, is carried down the column in a register and fetched as one byte at a block's first row
// (row 0 of column c > 0: mask[Hm - 1][c - 1]; pixel 0: clear).
//   pass 1   per unit: the number of changes, the position of its last change (or RLE_NONE), the number of set pixels;
//   scan     one workgroup per mask over its units in order: the exclusive sum of the changes (the unit's rank base) and the
//            running last change (the position before the unit's first change) replace the first two; the mask's run count
//            (changes + 1), its final run P - last change and its area; then one workgroup scans the run counts into run_offsets;
//   pass 2   reads the bytes again (no column words are kept between the passes: the masks are read twice and nothing of their size
//            is written) and stores counts[run_offsets[s] + rank] = p - previous change for every change; the lane of unit 0 stores
//            the mask's final run.  It reads the total from run_offsets[S] and leaves, every thread alike, when that exceeds the
//            capacity.
// No mask is held in LDS: no size bound but the 32-bit count (Hm Wm <= 2^32 - 1).  Every global store goes to an address that
// (mask, unit) or (mask) fixes, or to a rank below the capacity; nothing is added with atomics, so two calls write the same bytes.
#include <algorithm>

#include "ctx.h"

constexpr int RLE_ENCODE_ROWS = 256;   // rows per unit (rle.RLE_ENCODE_ROWS; tests/test_rle_encode_host.py compares the two)
constexpr int RLE_ENC_THREADS = 256;
constexpr uint32_t RLE_NONE = 0xffffffffu;   // "no change in this unit" (a position is < P <= 2^32 - 1)
static_assert(RLE_ENCODE_ROWS % 32 == 0, "a unit is whole 32-row words");
static_assert(RLE_ENC_THREADS == 256, "the scans below are written for four waves");

typedef unsigned long long u64;

// The work of one wave: 64 lanes x V adjacent columns of row block rb of mask s.  Items are numbered column group fastest, then row
// block, then mask.
struct RleEncGeom {
  int S, Hm, Wm, nrb, ncgb;   // row blocks per column; 64-lane column groups per row
  int64_t n_items;            // S * nrb * ncgb
};

// The change words of the V columns c0 .. c0 + V - 1, rows [r0, r1), of the mask at m: f(j, first row of the word, t, w & valid)
// for every 32-row word, top to bottom.
template <int V, class F>
__device__ __forceinline__ void rle_enc_walk(const uint8_t* __restrict__ m, uint32_t Hm, uint32_t Wm, uint32_t c0, uint32_t r0, uint32_t r1,
                                             F&& f) {
  uint32_t prev[V];
  if (r0 > 0) {
    const uint8_t* q = m + (size_t)(r0 - 1) * Wm + c0;
    if constexpr (V == 4) {
      const uint32_t x = *reinterpret_cast<const uint32_t*>(q);
#pragma unroll
      for (int j = 0; j < V; ++j) prev[j] = ((x >> (8 * j)) & 0xffu) != 0u;
    } else {
      prev[0] = q[0] != 0;
    }
  } else {
    const uint8_t* q = m + (size_t)(Hm - 1) * Wm;   // the last row: column c - 1 ends there
#pragma unroll
    for (int j = 0; j < V; ++j) prev[j] = (c0 + j > 0) ? (uint32_t)(q[c0 + j - 1] != 0) : 0u;
  }
  for (uint32_t r = r0; r < r1; r += 32) {
    const uint32_t n = min(32u, r1 - r);
    uint32_t w[V];
#pragma unroll
    for (int j = 0; j < V; ++j) w[j] = 0;
    const uint8_t* q = m + (size_t)r * Wm + c0;
    if (n == 32) {
#pragma unroll
      for (uint32_t i = 0; i < 32; ++i) {
        if constexpr (V == 4) {
          const uint32_t x = *reinterpret_cast<const uint32_t*>(q + (size_t)i * Wm);
#pragma unroll
          for (int j = 0; j < V; ++j) w[j] |= (uint32_t)(((x >> (8 * j)) & 0xffu) != 0u) << i;
        } else {
          w[0] |= (uint32_t)(q[(size_t)i * Wm] != 0) << i;
        }
      }
    } else {
      for (uint32_t i = 0; i < n; ++i) {
        if constexpr (V == 4) {
          const uint32_t x = *reinterpret_cast<const uint32_t*>(q + (size_t)i * Wm);
#pragma unroll
          for (int j = 0; j < V; ++j) w[j] |= (uint32_t)(((x >> (8 * j)) & 0xffu) != 0u) << i;
        } else {
          w[0] |= (uint32_t)(q[(size_t)i * Wm] != 0) << i;
        }
      }
    }
    const uint32_t valid = n == 32 ? 0xffffffffu : ((1u << n) - 1u);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const uint32_t t = (w[j] ^ ((w[j] << 1) | prev[j])) & valid;
      f(j, r, t, w[j] & valid);
      prev[j] = (w[j] >> (n - 1)) & 1u;
    }
  }
}

// item -> (mask, row block, first column of this lane); false: the lane has no column
template <int V>
__device__ __forceinline__ bool rle_enc_item(const RleEncGeom& g, int64_t item, int lane, int& s, int& rb, uint32_t& c0) {
  const int cgb = (int)(item % g.ncgb);
  const int64_t q = item / g.ncgb;
  rb = (int)(q % g.nrb);
  s = (int)(q / g.nrb);
  const int64_t c = ((int64_t)cgb * 64 + lane) * V;
  c0 = (uint32_t)c;
  return c < g.Wm;
}

// unit_n / unit_last / unit_area: [S][U], U = Wm * nrb
template <int V>
__global__ __launch_bounds__(RLE_ENC_THREADS) void rle_encode_count_kernel(const uint8_t* __restrict__ masks, RleEncGeom g,
                                                                          uint32_t* __restrict__ unit_n, uint32_t* __restrict__ unit_last,
                                                                          uint32_t* __restrict__ unit_area) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t P = (size_t)g.Hm * g.Wm, U = (size_t)g.Wm * g.nrb;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wv; item < g.n_items; item += (int64_t)gridDim.x * 4) {
    int s, rb;
    uint32_t c0;
    if (!rle_enc_item<V>(g, item, lane, s, rb, c0)) continue;
    const uint32_t r0 = (uint32_t)rb * RLE_ENCODE_ROWS, r1 = min((uint32_t)g.Hm, r0 + RLE_ENCODE_ROWS);
    uint32_t n[V], last[V], area[V];
#pragma unroll
    for (int j = 0; j < V; ++j) n[j] = 0, last[j] = RLE_NONE, area[j] = 0;
    rle_enc_walk<V>(masks + (size_t)s * P, (uint32_t)g.Hm, (uint32_t)g.Wm, c0, r0, r1, [&](int j, uint32_t r, uint32_t t, uint32_t w) {
      n[j] += __popc(t);
      area[j] += __popc(w);
      if (t) last[j] = (c0 + j) * (uint32_t)g.Hm + r + (31u - (uint32_t)__clz(t));
    });
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const size_t u = (size_t)s * U + (size_t)(c0 + j) * g.nrb + rb;
      unit_n[u] = n[j];
      unit_last[u] = last[j];
      unit_area[u] = area[j];
    }
  }
}

// One workgroup per mask (grid-stride).  In place: unit_n -> the unit's rank base, unit_last -> the position before its first change.
__global__ __launch_bounds__(RLE_ENC_THREADS) void rle_encode_scan_kernel(uint32_t* __restrict__ unit_n, uint32_t* __restrict__ unit_last,
                                                                         const uint32_t* __restrict__ unit_area, int S, int64_t U, uint32_t P,
                                                                         int64_t* __restrict__ n_runs, uint32_t* __restrict__ final_run,
                                                                         int64_t* __restrict__ area_out) {
  __shared__ uint32_t wsum[4], wmax[4];
  __shared__ u64 warea[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    uint32_t csum = 0, cmax = 0;   // changes so far; 1 + the last change so far (0: none -- RLE_NONE + 1 wraps to it)
    u64 a = 0;
    uint32_t* un = unit_n + (size_t)s * U;
    uint32_t* ul = unit_last + (size_t)s * U;
    const uint32_t* ua = unit_area + (size_t)s * U;
    for (int64_t b = 0; b < U; b += RLE_ENC_THREADS) {
      const int64_t u = b + tid;
      const uint32_t n = u < U ? un[u] : 0u, key = u < U ? ul[u] + 1u : 0u;
      if (u < U) a += ua[u];
      uint32_t isum = n, imax = key;
      for (int d = 1; d < 64; d <<= 1) {   // inclusive scans of the wave
        const uint32_t us = __shfl_up(isum, d), um = __shfl_up(imax, d);
        if (lane >= d) isum += us, imax = max(imax, um);
      }
      if (lane == 63) wsum[wv] = isum, wmax[wv] = imax;
      const uint32_t before = __shfl_up(imax, 1);
      __syncthreads();
      uint32_t psum = csum, pmax = cmax;
      for (int k = 0; k < wv; ++k) psum += wsum[k], pmax = max(pmax, wmax[k]);
      if (u < U) {
        un[u] = psum + (isum - n);
        const uint32_t k = max(pmax, lane > 0 ? before : 0u);
        ul[u] = k ? k - 1u : 0u;
      }
      csum += wsum[0] + wsum[1] + wsum[2] + wsum[3];
      cmax = max(max(cmax, wmax[0]), max(max(wmax[1], wmax[2]), wmax[3]));
      __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) warea[wv] = a;
    __syncthreads();
    if (tid == 0) {
      n_runs[s] = (int64_t)csum + 1;
      final_run[s] = P - (cmax ? cmax - 1u : 0u);
      if (area_out) area_out[s] = (int64_t)(warea[0] + warea[1] + warea[2] + warea[3]);
    }
    __syncthreads();
  }
}

// one workgroup: run_offsets[s] = n_runs[0] + ... + n_runs[s - 1], run_offsets[S] the total
__global__ __launch_bounds__(RLE_ENC_THREADS) void rle_encode_offsets_kernel(const int64_t* __restrict__ n_runs, int S, int64_t* __restrict__ run_offsets) {
  __shared__ int64_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t carry = 0;
  for (int b = 0; b < S; b += RLE_ENC_THREADS) {
    const int s = b + tid;
    const int64_t n = s < S ? n_runs[s] : 0;
    int64_t incl = n;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int64_t pre = carry;
    for (int k = 0; k < wv; ++k) pre += wsum[k];
    if (s < S) run_offsets[s] = pre + (incl - n);
    carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) run_offsets[S] = carry;
}

template <int V>
__global__ __launch_bounds__(RLE_ENC_THREADS) void rle_encode_emit_kernel(const uint8_t* __restrict__ masks, RleEncGeom g,
                                                                         const uint32_t* __restrict__ unit_base, const uint32_t* __restrict__ unit_prev,
                                                                         const uint32_t* __restrict__ final_run, const int64_t* __restrict__ run_offsets,
                                                                         int64_t capacity, uint32_t* __restrict__ counts) {
  if (run_offsets[g.S] > capacity) return;   // the same word for every thread: the batch does not fit, nothing is written
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t P = (size_t)g.Hm * g.Wm, U = (size_t)g.Wm * g.nrb;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wv; item < g.n_items; item += (int64_t)gridDim.x * 4) {
    int s, rb;
    uint32_t c0;
    if (!rle_enc_item<V>(g, item, lane, s, rb, c0)) continue;
    const uint32_t r0 = (uint32_t)rb * RLE_ENCODE_ROWS, r1 = min((uint32_t)g.Hm, r0 + RLE_ENCODE_ROWS);
    const int64_t off = run_offsets[s];
    int64_t at[V];
    uint32_t prevp[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const size_t u = (size_t)s * U + (size_t)(c0 + j) * g.nrb + rb;
      at[j] = off + (int64_t)unit_base[u];
      prevp[j] = unit_prev[u];
    }
    rle_enc_walk<V>(masks + (size_t)s * P, (uint32_t)g.Hm, (uint32_t)g.Wm, c0, r0, r1, [&](int j, uint32_t r, uint32_t t, uint32_t) {
      const uint32_t p0 = (c0 + j) * (uint32_t)g.Hm + r;
      while (t) {
        const uint32_t p = p0 + (uint32_t)(__ffs((int)t) - 1);
        t &= t - 1u;
        if (at[j] < capacity) counts[at[j]] = p - prevp[j];
        ++at[j];
        prevp[j] = p;
      }
    });
    if (c0 == 0 && rb == 0) {
      const int64_t fin = run_offsets[s + 1] - 1;
      if (fin >= 0 && fin < capacity) counts[fin] = final_run[s];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int segvlad_rle_encode(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int64_t* run_offsets_out, uint32_t* counts_out,
                                  int64_t capacity, int64_t* area_out, int64_t* n_runs_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("rle_encode");
  if (S < 0 || Hm <= 0 || Wm <= 0 || capacity < 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "rle_encode: bad arguments S=%d masks %dx%d capacity %lld", S, Hm, Wm, (long long)capacity);
  const u64 P = (u64)Hm * (u64)Wm;
  if (P > 0xffffffffull)   // (before any pointer is looked at)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "rle_encode: %dx%d masks have %llu pixels, a run is a 32-bit count (at most 2^32 - 1)", Hm, Wm, P);
  if (!run_offsets_out || (S > 0 && !masks) || (capacity > 0 && !counts_out)) return ctx->fail(SEGVLAD_ERR_ARG, "rle_encode: null pointer");
  const bool offs_dev = sv_is_device_ptr(run_offsets_out);
  if (S == 0) {
    if (offs_dev) SV_HIP(hipMemsetAsync(run_offsets_out, 0, sizeof(int64_t), ctx->stream));
    else run_offsets_out[0] = 0;
    if (n_runs_out) *n_runs_out = 0;
    return SEGVLAD_OK;
  }
  RleEncGeom g;
  g.S = S, g.Hm = Hm, g.Wm = Wm;
  g.nrb = (Hm + RLE_ENCODE_ROWS - 1) / RLE_ENCODE_ROWS;
  const size_t U = (size_t)Wm * g.nrb, SU = (size_t)S * U;
  const void* dm;
  SV_TRY(sv_in(ctx, masks, (size_t)S * P, &dm));
  void *doffs, *darea = nullptr;
  SV_TRY(sv_out(ctx, run_offsets_out, ((size_t)S + 1) * sizeof(int64_t), &doffs));
  if (area_out) SV_TRY(sv_out(ctx, area_out, (size_t)S * sizeof(int64_t), &darea));
  const bool counts_host = capacity > 0 && !sv_is_device_ptr(counts_out);
  uint32_t* dcounts = counts_out;
  if (counts_host) {   // staged by hand: the copy back depends on the total
    SV_HIP(ctx->s_re_counts.reserve((size_t)capacity * sizeof(uint32_t)));
    dcounts = ctx->s_re_counts.as<uint32_t>();
  }
  SV_HIP(ctx->s_re_unit.reserve(3 * SU * sizeof(uint32_t)));
  SV_HIP(ctx->s_re_mask.reserve((size_t)S * (sizeof(int64_t) + sizeof(uint32_t))));
  uint32_t *un = ctx->s_re_unit.as<uint32_t>(), *ul = un + SU, *ua = ul + SU;
  int64_t* nr = ctx->s_re_mask.as<int64_t>();
  uint32_t* fin = reinterpret_cast<uint32_t*>(nr + S);
  const bool vec4 = Wm % 4 == 0 && (reinterpret_cast<uintptr_t>(dm) & 3) == 0;
  g.ncgb = ((vec4 ? Wm / 4 : Wm) + 63) / 64;
  g.n_items = (int64_t)S * g.nrb * g.ncgb;
  const int grid = (int)std::min<int64_t>((g.n_items + 3) / 4, 256 * 64);
  {
    StageScope sc(ctx, "rle_encode");
    if (vec4) hipLaunchKernelGGL(rle_encode_count_kernel<4>, dim3(grid), dim3(RLE_ENC_THREADS), 0, ctx->stream, (const uint8_t*)dm, g, un, ul, ua);
    else hipLaunchKernelGGL(rle_encode_count_kernel<1>, dim3(grid), dim3(RLE_ENC_THREADS), 0, ctx->stream, (const uint8_t*)dm, g, un, ul, ua);
    SV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rle_encode_scan_kernel, dim3(std::min(S, 256 * 16)), dim3(RLE_ENC_THREADS), 0, ctx->stream, un, ul, ua, S, (int64_t)U, (uint32_t)P,
                       nr, fin, (int64_t*)darea);
    SV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rle_encode_offsets_kernel, dim3(1), dim3(RLE_ENC_THREADS), 0, ctx->stream, nr, S, (int64_t*)doffs);
    SV_HIP(hipGetLastError());
    sc.count(3);
    if (capacity > 0) {
      if (vec4)
        hipLaunchKernelGGL(rle_encode_emit_kernel<4>, dim3(grid), dim3(RLE_ENC_THREADS), 0, ctx->stream, (const uint8_t*)dm, g, un, ul, fin,
                           (const int64_t*)doffs, capacity, dcounts);
      else
        hipLaunchKernelGGL(rle_encode_emit_kernel<1>, dim3(grid), dim3(RLE_ENC_THREADS), 0, ctx->stream, (const uint8_t*)dm, g, un, ul, fin,
                           (const int64_t*)doffs, capacity, dcounts);
      SV_HIP(hipGetLastError());
      sc.count();
    }
  }
  // the total on the host: for n_runs_out, and to decide on the copy back of host counts (which a batch that does not fit must not touch)
  const bool want_total = n_runs_out || counts_host;
  int64_t total = 0;
  if (want_total && offs_dev) SV_HIP(hipMemcpyAsync(&total, (const int64_t*)doffs + S, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  const bool flushes = !ctx->pending_out.empty();
  SV_TRY(sv_finish(ctx));   // host run_offsets / areas: one synchronisation
  if (want_total) {
    if (!offs_dev) total = run_offsets_out[S];
    else if (!flushes) SV_HIP(hipStreamSynchronize(ctx->stream));
    if (n_runs_out) *n_runs_out = total;
    if (counts_host && total <= capacity) SV_HIP(hipMemcpy(counts_out, dcounts, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return SEGVLAD_OK;
}
