// Device helpers shared by the search's translation units: the (distance, id) word and its order-preserving float <-> key map
// (key_word.h, their only definition), the workgroup bitonic sort of keys or words and the top-k write-out behind it, the exact
// fp32 chain in its two shapes (a row in global memory, a row of an LDS tile), DPP wave reductions, the flagging of a row; the
// counted waits of the filter's DMA loops come with it (waitcnt_dev.h).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "key_word.h"
#include "waitcnt_dev.h"

// a row redone on another path: marked once in its flag word, counted once
__device__ __forceinline__ void sv_flag_once_(uint32_t* rows, uint32_t* count, int64_t row) {
  if (atomicExch(&rows[row], 1u) == 0u) atomicAdd(count, 1u);
}

// Single-image query preparations: the power-of-two scale of the fp16 plane comes from max |x| over the rows whose squared norm is
// finite -- the rows that can be listed, the set the filters' margins are taken over ("Non-finite rows").  A norm can
// only fail to be finite when some |x| >= 2^55 (d <= 2^18): below that bit pattern of the plain maximum nothing needs a second look.
constexpr uint32_t SV_BIG_BITS = 0x5B000000u;   // 2^55
// wave-uniform: is the squared norm of the row (d4 float4s, 16-byte aligned) NOT finite?
__device__ __forceinline__ bool row_norm_bad_(const float* __restrict__ row, int d4, int lane) {
  const float4* x4 = reinterpret_cast<const float4*>(row);
  float s = 0.f;
  for (int j = lane; j < d4; j += 64) {
    const float4 v = x4[j];
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return !(fabsf(s) < INFINITY);
}
__device__ __forceinline__ uint32_t mag4_(const float4& v) {
  return max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu),
             max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu));
}

// ascending bitonic sort of n (a power of two) words in LDS by a workgroup of NTH threads
template <class T, int NTH = 256>
__device__ __forceinline__ void sv_bitonic(T* a, int n, int tid) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (n >> 1); t += NTH) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const T x = a[lo], y = a[hi];
        if ((y < x) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
    }
  }
  __syncthreads();
}

// The write-out of every exact path: the k result slots of row `row` from the ascending words a[0 .. len) -- the entries, then
// (+inf, -1).  UNTIL_NONE = false: the first len words are real; true: real until the first empty word.  k > len is fine in both.
// (The row index, not the row's pointers: with d2_out + row * k formed by the caller hipcc moves the address arithmetic of the
//  refinement kernels to the scalar unit and their instruction text changes.)
template <bool UNTIL_NONE>
__device__ __forceinline__ void sv_write_topk(const uint64_t* a, int len, int k, float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                              int64_t row, int tid) {
  for (int j = tid; j < k; j += 256) {
    float dd = INFINITY;
    int64_t id = -1;
    if (j < len && (!UNTIL_NONE || a[j] != SV_WORD_NONE)) {
      dd = sv_word_d2(a[j]);
      id = sv_word_id(a[j]);
    }
    d2_out[row * k + j] = dd;
    idx_out[row * k + j] = id;
  }
}

// The exact chain of every distance the search reports: the sequential fp32 fma dot product over k = 0 .. 4 n4 - 1 (bit for bit the
// chain of v_mfma_f32_32x32x2_f32 on the matrix path), with U 16-byte loads of the index row in flight per lane (n4 % U == 0); the
// query row sits in LDS or in global memory.  U = 32 is refine_exact_kernel's walk: 512 B of the row in flight per lane, 8 round
// trips for a 1024-d row -- a 50-query pass has fewer waves than the chip has SIMDs, so the loop is pure load latency (an 8-deep
// register double buffer still paid one round trip per 128 B: 78 us per pass).
template <int U>
__device__ __forceinline__ float sv_dot_seq_(const float4* qp, const float4* __restrict__ rp, int n4) {
  float acc = 0.f;
  for (int t = 0; t < n4; t += U) {
    float4 buf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) buf[u] = rp[t + u];
    // all U loads are issued before the first fma (the scheduler otherwise sinks them next to their uses to save registers -- and
    // pays the latency U times); U = 1 holds nothing back: the compiler unrolls that loop itself
    if constexpr (U > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float4 qv = qp[t + u];
      acc = fmaf(qv.x, buf[u].x, acc);
      acc = fmaf(qv.y, buf[u].y, acc);
      acc = fmaf(qv.z, buf[u].z, acc);
      acc = fmaf(qv.w, buf[u].w, acc);
    }
  }
  return acc;
}

// The same chain for one lane walking ONE ROW of an LDS tile (tr_: the row, n4_ float4s) against query floats in LDS (qb_: broadcast
// reads), UNROLL float4s per trip; acc carries the chain from step to step.  A statement macro: as a force-inlined function template
// refine_exact_wide_kernel<128, 4> comes out with other registers and 254 -> 256 VGPRs (the named rings around it leave no slack).
#define SV_PRAGMA_(x) _Pragma(#x)
#define SV_LDS_ROW_WALK(tr_, qb_, n4_, UNROLL, acc)                      \
  {                                                                      \
    const float* tr = (tr_);                                             \
    const float* qb = (qb_);                                             \
    SV_PRAGMA_(unroll UNROLL) for (int s4 = 0; s4 < (n4_); ++s4) {       \
      const float4 rv = *reinterpret_cast<const float4*>(tr + s4 * 4);   \
      const float4 qv = *reinterpret_cast<const float4*>(qb + s4 * 4);   \
      acc = fmaf(qv.x, rv.x, acc);                                       \
      acc = fmaf(qv.y, rv.y, acc);                                       \
      acc = fmaf(qv.z, rv.z, acc);                                       \
      acc = fmaf(qv.w, rv.w, acc);                                       \
    }                                                                    \
  }

// sum over the 64 lanes, returned wave-uniform: quad swaps, half-row and row mirrors (DPP: no LDS crossbar), then the four
// row sums through readlane
__device__ __forceinline__ uint32_t wave_sum_u32_(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
  x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
  x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false);   // row_half_mirror
  x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);   // row_mirror
  return (uint32_t)(__builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
                    __builtin_amdgcn_readlane(x, 48));
}

__device__ __forceinline__ uint32_t wave_min_u32_(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));
  return min(min((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
             min((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}
__device__ __forceinline__ uint32_t wave_max_u32_(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));
  return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
             max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}

