// What the selects of the search share (knn_select_kernels.hip, select_kernels.hip):
//   * the row rule of the candidate-list selects (SvSelectArgs, ctx.h): entry test, flagging, band and carry limit, closing a band;
//   * the binary MSB-first radix select over keys in registers, by a wave or by a workgroup;
//   * the 8-bit radix select over keys in LDS or memory, with its wave-aggregated histogram.
#pragma once
#include "ctx.h"
#include "knn_dev.h"

// ---- the row rule: helpers for the row's leader lane or thread -----------------------------------------------------------
// The threshold the list was collected under, where the rule looks at it (read before thr_out -- possibly the same word -- is
// overwritten).
__device__ __forceinline__ float sel_thr_in_(const SvSelectArgs& a, int64_t row) {
  return ((a.check && a.mode == SvSelect::Band) || a.mode == SvSelect::Carry) ? a.thr_in[row * a.thr_in_ld] : 0.f;
}

// Entry test: the list overflowed (its own capacity, or the max_keys the calling form can rank), the row was flagged at a
// coarser level, or -- guessed thresholds -- the list is shorter than the rank.
__device__ __forceinline__ bool sel_rejects_(const SvSelectArgs& a, uint32_t c, uint32_t max_keys, uint32_t flagged) {
  return c > (uint32_t)a.cap || c > max_keys || flagged || (a.check && (int)c < a.k);
}

// The row is redone later (rigorous thresholds / exact matrix path): a threshold of -inf keeps its candidate list empty at the
// finer levels, an empty refine list makes the refinement a no-op.
__device__ __forceinline__ void sel_flag_row_(const SvSelectArgs& a, int64_t row) {
  sv_flag_once_(a.ovf_rows, a.ovf_count, row);
  if (a.mode == SvSelect::Band) a.ref_cnt[row] = 0;
  else a.thr_out[row] = -INFINITY;
}

// Guessed thresholds: the list holds every row with d2~ <= t_in + 2 eps; the refine set {d2~ <= A + 2 eps} is contained in it
// iff A <= t_in.
__device__ __forceinline__ bool sel_check_fails_(const SvSelectArgs& a, float ak, float t_in) { return a.check && !(ak <= t_in); }

// t + 2 eps(q): the band's limit (t = A), the carried survivors' limit (t = sel_carry_thr_)
__device__ __forceinline__ float sel_limit_(const SvSelectArgs& a, int64_t row, float t) {
  return t + 2.f * a.c_eps * sqrtf(a.qn[row] * a.rn_max);
}

// Carry: the next level runs over the rows this level has NOT seen (the complement of its sample), under the threshold
// t2 = min(A, t_in).  The list holds every sampled row with d2~ <= t_in + 2 eps, hence every one with d2~ <= t2 + 2 eps -- exactly
// the rows the next level's filter would append for the sample: they are compacted to the front and the counter is left at their
// number.  (A threshold below A is as good a guess as A: the last level's check is against the value stored.)
__device__ __forceinline__ float sel_carry_thr_(float ak, float t_in) { return fminf(ak, t_in); }

// Closing a band of `total` rows under flim.  More than the first-tier refine list holds: second tier (refine2_compact_kernel + a
// refinement pass straight from the candidate list), or -- without one -- the exact redo.
__device__ __forceinline__ void sel_close_band_(const SvSelectArgs& a, int64_t row, uint32_t total, float flim) {
  if (total > (uint32_t)a.rcap) {
    if (a.rovf_rows) {
      a.rovf_rows[row] = 1u;
      a.ref_lim[row] = flim;
      atomicAdd(a.rovf_count, 1u);
    } else {
      sv_flag_once_(a.ovf_rows, a.ovf_count, row);
    }
    a.ref_cnt[row] = 0;
  } else {
    a.ref_cnt[row] = total;
  }
}

// ---- binary radix select ---------------------------------------------------------------------------------------------------
// How a per-lane value becomes the total over the keys' holders.  A wave: DPP row reductions + four readlanes.  (The butterfly of
// six ds_bpermute shuffles it replaces was ~8 us of LDS-crossbar latency per launch; a ballot + scalar popcount per slot stalls
// on the VALU -> SALU hand-over of every compare: 42 us for 64 slots.)
struct SvWaveReduce {
  __device__ __forceinline__ uint32_t sum(uint32_t v) { return wave_sum_u32_(v); }
  __device__ __forceinline__ uint32_t min(uint32_t v) { return wave_min_u32_(v); }
  __device__ __forceinline__ uint32_t max(uint32_t v) { return wave_max_u32_(v); }
};
// A workgroup of four waves: the wave's value, then a four-entry LDS exchange (xs: [2][4] words; one barrier per reduction: the
// slots alternate).  Every thread of the workgroup takes part in every reduction.
struct SvWgReduce {
  uint32_t (*xs)[4];
  int tid, turn = 0;
  __device__ __forceinline__ uint4 exchange(uint32_t v_wave) {
    if ((tid & 63) == 0) xs[turn][tid >> 6] = v_wave;
    __syncthreads();
    const uint4 r = make_uint4(xs[turn][0], xs[turn][1], xs[turn][2], xs[turn][3]);
    turn ^= 1;
    return r;
  }
  __device__ __forceinline__ uint32_t sum(uint32_t v) {
    const uint4 r = exchange(wave_sum_u32_(v));
    return r.x + r.y + r.z + r.w;
  }
  __device__ __forceinline__ uint32_t min(uint32_t v) {
    const uint4 r = exchange(wave_min_u32_(v));
    return ::min(::min(r.x, r.y), ::min(r.z, r.w));
  }
  __device__ __forceinline__ uint32_t max(uint32_t v) {
    const uint4 r = exchange(wave_max_u32_(v));
    return ::max(::max(r.x, r.y), ::max(r.z, r.w));
  }
};

constexpr uint32_t SV_KEY_PAD = 0xffffffffu;   // padding sorts last (a real key is never all ones: NaN-free)

// k-th smallest of the keys a wave or workgroup holds in registers (PER per lane, padding = SV_KEY_PAD, c >= 1 real keys among
// them); +inf if c < k.  Uniform over the holders.  The slot loops are fully unrolled: a run-time bound on them cost a scalar
// branch per slot and bit -- 40 us per launch.
// The keys of a list share their leading bits (distances of one query: same sign, a handful of exponents), and after a dozen more
// only one key still matches the prefix: the bit loop starts below the common prefix of the list's smallest and largest key and
// stops as soon as a single candidate is left (32 bits x 2 PER VALU instructions were 7 of the ~10 us of a 4096-key launch).
template <int PER, class Reduce>
__device__ __forceinline__ float sv_kth_smallest_(const uint32_t (&key)[PER], uint32_t c, int k, Reduce& red) {
  if ((int)c < k) return INFINITY;
  uint32_t kmn = SV_KEY_PAD, kmx = 0u;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    kmn = min(kmn, key[i]);
    kmx = key[i] != SV_KEY_PAD ? max(kmx, key[i]) : kmx;
  }
  kmn = red.min(kmn);
  kmx = red.max(kmx);
  const uint32_t diff = kmn ^ kmx;
  uint32_t prefix = kmn, mask = 0xffffffffu, rem = (uint32_t)k, m = c;   // diff == 0: every key is kmn
  int bit = -1;
  if (diff) {
    bit = 31 - __builtin_clz(diff);
    mask = (bit == 31) ? 0u : ~((2u << bit) - 1u);
    prefix = kmn & mask;
  }
  for (; bit >= 0 && m > 1u; --bit) {
    const uint32_t b = 1u << bit;
    // keys that match the prefix so far and have this bit clear: counted per lane (a compare + an add per key slot), then ONE
    // reduction per bit
    uint32_t zl = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) zl += ((key[i] & (mask | b)) == prefix) ? 1u : 0u;
    const uint32_t zeros = red.sum(zl);
    if (rem > zeros) {
      rem -= zeros;
      m -= zeros;
      prefix |= b;
    } else {
      m = zeros;
    }
    mask |= b;
  }
  if (bit >= 0) {   // one key left under the prefix: it is the answer, whatever its remaining bits
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) v |= (key[i] != SV_KEY_PAD && (key[i] & mask) == prefix) ? key[i] : 0u;
    prefix = red.max(v);
  }
  return key2f_(prefix);
}

// ---- 8-bit radix select ----------------------------------------------------------------------------------------------------
// wave-aggregated LDS histogram increment: lanes that share a bin elect one leader per round (keys cluster on few digits: a
// plain atomicAdd would serialise)
__device__ __forceinline__ void hist_add(uint32_t* hist, bool active, uint32_t bin) {
  uint64_t todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lb = __shfl(bin, leader);
    const uint64_t same = __ballot(active && bin == lb) & todo;
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// prefix: the k-th smallest key; krem: how many of the keys equal to it are among the k smallest; ceq: how many exist
struct SvRadix8 {
  uint32_t prefix, krem, ceq;
};

// MSB-first, four passes of 256 bins, by a workgroup of 256 threads over the n >= k >= 1 keys key_at(0 .. n - 1).  Workgroup-uniform.
template <class Index, class KeyAt>
__device__ __forceinline__ SvRadix8 sv_radix8_select_(Index n, uint32_t k, KeyAt key_at, int tid) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_digit, s_krem, s_ceq;
  SvRadix8 r{0u, k, 0u};
  uint32_t mask = 0;
  for (int pass = 3; pass >= 0; --pass) {
    hist[tid] = 0;
    __syncthreads();
    const int shift = 8 * pass;
    for (Index j0 = 0; j0 < n; j0 += 256) {
      const Index j = j0 + tid;
      const uint32_t key = (j < n) ? key_at(j) : 0u;
      hist_add(hist, (j < n) && ((key & mask) == r.prefix), (key >> shift) & 255u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0, dsel = 255;
      for (uint32_t b = 0; b < 256; ++b) {
        const uint32_t h = hist[b];
        if (cum + h >= r.krem) {
          dsel = b;
          break;
        }
        cum += h;
      }
      s_digit = dsel;
      s_krem = r.krem - cum;
      s_ceq = hist[dsel];
    }
    __syncthreads();
    r.prefix |= s_digit << shift;
    mask |= 255u << shift;
    r.krem = s_krem;
    r.ceq = s_ceq;
    __syncthreads();
  }
  return r;
}
