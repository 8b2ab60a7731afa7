// Exact kNN, large-database path: what happens to the candidate lists the 16-bit filters (knn_filter_kernels.hip, knn_bf16_filter_kernels.hip) leave behind.
//   select_approx_kernel     per query: sort candidates by d2~; intermediate level: A_k (k-th smallest);
//                            last level: the refine list {d2~ <= A_k + 2 eps}
//   refine_exact_kernel      per query: exact fp32 distances of the refine list (the SAME sequential fp32 fma chain as the
//                            matrix path, gemm_nt_kernel<1>), sort by (distance, id), top-k
//   select_wg_kernel / refine_exact_small_kernel   the same two steps for ONE query image per pass (<= 128 lists): a
//                            workgroup per list, refinement lists shared by workgroups
//   l0_reduce_rank_kernel    the sampled exact level of such a pass: split-k partial sums -> distances -> rank thresholds
#include <stdlib.h>

#include <stdio.h>

#include "ctx.h"
#include "knn_dev.h"
#include "select_dev.h"
#include "small_pass_dev.h"

// ---- candidate handling ----------------------------------------------------------------------------------
// Candidate lists are only RANKED here, never sorted: a radix select over the keys yields A, the k-th smallest approximate
// distance (+inf if fewer than k candidates); what A then means is the row rule of select_dev.h (SvSelectArgs, ctx.h).
// This kernel: lists beyond the wave kernel's 4096 keys, a 256-thread workgroup per list, the keys in LDS.
__global__ __launch_bounds__(256) void select_approx_kernel(SvSelectArgs a, const uint32_t* __restrict__ todo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* keys = reinterpret_cast<uint32_t*>(smem);  // [cap]
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (todo && !todo[row]) return;   // already ranked by select_small_kernel
  __shared__ uint32_t s_c;
  if (tid == 0) {
    s_c = a.cnt[row];
    if (a.mode != SvSelect::Band) a.cnt[row] = 0u;   // (Carry: set again below)
  }
  __syncthreads();
  const uint32_t c = s_c;
  const float t_in = sel_thr_in_(a, row);
  if (sel_rejects_(a, c, (uint32_t)a.cap, a.ovf_rows[row])) {
    if (tid == 0) sel_flag_row_(a, row);
    return;
  }
  for (int j = tid; j < (int)c; j += 256) keys[j] = f2key_(a.cd2[row * a.cap + j]);
  float ak = INFINITY;
  if ((int)c >= a.k) ak = key2f_(sv_radix8_select_((int)c, (uint32_t)a.k, [&](int j) { return keys[j]; }, tid).prefix);
  else __syncthreads();
  if (a.mode == SvSelect::Threshold) {
    if (tid == 0) a.thr_out[row] = ak;
    return;
  }
  if (a.mode == SvSelect::Carry) {   // in place, 256 entries at a time -- a chunk's survivors land below its own start + 256
    const float t2 = sel_carry_thr_(ak, t_in);
    const float lim2 = sel_limit_(a, row, t2);
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int j0 = 0; j0 < (int)c; j0 += 256) {
      const int j = j0 + tid;
      const float v = (j < (int)c) ? key2f_(keys[j]) : INFINITY;
      const uint32_t id = (j < (int)c) ? a.cid[row * a.cap + j] : 0u;
      __syncthreads();   // the chunk is in registers
      if (j < (int)c && v <= lim2) {
        const uint32_t pos = atomicAdd(&s_n, 1u);
        a.cd2[row * a.cap + pos] = v;
        a.cid[row * a.cap + pos] = id;
      }
      __syncthreads();   // (the next chunk's reads start at j0 + 256 >= every position written so far)
    }
    if (tid == 0) {
      a.thr_out[row] = t2;
      a.cnt[row] = s_n;
    }
    return;
  }
  if (sel_check_fails_(a, ak, t_in)) {
    if (tid == 0) sel_flag_row_(a, row);
    return;
  }
  const float flim = sel_limit_(a, row, ak);
  const uint32_t klim = f2key_(flim);
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int j = tid; j < (int)c; j += 256) {
    if (keys[j] <= klim) {
      const uint32_t slot = atomicAdd(&s_n, 1u);
      if (slot < (uint32_t)a.rcap) a.ref_id[row * a.rcap + slot] = a.cid[row * a.cap + j];
    }
  }
  __syncthreads();
  if (tid == 0) sel_close_band_(a, row, s_n, flim);
}

// The same ranking for lists of up to 4096 candidates (every list of the low-rank level scheme, and nearly every list of
// the rigorous one), one WAVE per query instead of one 256-thread workgroup: the keys live in registers (4, 16, 32 or 64 per
// lane, by the list's length), the rank-th smallest is found by the binary radix select with DPP wave reductions, the refine
// list is compacted by ballots.  No LDS, no barriers.  Longer lists are left to select_approx_kernel (todo[row] = 1).
// select_small_body: the ranking itself for lists of at most 64 * PER keys; l: the lane, c: the list's length, past the entry test.
template <int PER>
__device__ __forceinline__ void select_small_body(const SvSelectArgs& a, int64_t row, int l, uint32_t c, float t_in) {
  uint32_t key[PER], cidv[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = l + 64 * i;
    key[i] = SV_KEY_PAD;
    cidv[i] = 0u;
    if (j < (int)c) {
      key[i] = f2key_(a.cd2[row * a.cap + j]);
      // Band, Carry: the ids travel with the keys (fetched behind a ballot branch, slot by slot, each was a round trip of its
      // own: 12 of the 19 us of a pass's last select)
      if (a.mode != SvSelect::Threshold) cidv[i] = a.cid[row * a.cap + j];
    }
  }
  SvWaveReduce red;
  const float ak = sv_kth_smallest_<PER>(key, c, a.k, red);
  if (a.mode == SvSelect::Threshold) {
    if (l == 0) a.thr_out[row] = ak;
    return;
  }
  if (a.mode == SvSelect::Carry) {
    const float t2 = sel_carry_thr_(ak, t_in);
    const float lim2 = sel_limit_(a, row, t2);
    uint32_t kept = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const float v = key2f_(key[i]);
      const bool hit = key[i] != SV_KEY_PAD && v <= lim2;
      const uint64_t mk = __builtin_amdgcn_ballot_w64(hit);
      if (mk != 0ull) {
        const uint32_t pos = kept + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (hit) {   // (every key of the list is in registers: writing in place races with nothing)
          a.cd2[row * a.cap + pos] = v;
          a.cid[row * a.cap + pos] = cidv[i];
        }
        kept += (uint32_t)__popcll(mk);
      }
    }
    if (l == 0) {
      a.thr_out[row] = t2;
      a.cnt[row] = kept;
    }
    return;
  }
  if (sel_check_fails_(a, ak, t_in)) {
    if (l == 0) sel_flag_row_(a, row);
    return;
  }
  const float flim = sel_limit_(a, row, ak);
  const uint32_t klim = f2key_(flim);
  uint32_t total = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const bool hit = key[i] <= klim;   // (klim is a finite float's key: the padding never hits)
    const uint64_t mk = __builtin_amdgcn_ballot_w64(hit);
    if (mk != 0ull) {
      const uint32_t pos = total + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      if (hit && pos < (uint32_t)a.rcap) a.ref_id[row * a.rcap + pos] = cidv[i];
      total += (uint32_t)__popcll(mk);
    }
  }
  if (l == 0) sel_close_band_(a, row, total, flim);
}

// One query image per pass (<= 128 lists): a whole workgroup per list instead of a wave -- 32 keys per thread (lists of up
// to 8192 entries, the capacity of the candidate lists; longer ones are flagged for the exact path), the binary radix select
// with the workgroup reducer (one barrier per bit).
// The wave kernel's 64-keys-per-lane instantiation is ~8000 straight-line instructions that a pass runs through ONCE --
// instruction fetch, not arithmetic: 29 us for a 3906-entry sample row; this kernel takes ~10.
// PERK: keys per thread.  32 covers the candidate lists' capacity (8192, SV_CAP); 16 (lists of <= 4096 entries -- every list the
// single-image plan produces in practice) halves the slot loops of the load and of every radix step: the kernel picks the
// body by the list's length (workgroup-uniform).
template <int PERK>
__device__ __forceinline__ void select_wg_body(const SvSelectArgs& a, const uint32_t c, const float (&pre_d2)[16],
                                               const uint32_t (&pre_id)[16], const uint32_t flagged, const float t_in) {
  constexpr int PER = PERK;
  __shared__ uint32_t xs[2][4];
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  uint32_t key[PER], cidv[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = tid + 256 * i;
    key[i] = SV_KEY_PAD;
    cidv[i] = 0u;
    if (j < (int)c && c <= (uint32_t)(256 * PER)) {
      // (the first 16 slots per thread were requested by the kernel together with the list's length: one round trip, not two)
      key[i] = f2key_(i < 16 ? pre_d2[i < 16 ? i : 0] : a.cd2[row * a.cap + j]);
      if (a.mode == SvSelect::Band) cidv[i] = i < 16 ? pre_id[i < 16 ? i : 0] : a.cid[row * a.cap + j];
    }
  }
  if (tid == 0) s_n = 0u;
  __syncthreads();   // every thread has read cnt[row]
  // (no Carry in this kernel -- the host refuses it for a single image --: Threshold is the only mode that resets the counter)
  if (tid == 0 && a.mode == SvSelect::Threshold) a.cnt[row] = 0u;
  if (sel_rejects_(a, c, (uint32_t)(256 * PER), flagged)) {
    if (tid == 0) sel_flag_row_(a, row);
    return;
  }
  SvWgReduce red{xs, tid};
  const float ak = sv_kth_smallest_<PER>(key, c, a.k, red);
  if (a.mode == SvSelect::Threshold) {
    if (tid == 0) a.thr_out[row] = ak;
    return;
  }
  if (sel_check_fails_(a, ak, t_in)) {
    if (tid == 0) sel_flag_row_(a, row);
    return;
  }
  const float flim = sel_limit_(a, row, ak);
  const uint32_t klim = f2key_(flim);
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (key[i] <= klim) {   // (a finite float's key: the padding never hits)
      const uint32_t pos = atomicAdd(&s_n, 1u);
      if (pos < (uint32_t)a.rcap) a.ref_id[row * a.rcap + pos] = cidv[i];
    }
  __syncthreads();
  if (tid == 0) sel_close_band_(a, row, s_n, flim);
}

__global__ __launch_bounds__(256) void select_wg_kernel(SvSelectArgs a) {
  // Everything the list's length decides is REQUESTED before the length is known: the first 16 slots of every thread (lists of
  // <= 4096 entries -- every list the single-image plan produces in practice -- are complete with them; the slots lie inside the
  // row's `cap` entries whatever the length, entries beyond it are never looked at), the row's flag, its threshold.  The length
  // used to be a round trip of its own in front of them (round 6: ~1.5 us of a 20-us kernel that is a chain of such trips).
  const int64_t row = blockIdx.x;
  float pre_d2[16];
  uint32_t pre_id[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = threadIdx.x + 256 * i;
    const bool in = j < a.cap;
    pre_d2[i] = in ? a.cd2[row * a.cap + j] : 0.f;
    pre_id[i] = (in && a.mode == SvSelect::Band) ? a.cid[row * a.cap + j] : 0u;
  }
  const uint32_t flagged = a.ovf_rows[row];
  const float t_in = sel_thr_in_(a, row);
  const uint32_t c = a.fixed_cnt >= 0 ? (uint32_t)a.fixed_cnt : a.cnt[row];
  if (c <= 4096u) select_wg_body<16>(a, c, pre_d2, pre_id, flagged, t_in);
  else select_wg_body<32>(a, c, pre_d2, pre_id, flagged, t_in);
}

// The sampled exact level of a single-image pass: the K-split partial dot products of <= 128 query rows against <= 4096
// sample rows are reduced (slices added in index order, sv_d2 with the norms: splitk_reduce_d2_kernel's arithmetic, value for
// value) and the row's rank-th smallest distance is selected in the same workgroup -- one launch instead of two in a pass
// that is a chain of dependent launches.
__global__ __launch_bounds__(256) void l0_reduce_rank_kernel(const float* __restrict__ part, int splits, int M, int N, int64_t ldc,
                                                             const float* __restrict__ row_add, const float* __restrict__ col_add,
                                                             int b_stride, int rank, float* __restrict__ thr_out,
                                                             uint32_t* __restrict__ cnt, const uint32_t* __restrict__ ovf_rows) {
  constexpr int PER = 16;
  __shared__ uint32_t xs[2][4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t mn = (int64_t)M * ldc;
  const float q2 = row_add[row];
  // slice-major: the 16 loads of a slice are in flight together, two slices per round trip (one load after the other down a
  // column is 8 dependent round trips per key: 35 us for this kernel)
  float sum[PER], rn[PER];
  const float* p0 = part + row * ldc + tid;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const bool in = tid + 256 * i < N;
    sum[i] = in ? p0[256 * i] : 0.f;
    rn[i] = in ? col_add[(int64_t)(tid + 256 * i) * b_stride] : 0.f;
  }
  int t = 1;
  for (; t + 1 < splits; t += 2) {
    float a[PER], b[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const bool in = tid + 256 * i < N;
      a[i] = in ? p0[(int64_t)t * mn + 256 * i] : 0.f;
      b[i] = in ? p0[(int64_t)(t + 1) * mn + 256 * i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) sum[i] = (sum[i] + a[i]) + b[i];   // (index order, as splitk_reduce_d2_kernel adds them)
  }
  if (t < splits) {
#pragma unroll
    for (int i = 0; i < PER; ++i) sum[i] += (tid + 256 * i < N) ? p0[(int64_t)t * mn + 256 * i] : 0.f;
  }
  uint32_t key[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) key[i] = (tid + 256 * i < N) ? f2key_(sv_d2(q2, rn[i], sum[i])) : SV_KEY_PAD;
  if (tid == 0) cnt[row] = 0u;   // the next level's filter appends from zero
  if (ovf_rows[row] || N < rank) {   // (workgroup-uniform)
    if (tid == 0) thr_out[row] = -INFINITY;
    return;
  }
  SvWgReduce red{xs, tid};
  const float ak = sv_kth_smallest_<PER>(key, (uint32_t)N, rank, red);
  if (tid == 0) thr_out[row] = ak;
}

int sv_launch_l0_reduce_rank(segvlad_ctx* ctx, const float* parts, int splits, int M, int n_sample, int64_t ldc, const float* qn,
                             const float* rn, int b_stride, int rank, float* thr_out, uint32_t* cand_cnt, const uint32_t* fail_rows) {
  if (M <= 0) return SEGVLAD_OK;
  if (n_sample > 4096) return ctx->fail(SEGVLAD_ERR_LIMIT, "l0_reduce_rank: rows of at most 4096 columns");
  hipLaunchKernelGGL(l0_reduce_rank_kernel, dim3(M), dim3(256), 0, ctx->stream, parts, splits, M, n_sample, ldc, qn, rn, b_stride, rank,
                     thr_out, cand_cnt, fail_rows);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

__global__ __launch_bounds__(256) void select_small_kernel(SvSelectArgs a, int nq, uint32_t* __restrict__ todo) {
  constexpr int PER = 64;   // up to 4096 keys per wave, in registers
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq) return;
  const uint32_t c = a.fixed_cnt >= 0 ? (uint32_t)a.fixed_cnt : a.cnt[row];
  if (todo && c > (uint32_t)(64 * PER) && c <= (uint32_t)a.cap && !a.ovf_rows[row]) {   // long list: the workgroup kernel ranks it
    if (l == 0) todo[row] = 1u;
    return;
  }
  if (l == 0) {
    if (todo) todo[row] = 0u;
    if (a.mode != SvSelect::Band) a.cnt[row] = 0u;   // (Carry: set again by the body)
  }
  const float t_in = sel_thr_in_(a, row);
  // todo == null (a handful of queries: the workgroup kernel is not even launched): a list beyond the wave's 4096 keys is
  // treated like an overflowing one -- the query is redone on the exact path
  if (sel_rejects_(a, c, todo ? 0xffffffffu : (uint32_t)(64 * PER), a.ovf_rows[row])) {
    if (l == 0) sel_flag_row_(a, row);
    return;
  }
  if (c <= 256u) select_small_body<4>(a, row, l, c, t_in);
  else if (c <= 1024u) select_small_body<16>(a, row, l, c, t_in);
  else if (c <= 2048u) select_small_body<32>(a, row, l, c, t_in);
  else select_small_body<64>(a, row, l, c, t_in);
}

int sv_launch_select_approx(segvlad_ctx* ctx, int nq, const SvSelectArgs& a) {
  if (nq <= 0) return SEGVLAD_OK;
  if (a.mode == SvSelect::Carry && nq <= 128) return ctx->fail(SEGVLAD_ERR_STATE, "select: the carrying form exists for batches only");
  if (nq <= 128) {   // one query image per pass: a workgroup per list
    hipLaunchKernelGGL(select_wg_kernel, dim3(nq), dim3(256), 0, ctx->stream, a);
    SV_HIP(hipGetLastError());
    return SEGVLAD_OK;
  }
  const bool wave_only = a.fixed_cnt >= 0 && a.fixed_cnt <= 4096;
  uint32_t* todo = nullptr;
  if (!wave_only) {
    SV_HIP(ctx->s_sel_todo.reserve((size_t)nq * 4));
    todo = ctx->s_sel_todo.as<uint32_t>();
  }
  hipLaunchKernelGGL(select_small_kernel, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, a, nq, todo);
  if (wave_only) {   // every list is ranked (or flagged) by the wave kernel
    SV_HIP(hipGetLastError());
    return SEGVLAD_OK;
  }
  hipLaunchKernelGGL(select_approx_kernel, dim3(nq), dim3(256), (size_t)a.cap * 4, ctx->stream, a, (const uint32_t*)todo);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// Second refinement tier.  A query whose band {d2~ <= A_k + 2 eps} holds more rows than the first-tier list (SV_RCAP) --
// temporally redundant databases: every reference segment comes with its ~30 near-duplicates from the neighbouring video
// frames, so whole clumps of rows sit inside the band -- keeps its candidate list (<= cap entries, a superset of the band):
// this kernel compacts the band's ids to the front of that list, in place, and the exact refinement then runs straight
// from it (rcap = cap).  Only the flagged rows do any work; nobody is sent to the distance-matrix path for this.
__global__ __launch_bounds__(256) void refine2_compact_kernel(const uint32_t* __restrict__ rovf_rows, const float* __restrict__ ref_lim,
                                                              uint32_t* __restrict__ cnt, const float* __restrict__ cd2,
                                                              uint32_t* __restrict__ cid, int cap) {
  __shared__ uint32_t wtot[4];
  const int64_t row = blockIdx.x;
  if (!rovf_rows[row]) return;
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const uint32_t c = cnt[row];
  const float lim = ref_lim[row];
  uint32_t base = 0;
  for (uint32_t j0 = 0; j0 < c; j0 += 256) {
    const uint32_t j = j0 + tid;
    const bool hit = j < c && cd2[row * cap + j] <= lim;
    const uint32_t id = hit ? cid[row * cap + j] : 0u;
    const uint64_t mk = __builtin_amdgcn_ballot_w64(hit);
    if (l == 0) wtot[w] = (uint32_t)__popcll(mk);
    __syncthreads();   // every read of this chunk precedes its writes (which land at positions <= the reads': in place is safe)
    uint32_t off = base;
    for (int x = 0; x < w; ++x) off += wtot[x];
    const uint32_t pos = off + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (hit) cid[row * cap + pos] = id;
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (tid == 0) cnt[row] = base;
}

int sv_launch_refine2_compact(segvlad_ctx* ctx, const uint32_t* rovf_rows, const float* ref_lim, uint32_t* cand_cnt,
                              const float* cand_d2, uint32_t* cand_id, int nq, int cap) {
  if (nq <= 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(refine2_compact_kernel, dim3(nq), dim3(256), 0, ctx->stream, rovf_rows, ref_lim, cand_cnt, cand_d2, cand_id, cap);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// exact distances of the refine list: the sequential fp32 fma chain over k = 0..d-1 (bit-identical to the
// v_mfma_f32_32x32x2_f32 chain of the matrix path), then (distance, id) sort and top-k.  One thread per candidate row; the
// query row is cached in LDS (QLDS; d up to ~38k).  The row is walked with THIRTY-TWO 16-byte loads in flight per thread:
// a 50-query pass has fewer waves than the chip has SIMDs, so the loop is pure load latency -- one round trip per
// 32 x 16 B (an 8-deep register double buffer still paid one round trip per 128 B: 78 us per pass).
// only_rows != null: rows whose flag is clear are left untouched (second refinement tier).
template <bool QLDS>
__global__ __launch_bounds__(256) void refine_exact_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                           const float* __restrict__ qn, const float* __restrict__ rn,
                                                           const uint32_t* __restrict__ ref_cnt,
                                                           const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                           float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                           const uint32_t* __restrict__ only_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                     // [d] when QLDS
  uint64_t* a = reinterpret_cast<uint64_t*>(smem + (QLDS ? (size_t)d * 4 : 0));   // [rpad]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (only_rows && !only_rows[row]) return;
  const int n = (int)ref_cnt[row];
  int np2 = 2;   // sort length: the smallest power of two holding the list (<= rpad)
  while (np2 < n) np2 <<= 1;
  if (QLDS)
    for (int j = tid; j < d; j += 256) qs[j] = Q[row * d + j];
  for (int j = tid; j < np2; j += 256) a[j] = ~0ull;
  __syncthreads();
  const float q2 = qn[row];
  const float4* qp = QLDS ? reinterpret_cast<const float4*>(qs) : reinterpret_cast<const float4*>(Q + row * d);
  const int n4 = d >> 2;
  for (int j = tid; j < n; j += 256) {
    const uint32_t id = ref_id[row * rcap + j];
    const float4* rp = reinterpret_cast<const float4*>(R + (size_t)id * d);
    float acc = 0.f;
    int t = 0;
    if ((n4 & 31) == 0) {
      for (; t < n4; t += 32) {   // 512 B of the row in flight per lane: 8 round trips for a 1024-d row
        float4 buf[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) buf[u] = rp[t + u];
        __builtin_amdgcn_sched_barrier(0);   // all 32 loads are issued before the first fma (the scheduler otherwise
                                             // sinks them next to their uses to save registers -- and pays the latency 32 times)
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const float4 qv = qp[t + u];
          acc = fmaf(qv.x, buf[u].x, acc);
          acc = fmaf(qv.y, buf[u].y, acc);
          acc = fmaf(qv.z, buf[u].z, acc);
          acc = fmaf(qv.w, buf[u].w, acc);
        }
      }
    } else {
      for (; t < n4; ++t) {
        const float4 rv = rp[t];
        const float4 qv = qp[t];
        acc = fmaf(qv.x, rv.x, acc);
        acc = fmaf(qv.y, rv.y, acc);
        acc = fmaf(qv.z, rv.z, acc);
        acc = fmaf(qv.w, rv.w, acc);
      }
    }
    const float v = sv_d2(q2, rn[id], acc);
    a[j] = ((uint64_t)f2key_(v) << 32) | id;
  }
  sv_bitonic(a, np2, tid);
  for (int j = tid; j < k; j += 256) {
    float dd = INFINITY;
    int64_t id = -1;
    if (j < n) {
      dd = key2f_((uint32_t)(a[j] >> 32));
      id = (int64_t)(uint32_t)a[j];
    }
    d2_out[row * k + j] = dd;
    idx_out[row * k + j] = id;
  }
}

// Deep rows (raw K*D descriptors: d = 98 304 is 384 KiB per row, far beyond the LDS and -- one row per lane -- beyond what
// L1 can keep of 256 private streams): the same sequential chain, with the candidate rows fetched COALESCED (KC * 4 bytes
// of a row per step: C4 lanes x 16 B) into an LDS tile [64 rows][KC (+4 pad)], double buffered, which the 64 lanes of wave 0
// then walk ONE ROW EACH (conflict-free ds_read_b128: the row stride is 4 banks mod 64); all four waves load.
// What bounds it is bytes in flight: one workgroup per CU (the tile) with one step of 32 KiB outstanding ran at 1.4-1.8 TB/s
// -- piece size, a time skew between the rows and the 3 * 2^17-byte row pitch made no difference, and
// tools/ubench/gather_bw.hip reaches 7 TB/s on the same addresses with 256 KiB per CU in flight.  So the loads run DEPTH
// steps ahead in a register ring (DEPTH x NP float4 per thread: 128 KiB per CU at DEPTH = 4), and only the step that is due
// is written to the LDS tile.  d % KC == 0.
template <int KC, int DEPTH>
__global__ __launch_bounds__(256) void refine_exact_wide_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                                const float* __restrict__ qn, const float* __restrict__ rn,
                                                                const uint32_t* __restrict__ ref_cnt,
                                                                const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                                float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                                const uint32_t* __restrict__ only_rows) {
  constexpr int ROWS = 64, LDR = KC + 4, C4 = KC / 4;    // C4 16-byte pieces per row and step
  constexpr int NP = ROWS * C4 / 256;                    // pieces per thread and step
  constexpr int RSTEP = 256 / C4;                        // tile rows between two pieces of a thread
  static_assert(C4 <= 64 && 64 % C4 == 0 && NP * 256 == ROWS * C4, "a wave covers whole rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);                                 // [2][ROWS][LDR]
  float* qs = tile + 2 * ROWS * LDR;                                            // [2][KC]
  uint32_t* ids = reinterpret_cast<uint32_t*>(qs + 2 * KC);                     // [ROWS]
  uint64_t* a = reinterpret_cast<uint64_t*>(ids + ROWS);                        // [rpad]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (only_rows && !only_rows[row]) return;
  const int n = (int)ref_cnt[row];
  int np2 = 2;
  while (np2 < n) np2 <<= 1;
  for (int j = tid; j < np2; j += 256) a[j] = ~0ull;
  const float q2 = qn[row];
  const float* qrow = Q + row * d + (tid < C4 ? tid * 4 : 0);
  const int nch = d / KC;
  const int seg = tid % C4, lrow0 = tid / C4;   // piece u of this thread: tile row lrow0 + RSTEP u, 16-byte segment seg
  for (int base = 0; base < n; base += ROWS) {
    const int cnt = (n - base < ROWS) ? (n - base) : ROWS;
    __syncthreads();   // the previous pass is done with ids[] and the tile
    if (tid < cnt) ids[tid] = ref_id[row * rcap + base + tid];
    __syncthreads();
    // (no per-piece predication: a branch around every load makes the compiler wait for each one.  Tile rows beyond the
    //  list re-read candidate 0 -- L2 hits -- and are never looked at; every thread carries a query piece, lanes >= C4 a
    //  duplicate of piece 0 that is never stored)
    const float* src[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int lr = lrow0 + RSTEP * u;
      src[u] = R + (size_t)ids[lr < cnt ? lr : 0] * d + seg * 4;
    }
    // The ring is four NAMED register sets and the step is a macro instantiated once per set: hipcc 7.2 sends a
    // [DEPTH][NP] array that is indexed through a lambda parameter to scratch memory (seen in the ISA: scratch_load/_store
    // around every piece, vmcnt(0) after every load).
    static_assert(DEPTH == 4 && NP == 8, "four named ring sets of eight named pieces");
#define SV_WG_DECL(X) float4 g##X##0, g##X##1, g##X##2, g##X##3, g##X##4, g##X##5, g##X##6, g##X##7, q##X
    SV_WG_DECL(A);
    SV_WG_DECL(B);
    SV_WG_DECL(C);
    SV_WG_DECL(D);
#define SV_WG_LOAD(X, c_)                                                          \
    do {                                                                           \
      const size_t o_ = (size_t)(c_) * KC;                                         \
      g##X##0 = *reinterpret_cast<const float4*>(src[0] + o_);                     \
      g##X##1 = *reinterpret_cast<const float4*>(src[1] + o_);                     \
      g##X##2 = *reinterpret_cast<const float4*>(src[2] + o_);                     \
      g##X##3 = *reinterpret_cast<const float4*>(src[3] + o_);                     \
      g##X##4 = *reinterpret_cast<const float4*>(src[4] + o_);                     \
      g##X##5 = *reinterpret_cast<const float4*>(src[5] + o_);                     \
      g##X##6 = *reinterpret_cast<const float4*>(src[6] + o_);                     \
      g##X##7 = *reinterpret_cast<const float4*>(src[7] + o_);                     \
      q##X = *reinterpret_cast<const float4*>(qrow + o_);                          \
    } while (0)
#define SV_WG_STORE(X, buf_)                                                       \
    do {                                                                           \
      float* t_ = tile + ((size_t)(buf_) * ROWS + lrow0) * LDR + seg * 4;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 0 * LDR) = g##X##0;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 1 * LDR) = g##X##1;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 2 * LDR) = g##X##2;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 3 * LDR) = g##X##3;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 4 * LDR) = g##X##4;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 5 * LDR) = g##X##5;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 6 * LDR) = g##X##6;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 7 * LDR) = g##X##7;          \
      if (tid < C4) *reinterpret_cast<float4*>(qs + (buf_) * KC + tid * 4) = q##X; \
    } while (0)
    // one step: multiply step c out of tile buffer c & 1, move step c + 1 (ring set XN) into the other buffer, request
    // step c + 1 + DEPTH into the set that just became free
#define SV_WG_MUL(c)                                                                                       \
    if (tid < cnt) {                                                                                       \
      const float* tr = tile + ((size_t)((c) & 1) * ROWS + tid) * LDR;                                     \
      const float* qb = qs + ((c) & 1) * KC;                                                               \
      _Pragma("unroll 8") for (int s4 = 0; s4 < C4; ++s4) {                                                \
        const float4 rv = *reinterpret_cast<const float4*>(tr + s4 * 4);                                   \
        const float4 qv = *reinterpret_cast<const float4*>(qb + s4 * 4);                                   \
        acc = fmaf(qv.x, rv.x, acc);                                                                       \
        acc = fmaf(qv.y, rv.y, acc);                                                                       \
        acc = fmaf(qv.z, rv.z, acc);                                                                       \
        acc = fmaf(qv.w, rv.w, acc);                                                                       \
      }                                                                                                    \
    }
    // steady state (no conditions on the loads: the compiler's wait counts then leave the three younger steps in flight)
#define SV_WG_STEP_FULL(c_, XN)                                                                            \
    do {                                                                                                   \
      const int c = (c_);                                                                                  \
      SV_WG_MUL(c)                                                                                         \
      SV_WG_STORE(XN, (c + 1) & 1);                                                                        \
      SV_WG_LOAD(XN, c + 1 + DEPTH);                                                                       \
      __syncthreads();                                                                                     \
    } while (0)
#define SV_WG_STEP(c_, XN)                                                                                 \
    do {                                                                                                   \
      const int c = (c_);                                                                                  \
      if (c < nch) {                                                                                       \
        if (tid < cnt) {                                                                                   \
          const float* tr = tile + ((size_t)(c & 1) * ROWS + tid) * LDR;                                   \
          const float* qb = qs + (c & 1) * KC;                                                             \
          _Pragma("unroll 8") for (int s4 = 0; s4 < C4; ++s4) {                                            \
            const float4 rv = *reinterpret_cast<const float4*>(tr + s4 * 4);                               \
            const float4 qv = *reinterpret_cast<const float4*>(qb + s4 * 4);                               \
            acc = fmaf(qv.x, rv.x, acc);                                                                   \
            acc = fmaf(qv.y, rv.y, acc);                                                                   \
            acc = fmaf(qv.z, rv.z, acc);                                                                   \
            acc = fmaf(qv.w, rv.w, acc);                                                                   \
          }                                                                                                \
        }                                                                                                  \
        if (c + 1 < nch) {                                                                                 \
          SV_WG_STORE(XN, (c + 1) & 1);   /* waits for the loads of step c + 1 only */                     \
          if (c + 1 + DEPTH < nch) SV_WG_LOAD(XN, c + 1 + DEPTH);                                          \
        }                                                                                                  \
        __syncthreads();                                                                                   \
      }                                                                                                    \
    } while (0)
    float acc = 0.f;
    // set A holds steps 0, 4, 8, ...; B 1, 5, ...; C 2, 6, ...; D 3, 7, ...
    SV_WG_LOAD(A, 0);
    if (1 < nch) SV_WG_LOAD(B, 1);
    if (2 < nch) SV_WG_LOAD(C, 2);
    if (3 < nch) SV_WG_LOAD(D, 3);
    SV_WG_STORE(A, 0);
    if (4 < nch) SV_WG_LOAD(A, 4);
    __syncthreads();
    int c0 = 0;
    for (; c0 + 3 + 1 + DEPTH < nch; c0 += 4) {   // every load of these four steps exists
      SV_WG_STEP_FULL(c0, B);
      SV_WG_STEP_FULL(c0 + 1, C);
      SV_WG_STEP_FULL(c0 + 2, D);
      SV_WG_STEP_FULL(c0 + 3, A);
    }
    for (; c0 < nch; c0 += 4) {                    // the last steps: nothing (or not everything) left to request
      SV_WG_STEP(c0, B);
      SV_WG_STEP(c0 + 1, C);
      SV_WG_STEP(c0 + 2, D);
      SV_WG_STEP(c0 + 3, A);
    }
#undef SV_WG_STEP
#undef SV_WG_STEP_FULL
#undef SV_WG_MUL
#undef SV_WG_STORE
#undef SV_WG_LOAD
#undef SV_WG_DECL
    if (tid < cnt) {
      const uint32_t id = ids[tid];
      a[base + tid] = ((uint64_t)f2key_(sv_d2(q2, rn[id], acc)) << 32) | id;
    }
  }
  sv_bitonic(a, np2, tid);
  for (int j = tid; j < k; j += 256) {
    float dd = INFINITY;
    int64_t id = -1;
    if (j < n) {
      dd = key2f_((uint32_t)(a[j] >> 32));
      id = (int64_t)(uint32_t)a[j];
    }
    d2_out[row * k + j] = dd;
    idx_out[row * k + j] = id;
  }
}

// A handful of queries (one query image per pass): fewer lists than CUs, and a list walked by ONE workgroup is one memory
// round trip after the other (59 us for 240 rows of 1024 floats).  Here a list is dealt to `parts` workgroups, 32 rows each:
// a workgroup requests 1024 floats of each of its 32 rows in ONE burst (thread t: 16 bytes of row 2 j + (t >> 7), in both
// 512-float halves: 32 coalesced loads in flight per thread, one round trip per 1024 floats), parks one half at a time in an
// LDS tile [32][516], and 32 lanes walk one row each (the same sequential fp32 chain; the query's floats are LDS
// broadcasts).  The keys go to global memory as device-scope stores; the workgroup that takes the last ticket of its query
// reads them back, sorts them and writes the top k.  d % 1024 == 0.  tick[] is all zero before and after.
// Measured (50 queries x ~240 rows, 1 M x 1024 index): 59 us -> 34-38 us; what is left is a chain of ~7 dependent memory
// round trips (list length + ids, rows, key stores, ticket, key loads, results) around 5 us of arithmetic.
constexpr int SV_TICK_ROWS = 128, SV_TICK_POISON = SV_TICK_ROWS;   // tick[0..127]: one ticket counter per query; [128]: sticky failure word
__global__ __launch_bounds__(256) void refine_exact_small_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                                 const float* __restrict__ qn, const float* __restrict__ rn,
                                                                 const uint32_t* __restrict__ ref_cnt,
                                                                 const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                                 float* __restrict__ d2_out, int64_t* __restrict__ idx_out, int parts,
                                                                 uint64_t* __restrict__ gkeys, uint32_t* __restrict__ tick,
                                                                 uint32_t* __restrict__ fail_rows, uint32_t* __restrict__ fail_count,
                                                                 SvSmallFinish fz) {
  constexpr int ROWS = 32, KC = 512, LDR = KC + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);                  // [ROWS][LDR]
  uint64_t* a = reinterpret_cast<uint64_t*>(tile + ROWS * LDR);  // [rpad]
  __shared__ uint32_t ids[ROWS];
  __shared__ int last;
  const int tid = threadIdx.x;
#ifdef SV_REFINE_TIMING
  unsigned long long T[12];
  int ti = 0;
#define RTICK() T[ti++] = __builtin_amdgcn_s_memtime()
#else
#define RTICK()
#endif
  RTICK();
  // part-major: the first workgroups of the grid are part 0 of EVERY list, then part 1, ... -- the parts that hold rows (a band of ~270
  // rows: parts 0-8 of 16) are all resident in the first round of workgroups, the empty ones come last and leave at once.  Row-major
  // (rounds 3-5) put all 16 parts of lists 0-31 into the 512 resident slots and made lists 32-49 wait for them (round 6: 40 -> 33 us).
  const int nlists = (int)(gridDim.x / parts);
  const int64_t row = blockIdx.x % nlists;
  const int base = (int)(blockIdx.x / nlists) * ROWS;
  // the list's length and this workgroup's slice of it are requested together (the slice lies inside the list's rcap slots
  // whatever the length; entries beyond it are not looked at)
  const uint32_t idv = tid < ROWS ? ref_id[row * rcap + base + tid] : 0u;
  // fz.on (round 6, second step: the pass WITHOUT small_tail_kernel -- every kernel boundary of this chain costs 4-5 us, whatever the
  // kernel does): the rows the select flagged are finished HERE, by the row's own `parts` workgroups -- a band that outgrew the
  // first tier: every part evaluates its slice of the candidate list, the last one sorts; a row flagged for the redo: exact brute
  // force, every part a slice of the index, the last one merges (small_pass_dev.h; the same chain, sv_d2, (distance, id) order).
  // The two flags are requested with the list's length: no extra round trip on the common path.
  const uint32_t f_fail = fz.on ? fail_rows[row] : 0u, f_rovf = fz.on ? fz.rovf_rows[row] : 0u;
  const int n = (int)ref_cnt[row];
  if (f_fail | f_rovf) {   // (workgroup-uniform)
    const int p = (int)(blockIdx.x / nlists);
    uint64_t* a2 = reinterpret_cast<uint64_t*>(smem);                 // <= 8192 words of sort scratch
    float* qs2 = reinterpret_cast<float*>(smem + 65536);              // 1024 floats
    uint64_t* best2 = a2 + 2048;                                      // (brute force: the sort scratch is 2048 words)
    uint64_t* slot = fz.part2 + (size_t)row * fz.row_words;           // this row's words of the exchange buffer
    if (f_fail) sp_brute_slice(Q, R, qn, rn, fz.n_db, d, k, fz.kp, row, p, parts, slot, a2, best2, qs2, tid);
    else sp_tier2_slice(Q, R, qn, rn, d, row, p, parts, min(fz.cand_cnt[row], (uint32_t)fz.cap), fz.ref_lim[row], fz.cand_d2, fz.cand_id, fz.cap, slot,
                        qs2, tid);
    __threadfence();
    __syncthreads();
    if (tid == 0) last = (__hip_atomic_fetch_add(&tick[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(parts - 1));
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (f_fail) {
      sp_brute_merge(slot, k, fz.kp, parts, a2, best2, tid);
      for (int j = tid; j < k; j += 256) {
        const uint64_t v = best2[j];
        d2_out[row * k + j] = v != ~0ull ? key2f_((uint32_t)(v >> 32)) : INFINITY;
        idx_out[row * k + j] = v != ~0ull ? (int64_t)(uint32_t)v : -1;
      }
    } else {
      const int c = (int)min(fz.cand_cnt[row], (uint32_t)fz.cap);
      int np2 = 2;
      while (np2 < c) np2 <<= 1;
      for (int j = tid; j < np2; j += 256)
        a2[j] = j < c ? __hip_atomic_load(&slot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
      sv_bitonic(a2, np2, tid);
      for (int j = tid; j < k; j += 256) {
        const uint64_t v = j < np2 ? a2[j] : ~0ull;
        d2_out[row * k + j] = v != ~0ull ? key2f_((uint32_t)(v >> 32)) : INFINITY;
        idx_out[row * k + j] = v != ~0ull ? (int64_t)(uint32_t)v : -1;
      }
    }
    if (tid == 0) {
      __hip_atomic_store(&tick[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(&fz.stats[f_fail ? 0 : 1], 1u);
      const uint32_t tot = atomicAdd(&fz.totals[f_fail ? 0 : 1], 1u) + 1u;
      if (fz.host_totals) fz.host_totals[f_fail ? 0 : 1] = tot;   // (the pinned mirror: the latest writer's total)
    }
    return;
  }
  const int cnt = min(ROWS, n - base);
  RTICK();   // T1: list length + ids
  if (cnt > 0) {
    if (tid < ROWS) ids[tid] = idv;
    __syncthreads();
    if (tid >= cnt && tid < ROWS) ids[tid] = ids[0];   // rows beyond the list re-read its first one
    __syncthreads();
    const int h = tid >> 7, off = (tid & 127) * 4;
    // (named registers: hipcc 7.2 sends a float4 g[..] filled in an unrolled loop to scratch memory here, with a vmcnt(0)
    //  behind every load)
#define SV_RS_J(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15)
#define SV_RS_SRC(j) const float* src##j = R + (size_t)ids[2 * j + h] * d + off;
#define SV_RS_LOAD(j)                                                       \
  const float4 gA##j = *reinterpret_cast<const float4*>(src##j + c0);        \
  const float4 gB##j = *reinterpret_cast<const float4*>(src##j + c0 + KC);
#define SV_RS_STORE_A(j) *reinterpret_cast<float4*>(tile + (2 * j + h) * LDR + off) = gA##j;
#define SV_RS_STORE_B(j) *reinterpret_cast<float4*>(tile + (2 * j + h) * LDR + off) = gB##j;
#define SV_RS_WALK(c_)                                                      \
  if (tid < cnt) {                                                          \
    const float* tr = tile + tid * LDR;                                     \
    const float* qb = qs + (c_);                                            \
    _Pragma("unroll 16") for (int s4 = 0; s4 < KC / 4; ++s4) {              \
      const float4 rv = *reinterpret_cast<const float4*>(tr + s4 * 4);      \
      const float4 qv = *reinterpret_cast<const float4*>(qb + s4 * 4);      \
      acc = fmaf(qv.x, rv.x, acc);                                          \
      acc = fmaf(qv.y, rv.y, acc);                                          \
      acc = fmaf(qv.z, rv.z, acc);                                          \
      acc = fmaf(qv.w, rv.w, acc);                                          \
    }                                                                       \
  }
    SV_RS_J(SV_RS_SRC)
    // (the query's 1024 floats of the step sit in LDS beside the tile, read as broadcasts: through the scalar cache every
    //  batch of 64 floats was a cold ~0.7 us miss in front of its fmas)
    float* qs = reinterpret_cast<float*>(a + rpad);   // [2 KC]
    const float* qsrc = Q + row * d + tid * 4;
    float acc = 0.f;
    for (int c0 = 0; c0 < d; c0 += 2 * KC) {
      SV_RS_J(SV_RS_LOAD)
      const float4 qv4 = *reinterpret_cast<const float4*>(qsrc + c0);
      if (c0) __syncthreads();   // the walkers are done with the previous half
      SV_RS_J(SV_RS_STORE_A)
      *reinterpret_cast<float4*>(qs + tid * 4) = qv4;
      __syncthreads();
      SV_RS_WALK(0)
      __syncthreads();
      SV_RS_J(SV_RS_STORE_B)
      __syncthreads();
      SV_RS_WALK(KC)
    }
#undef SV_RS_WALK
#undef SV_RS_STORE_B
#undef SV_RS_STORE_A
#undef SV_RS_LOAD
#undef SV_RS_SRC
#undef SV_RS_J
    RTICK();   // T2: rows loaded and walked
    if (tid < cnt) {
      const uint32_t id = ids[tid];
      __hip_atomic_store(&gkeys[row * rcap + base + tid], ((uint64_t)f2key_(sv_d2(qn[row], rn[id], acc)) << 32) | id, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // The keys are device-scope (write-through) stores and device-scope loads; each wave waits for its stores to be
  // acknowledged before the barrier that precedes the ticket.  (A __threadfence() on either side is an L2 write-back +
  // invalidate on this eight-L2 part.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) last = (__hip_atomic_fetch_add(&tick[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(parts - 1));
  __syncthreads();
  RTICK();   // T3: key stores acknowledged + ticket
  if (!last) return;
  int np2 = 2;
  while (np2 < n) np2 <<= 1;
  // Ordering.  Every access to gkeys / tick is an agent-scope atomic (sc1: performed at the memory side, never served from
  // an XCD's own L2), the writers wait for their key stores to be ACKNOWLEDGED (vmcnt(0)) before the barrier in front of the
  // ticket, and the reader issues its loads after its ticket returned: on this hardware that is a release / acquire chain
  // through the ticket.  The C++ model does not promise it for relaxed atomics, and a formal acq_rel ticket costs an L2
  // write-back + invalidate per workgroup (see above) -- so the protocol is CHECKED instead of trusted: gkeys holds all ones
  // wherever no key of this launch has landed (the launcher fills a new buffer so, the reader puts the fill back behind
  // every key it takes; a key is never all ones: finite distance, 32-bit id); a slot still all ones is re-read a bounded
  // number of times, and a slot that never fills FLAGS its query (fail_rows: the caller redoes flagged rows on another
  // path, exactly) and raises the sticky word tick[SV_TICK_POISON], on which the host re-initialises both buffers before
  // their next use (a key landing after the reader gave up would otherwise pass for a key of the next launch).
  int holes = 0;
  for (int j = tid; j < np2; j += 256) {
    uint64_t v = ~0ull;
    if (j < n) {
      for (int spin = 0; spin < 4096; ++spin) {
        v = __hip_atomic_load(&gkeys[row * rcap + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v != ~0ull) break;
      }
      if (v == ~0ull) ++holes;
      __hip_atomic_store(&gkeys[row * rcap + j], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a[j] = v;
  }
  if (tid == 0) __hip_atomic_store(&tick[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (fz.on && (fz.debug & 8) && row == 1) holes = 1;   // (tests: the path below has never been taken by the hardware)
  if (__syncthreads_or(holes)) {   // (never observed)
    if (tid == 0) __hip_atomic_store(&tick[SV_TICK_POISON], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!fz.on) {   // the row's output is left to the redo (the caller's read-back, or small_tail_kernel)
      if (tid == 0 && fail_rows) sv_flag_once_(fail_rows, fail_count, row);
      return;
    }
    // fused finish: nobody comes after this kernel -- this workgroup re-evaluates the row's whole band itself (<= rcap rows, a thread
    // per row: the same chain); the sticky word makes the NEXT pass's head refill the hand-over buffers (a key that lands late must
    // not pass for a key of that pass)
    float* qs2 = reinterpret_cast<float*>(smem);   // (the row tile is free: every part has drawn its ticket)
    for (int j0 = 0; j0 < n; j0 += 256) {
      const int j = j0 + tid;
      const uint32_t id = ref_id[row * rcap + min(j, n - 1)];
      float acc2[1] = {0.f};
      for (int c0 = 0; c0 < d; c0 += ST_KC) {
        const int kc = min(ST_KC, d - c0);
        __syncthreads();
        for (int t = tid; t < kc; t += 256) qs2[t] = Q[row * d + c0 + t];
        __syncthreads();
        chain_step<1>(R + (size_t)id * d + c0, kc, qs2, acc2);
      }
      if (j < n) a[j] = ((uint64_t)f2key_(sv_d2(qn[row], rn[id], acc2[0])) << 32) | id;
    }
    __syncthreads();
    if (tid == 0) atomicAdd(&fz.stats[2], 1u);
  }
  RTICK();   // T4: keys read back
  // (distance, id) order WITHOUT a sort: the keys are distinct (the id is part of them), so a key's place in the sorted list is the
  // number of smaller keys -- every thread counts that for its own one or two keys against the n keys in LDS (broadcast reads, no
  // barrier) and writes its result straight to that place.  The bitonic sort of 512 words was 45 barrier-separated stages: 9.6 us of
  // the last workgroup's 25 (round 6); the count is ~2.
  for (int j = tid; j < n; j += 256) {
    const uint64_t v = a[j];
    int place = 0;
#pragma unroll 8
    for (int t = 0; t < n; ++t) place += (a[t] < v) ? 1 : 0;
    if (place < k) {
      d2_out[row * k + place] = key2f_((uint32_t)(v >> 32));
      idx_out[row * k + place] = (int64_t)(uint32_t)v;
    }
  }
  for (int j = n + tid; j < k; j += 256) {   // a list shorter than k pads with (inf, -1)
    d2_out[row * k + j] = INFINITY;
    idx_out[row * k + j] = -1;
  }
  RTICK();   // T5: placed
#ifdef SV_REFINE_TIMING
  if (tid == 0 && row == 0 && cnt > 0)
    printf("refine row0 last wg: ids %llu rows+walk %llu store+ticket %llu readback %llu sort %llu cycles (n=%d)\n", T[1]-T[0], T[2]-T[1], T[3]-T[2], T[4]-T[3], T[5]-T[4], n);
#endif
#undef RTICK
}

int sv_refine_small_repair(segvlad_ctx* ctx) {
  // the hand-over buffers of refine_exact_small_kernel back to their initial state (all ones / all zero)
  if (ctx->s_ref_tick.p) SV_HIP(hipMemsetAsync(ctx->s_ref_tick.p, 0, ctx->s_ref_tick.cap, ctx->stream));
  if (ctx->s_ref_keys.p) SV_HIP(hipMemsetAsync(ctx->s_ref_keys.p, 0xff, ctx->s_ref_keys.cap, ctx->stream));
  return SEGVLAD_OK;
}

int sv_launch_refine_exact(segvlad_ctx* ctx, const float* Q, const float* R, int nq, int d, const float* qn, const float* rn,
                           const uint32_t* ref_cnt, const uint32_t* ref_id, int rcap, int k, float* d2_out, int64_t* idx_out,
                           const uint32_t* only_rows, uint32_t* fail_rows, uint32_t* fail_count, const uint32_t** poison_dev,
                           const SvSmallFinish* fz, bool* fused_done) {
  if (poison_dev) *poison_dev = nullptr;
  if (fused_done) *fused_done = false;
  if (nq <= 0) return SEGVLAD_OK;
  int rpad = 2;
  while (rpad < rcap) rpad <<= 1;
  size_t lds = (size_t)d * 4 + (size_t)rpad * 8;
  if (nq <= SV_TICK_ROWS && d % 1024 == 0 && rcap <= 1024 && rcap % 32 == 0 && !only_rows) {   // one query image: lists shared by workgroups
    const int parts = rcap / 32;
    const size_t tick_cap = ctx->s_ref_tick.cap;
    SV_HIP(ctx->s_ref_tick.reserve((size_t)(SV_TICK_ROWS + 1) * 4));
    if (ctx->s_ref_tick.cap != tick_cap) SV_HIP(hipMemsetAsync(ctx->s_ref_tick.p, 0, ctx->s_ref_tick.cap, ctx->stream));
    const size_t keys_cap = ctx->s_ref_keys.cap;
    SV_HIP(ctx->s_ref_keys.reserve((size_t)nq * rcap * 8));
    if (ctx->s_ref_keys.cap != keys_cap) SV_HIP(hipMemsetAsync(ctx->s_ref_keys.p, 0xff, ctx->s_ref_keys.cap, ctx->stream));
    lds = (size_t)(32 * 516 + 1024) * 4 + (size_t)rpad * 8;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_small_kernel), lds));
    SvSmallFinish f;   // (off)
    if (fz && fz->on && fail_rows && fused_done && k <= 1024) {
      // the flagged rows' exchange words: a row's `parts` lists of kp keys (brute force) or its `cap` candidate keys (second tier)
      f = *fz;
      f.kp = 256;
      while (f.kp < k) f.kp <<= 1;
      f.row_words = std::max<int64_t>((int64_t)parts * f.kp, f.cap);
      SV_HIP(ctx->s_tail_part.reserve((size_t)nq * f.row_words * 8));
      SV_TRY(sv_small_words(ctx));
      SV_TRY(sv_ensure_pinned_words(ctx));
      f.part2 = ctx->s_tail_part.as<uint64_t>();
      f.totals = ctx->s_tail_tick.as<uint32_t>() + 129;
      f.host_totals = ctx->h_pin + 8;
      f.debug = ctx->opt.debug_small_tail;
      *fused_done = true;
    }
    hipLaunchKernelGGL(refine_exact_small_kernel, dim3(nq * parts), dim3(256), lds, ctx->stream, Q, R, d, qn, rn, ref_cnt, ref_id, rcap,
                       rpad, k, d2_out, idx_out, parts, ctx->s_ref_keys.as<uint64_t>(), ctx->s_ref_tick.as<uint32_t>(), fail_rows, fail_count, f);
    SV_HIP(hipGetLastError());
    if (poison_dev) *poison_dev = ctx->s_ref_tick.as<uint32_t>() + SV_TICK_POISON;
    return SEGVLAD_OK;
  }
#define SV_REFINE_ARGS dim3(nq), dim3(256), lds, ctx->stream, Q, R, d, qn, rn, ref_cnt, ref_id, rcap, rpad, k, d2_out, idx_out, only_rows
  if (lds <= 160 * 1024) {
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_kernel<true>), lds));
    hipLaunchKernelGGL(refine_exact_kernel<true>, SV_REFINE_ARGS);
  } else if (d % 128 == 0) {
    // [2][64 rows][132] floats + [2][128] query floats + [64] ids + the sort keys (<= 64 KiB for a second-tier list)
    lds = (size_t)(2 * 64 * 132 + 2 * 128 + 64) * 4 + (size_t)rpad * 8;
    if (lds > 160 * 1024) return ctx->fail(SEGVLAD_ERR_LIMIT, "refine: a %d-entry list of %d-d rows exceeds the LDS", rcap, d);
    auto kern = refine_exact_wide_kernel<128, 4>;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, SV_REFINE_ARGS);
  } else {
    lds = (size_t)rpad * 8;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_kernel<false>), lds));
    hipLaunchKernelGGL(refine_exact_kernel<false>, SV_REFINE_ARGS);
  }
#undef SV_REFINE_ARGS
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
