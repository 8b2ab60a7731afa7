// Exact kNN, large-database path: the candidate lists the 16-bit filters (knn_filter_kernels.hip, knn_bf16_filter_kernels.hip) leave
// behind are RANKED here (the row rule: select_dev.h); their exact refinement is knn_refine_kernels.hip.
//   select_approx_kernel     per query: rank the candidates by d2~; intermediate level: A_k (k-th smallest);
//                            last level: the refine list {d2~ <= A_k + 2 eps}
//   select_small_kernel      the same for lists of <= 4096 keys, a wave per list
//   select_wg_kernel         the same for ONE query image per pass (<= 128 lists): a workgroup per list
//   l0_reduce_rank_kernel    the sampled exact level of such a pass: split-k partial sums -> distances -> rank thresholds
//   refine2_compact_kernel   second refinement tier: a band that outgrew its refine list, compacted out of the candidate list
#include <stdlib.h>

#include <stdio.h>

#include "ctx.h"
#include "knn_dev.h"
#include "select_dev.h"

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
