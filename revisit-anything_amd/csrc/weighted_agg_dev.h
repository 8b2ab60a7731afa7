// The frame of the weighted aggregations (soft_aggregate_kernel, soft_vlad_kernels.hip; burst_seg_aggregate_kernel<HARD>,
// burst_seg_kernels.hip).  Workgroup = (kpb consecutive clusters, image b, 32 segments of it), wave w owns d in [128 w, 128 w + 128):
// aggregate_kernel's geometry with one M-tile.  Per cluster k an MFMA product (32 segments x 2 tokens) . (2 tokens x 32 d) over a list of
// token positions in LDS leaves acc[4] (the four d of the lane's 16 bytes); then ||V[s][k]|| across the workgroup, the block norm, and the
// intra-normalised block stored packed.  This file holds what the kernels share -- the LDS layout, the list of covered positions, that
// epilogue, and the launch geometry; how a kernel streams its token rows through the product is its own (a wave-private DMA queue with
// counted waits on one side; plain loads one group ahead on the other, which also needs a row of u per step).
#pragma once
#include "ctx.h"
#include "mfma_f32_dev.h"

// The workgroup's dynamic LDS.  One definition for both sides: the kernels carve their addresses with P = unsigned char* from smem,
// the launch geometry below takes its byte count with P = size_t from 0 (`end`).
//   mskl [Ncap] u32  the half column mask (this workgroup's 32 segments) of list entry j        Ncap % 4 == 0, > N: entry n, the
//   tokl [Ncap] i32  its token row in Xt                                                        one behind the list, is the zero
//   rnl  [Ncap] f32  its 1 / ||x||                                                              entry out-of-range steps read
//   wl   [Ncap] f32  its weight for the cluster at hand
//   posl [Ncap] i32  (with_pos) its position in the label-grouped order: the row of u
//   part [32][2 nwaves + 1], alpha [32], wcount [16]   the block-norm reduction and the compaction's wave counts
//   queue [nwaves][queue_bytes_per_wave]               a kernel's own staging (16-byte aligned)
template <class P>
struct SvAggLds {
  P mskl, tokl, rnl, wl, posl, part, alpha, wcount, queue, end;
  __host__ __device__ SvAggLds(P base, int Ncap, int nwaves, bool with_pos, int queue_bytes_per_wave) {
    const size_t list = 4 * (size_t)Ncap;
    mskl = base, tokl = mskl + list, rnl = tokl + list, wl = rnl + list, posl = wl + list;
    part = with_pos ? posl + list : posl, alpha = part + 4 * (size_t)(32 * (2 * nwaves + 1)), wcount = alpha + 4 * 32;
    queue = wcount + 4 * 16;
    end = queue + (size_t)nwaves * queue_bytes_per_wave;
  }
};

// The positions (label-grouped order of prep_kernel) of image b that one of the workgroup's 32 segments covers -- half `half` of word
// `sc` of the column masks is not 0 --, ascending, by an ordered ballot compaction: entry by entry the mask, the token row, 1 / ||x||
// and, with POS, the position itself.  Called by the whole workgroup; returns the count n.  The caller writes the zero entry
// (sv_agg_zero_entry) and places the barrier in front of the first read.
template <bool POS>
__device__ __forceinline__ int sv_agg_covered_list(const uint64_t* __restrict__ colmask, const int32_t* __restrict__ tok_order,
                                                   const float* __restrict__ rn_sorted, int b, int N, int SC, int sc, int half,
                                                   uint32_t* mskl, int* tokl, float* rnl, int* posl, int* wcount) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nwaves = blockDim.x >> 6;
  int n = 0;
  for (int base = 0; base < N; base += (int)blockDim.x) {
    const int j = base + tid;
    uint32_t m = 0;
    if (j < N) m = (uint32_t)(colmask[((size_t)b * N + j) * SC + sc] >> (32 * half));
    const uint64_t bal = __builtin_amdgcn_ballot_w64(m != 0);
    if (l == 0) wcount[w] = __popcll(bal);
    __syncthreads();
    int off = n, tot = 0;
    for (int ww = 0; ww < nwaves; ++ww) {
      const int c = wcount[ww];
      if (ww < w) off += c;
      tot += c;
    }
    if (m != 0) {
      const int pos = off + __popcll(bal & ((1ull << l) - 1ull));
      mskl[pos] = m;
      tokl[pos] = tok_order[(size_t)b * N + j];
      rnl[pos] = rn_sorted[(size_t)b * N + j];
      if (POS) posl[pos] = j;
    }
    n += tot;
    __syncthreads();
  }
  return n;
}
// entry n: mask 0, token row 0 (a valid address), 1 / ||x|| = 0.  One thread calls it; its weight is the caller's to zero.
template <bool POS>
__device__ __forceinline__ void sv_agg_zero_entry(int n, uint32_t* mskl, int* tokl, float* rnl, int* posl) {
  mskl[n] = 0;
  tokl[n] = 0;
  rnl[n] = 0.f;
  if (POS) posl[n] = 0;
}

// Cluster k's epilogue, called by the whole workgroup with the product in acc.  Block norms: quad reduce in registers, then across
// lanes / waves through LDS (aggregate_kernel's order: part[row][2 w + half-row], summed c = 0 .. 2 nwaves - 1);
// nrm = nscale sqrt(sum) -- nscale: 1, or K where the accumulators hold V / K (soft_pooled) -- to block_norms[row0 + row][k], and the
// block scaled by nscale / max(nrm, 1e-12) (intra-normalisation; the row's own scale follows in soft_finalize_kernel) to
// out[row0 + row][k][dcol .. dcol + 3].  Sc: the workgroup's segments (<= 32), row0 its first row of out.  Ends on a barrier:
// part / alpha are free for the next cluster.
__device__ __forceinline__ void sv_agg_block_epilogue(const f32x16 (&acc)[4], float* part, float* alpha, int Sc, float nscale, int row0,
                                                      int k, int K, int D, int dcol, bool dvalid, float* __restrict__ out,
                                                      float* __restrict__ block_norms) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, kk = l >> 5;
  const int nwaves = blockDim.x >> 6, PW = nwaves * 2 + 1;
  const size_t KD = (size_t)K * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float p = acc[0][r] * acc[0][r];
    p = fmaf(acc[1][r], acc[1][r], p);
    p = fmaf(acc[2][r], acc[2][r], p);
    p = fmaf(acc[3][r], acc[3][r], p);
    p = sv_dpp_row_sum(p);
    if ((l & 15) == 0) part[sv_frag_row(r, kk) * PW + w * 2 + ((l >> 4) & 1)] = p;
  }
  __syncthreads();
  if (tid < Sc) {
    float sum = 0.f;
    const int cnt = nwaves * 2;
    for (int c = 0; c < cnt; ++c) sum += part[tid * PW + c];
    const float nrm = nscale * sqrtf(sum);
    alpha[tid] = nscale / fmaxf(nrm, 1e-12f);
    block_norms[(size_t)(row0 + tid) * K + k] = nrm;
  }
  __syncthreads();
  if (dvalid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = sv_frag_row(r, kk);
      if (row < Sc) {
        const float a = alpha[row];
        const float4 v = make_float4(acc[0][r] * a, acc[1][r] * a, acc[2][r] * a, acc[3][r] * a);
        *reinterpret_cast<float4*>(out + (size_t)(row0 + row) * KD + (size_t)k * D + dcol) = v;
      }
    }
  }
  __syncthreads();
}

// The launch: grid ((K + kpb - 1) / kpb, B, 2 SC) of 64 ceil(D / 128) threads, the LDS of SvAggLds (fn's limit raised where it passes
// 64 KiB), and the centre operand -- with mean_centre (soft_pooled) every cluster reads that one row (cstride 0) and the norms scale by
// K.  Refuses, under the caller's name, a D beyond 12 waves and an N whose lists pass 160 KiB.
struct SvAggLaunch {
  dim3 grid, block;
  size_t lds;
  int Ncap, kpb, cstride;
  const float* centres;
  float nscale;
};
inline int sv_agg_launch_geometry(segvlad_ctx* ctx, const char* who, const void* fn, bool with_pos, int queue_bytes_per_wave, int K, int D,
                                  int B, int N, int SC, const float* centres, const float* mean_centre, SvAggLaunch* g) {
  const int nwaves = (D + 127) / 128;
  if (nwaves > 12) return ctx->fail(SEGVLAD_ERR_LIMIT, "%s: D=%d exceeds the 1536-wide workgroup of this build", who, D);
  g->Ncap = (N + 4) & ~3;
  g->lds = SvAggLds<size_t>(0, g->Ncap, nwaves, with_pos, queue_bytes_per_wave).end;   // a multiple of 16
  if (g->lds > 160 * 1024) return ctx->fail(SEGVLAD_ERR_LIMIT, "%s: N=%d tokens need %zu B of LDS (limit 160 KiB)", who, N, g->lds);
  if (g->lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(fn, g->lds));
  g->kpb = ctx->opt.agg_kpb < 1 ? 1 : ctx->opt.agg_kpb;   // clusters per workgroup
  g->grid = dim3((K + g->kpb - 1) / g->kpb, B, 2 * SC), g->block = dim3(nwaves * 64);
  g->centres = mean_centre ? mean_centre : centres, g->cstride = mean_centre ? 0 : D, g->nscale = mean_centre ? (float)K : 1.0f;
  return SEGVLAD_OK;
}
