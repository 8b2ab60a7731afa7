// Soft-assignment VLAD (option vlad_assign=soft:<T> | soft_pooled:<T>; utilities.py:862-887, VLAD.generate's vlad_mode='soft').
//
//   soft_centre_mean_kernel soft_pooled alone: the mean centre that stands in for every c_k below
//   soft_weights_kernel     tokens [D][N] -> w[n][0..K) = softmax_k(T <x^_n, c^_k>), max-subtracted, over the K real centres
//   soft_aggregate_kernel   per (image, cluster): V[s][k] = sum_{n in U(s)} w[n][k] (x^_n - c_k) on the fp32 MFMA, ||V[s][k]||,
//                           the intra-normalised block stored packed: the frame of weighted_agg_dev.h around a DMA-queue loop
//   soft_finalize_kernel    per segment: the row scaled to unit length from its K block norms
//
// V is accumulated as sum w (x^ - c), which is sum w x^ - (sum w) c of segvlad.h term for term regrouped: the token's residual is
// formed first and weighted second, as the reference does, so no block is the difference of two large sums.  The [N][K][D] tensor of
// weighted residuals exists one (token pair, cluster, 128-column slice) at a time in the B operand's registers, never in memory.
// Every sum runs in the order of prep_kernel's label-grouped token positions of ONE image: fixed, and independent of the batch.
#include "ctx.h"
#include "assign_dev.h"
#include "weighted_agg_dev.h"

// ------------------------------------------------------------------------------------------------
// weights: workgroup = (image, 64-token tile), wave w owns tokens 32 w .. 32 w + 31 for ALL d: one sequential fp32 chain per score,
// like assign_wide_kernel.  A operand: lane (i, kk) loads T[2 dp + kk][t0 + 32 w + i] (128 contiguous bytes per half-wave);
// B operand: the pre-swizzled normalised centres (vocab_bt_kernel).  The scores of the Kpad - K padded centres are computed (zero
// columns of bt) and never read: the maximum, the sum and the stores run over k < K.
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(128) void soft_weights_kernel(const float* __restrict__ T, int N, int D, int K,
                                                           const float* __restrict__ bt, float temp, float* __restrict__ W) {
  constexpr int KP = NT * 32;
  __shared__ float sc[64 * (KP + 1)];
  __shared__ float ssum[64], smul[64], smax[64], sden[64];
  const int b = blockIdx.y, t0 = blockIdx.x * 64;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int tok = t0 + 32 * w + i;
  const bool valid = tok < N;
  const float* Tb = T + (size_t)b * D * N;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  float ss = 0.f;
  const int npairs = (D + 1) >> 1;
#pragma unroll 8
  for (int dp = 0; dp < npairs; ++dp) {
    const int d = 2 * dp + kk;
    const float x = (valid && d < D) ? Tb[(size_t)d * N + tok] : 0.f;
    ss = fmaf(x, x, ss);
    const float* bp = bt + ((size_t)dp * NT) * 64 + l;
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = MFMA32(x, bp[n * 64], acc[n]);
  }
  SV_SCORE_TILE_STORE(NT, acc, ss, sc, ssum, w, i, kk);
  __syncthreads();
  if (tid < 64) {
    const float rn = 1.0f / fmaxf(sqrtf(ssum[tid]), 1e-12f);
    const float a = fminf(temp * rn, 3.0e38f);   // T / ||x||: the argument is a * (<x, c^_k> - max)
    float best = -INFINITY;
    for (int k = 0; k < K; ++k) best = fmaxf(best, sc[tid * (KP + 1) + k]);
    float den = 0.f;
    for (int k = 0; k < K; ++k) den += expf(a * (sc[tid * (KP + 1) + k] - best));   // k = 0 .. K-1: fixed order
    smul[tid] = a;
    smax[tid] = best;
    sden[tid] = den;
  }
  __syncthreads();
  // the tile's weights are one contiguous run of W: [64 tokens][K]
  const int ntok = min(64, N - t0);
  float* Wt = W + ((size_t)b * N + t0) * K;
  for (int idx = tid; idx < ntok * K; idx += 128) {
    const int tk = idx / K, k = idx - tk * K;
    Wt[idx] = expf(smul[tk] * (sc[tk * (KP + 1) + k] - smax[tk])) / sden[tk];
  }
}

int sv_launch_soft_weights(segvlad_ctx* ctx, const float* tokens, int B, int N, float temp, float* w) {
  const int NT = ctx->Kpad / 32;
  const dim3 grid((N + 63) / 64, B), block(128);
  const float* bt = ctx->vocab_bt.as<float>();
  switch (NT) {
    case 1: hipLaunchKernelGGL(soft_weights_kernel<1>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, temp, w); break;
    case 2: hipLaunchKernelGGL(soft_weights_kernel<2>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, temp, w); break;
    case 4: hipLaunchKernelGGL(soft_weights_kernel<4>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, temp, w); break;
    default: return ctx->fail(SEGVLAD_ERR_LIMIT, "soft weights: K=%d (Kpad in {32,64,128})", ctx->K);
  }
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// soft_pooled: the reference reduces `w * residuals` over tokens AND centres (utilities.py:883-884), so its block k is
//   sum_n w[n][k] sum_c (x^_n - c_c) = K sum_n w[n][k] (x^_n - m),   m = (1/K) sum_c c_c.
// The aggregation below runs unchanged with m in the place of every c_k (cstride 0) and scales the block norm by K.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void soft_centre_mean_kernel(const float* __restrict__ C, int K, int D, float* __restrict__ m) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += C[(size_t)k * D + d];   // k = 0 .. K-1: fixed order
  m[d] = s / (float)K;
}

int sv_launch_soft_centre_mean(segvlad_ctx* ctx, const float* centres, int K, int D, float* mean_centre) {
  hipLaunchKernelGGL(soft_centre_mean_kernel, dim3((D + 255) / 256), dim3(256), 0, ctx->stream, centres, K, D, mean_centre);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// aggregate: the frame of weighted_agg_dev.h (workgroup = (kpb consecutive clusters, image b, 32 segments of it); one M-tile, 16
// accumulator quads less than aggregate_kernel: no spill inside the counted-wait loop).  The workgroup first lists the positions some
// segment of its 32 covers (a token none of them covers is never read), then per cluster k runs the MFMA product
//   (32 segments x 2 tokens) . (2 tokens x 32 d):  A[i][kk] = bit i of the token's half column mask (0/1 exact),
//                                                  B[kk][j] = w[t_kk][k] * fma(Xt[t_kk][d], 1/||x||, -C[k][d])
// with the token rows streaming through a wave-private queue of global->LDS DMAs.
// ------------------------------------------------------------------------------------------------
// one step's operands, a raw LDS read (mfma_f32_dev.h: the counted s_waitcnt in the loop is the only wait): the queue slot (16 B),
// 1 / ||x||, the weight and the half column mask of the lane's token
__device__ __forceinline__ void soft_step_read(unsigned a_slot, unsigned a_rn, unsigned a_w, unsigned a_m, f32x4& x, float& rn, float& wt,
                                               uint32_t& m) {
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b32 %1, %5\n\tds_read_b32 %2, %6\n\tds_read_b32 %3, %7\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(x), "=&v"(rn), "=&v"(wt), "=&v"(m)
               : "v"(a_slot), "v"(a_rn), "v"(a_w), "v"(a_m)
               : "memory");
}

constexpr int SOFT_QD = 6;   // token-pair rows in flight per wave

__global__ __launch_bounds__(768) void soft_aggregate_kernel(const float* __restrict__ Xt, const float* __restrict__ W,
                                                             const float* __restrict__ rn_sorted, const int32_t* __restrict__ tok_order,
                                                             const uint64_t* __restrict__ colmask, const float* __restrict__ C,
                                                             const int32_t* __restrict__ seg_off, int N, int D, int K, int SC, int Ncap,
                                                             float* __restrict__ out, float* __restrict__ block_norms, int kpb,
                                                             int cstride, float nscale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const SvAggLds<unsigned char*> L(smem, Ncap, blockDim.x >> 6, false, SOFT_QD * 1024);
  uint32_t* mskl = reinterpret_cast<uint32_t*>(L.mskl);
  int* tokl = reinterpret_cast<int*>(L.tokl);
  float* rnl = reinterpret_cast<float*>(L.rnl);
  float* wl = reinterpret_cast<float*>(L.wl);
  unsigned char* xq = L.queue;   // [nwaves][SOFT_QD][1 KiB] DMA queue

  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  const int r0 = 32 * (int)blockIdx.z;   // first segment of this workgroup inside the image
  if (r0 >= S) return;
  const int Sc = min(32, S - r0);
  const int sc = r0 >> 6, half = (r0 >> 5) & 1;
  const int dcol = w * 128 + 4 * i;
  const bool dvalid = dcol < D;
  const float* Xb = Xt + (size_t)b * N * D + dcol;
  const int k_begin = (int)blockIdx.x * kpb, k_end = min(K, k_begin + kpb);

  const int n = sv_agg_covered_list<false>(colmask, tok_order, rn_sorted, b, N, SC, sc, half, mskl, tokl, rnl, nullptr, reinterpret_cast<int*>(L.wcount));
  if (tid == 0 && (n & 1)) sv_agg_zero_entry<false>(n, mskl, tokl, rnl, nullptr);   // pad to an even count with a zero-weight entry
  __syncthreads();
  const int npairs = (n + 1) >> 1;
  unsigned char* qbase = xq + (size_t)__builtin_amdgcn_readfirstlane(w) * (SOFT_QD * 1024);   // wave-uniform: lives in M0

  for (int k = k_begin; k < k_end; ++k) {
    for (int j = tid; j < n; j += blockDim.x) wl[j] = W[((size_t)b * N + tokl[j]) * K + k];
    if (tid == 0 && (n & 1)) wl[n] = 0.f;
    float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (dvalid) c4 = *reinterpret_cast<const float4*>(C + (size_t)k * cstride + dcol);   // (cstride 0: the mean centre, whatever k)
    __syncthreads();
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    {
      auto issue = [&](int p) {
        const int t = sv_lds_read_i32(sv_lds_addr(tokl + 2 * p + kk));
        // lanes beyond D (a partial last wave) fetch a valid dummy address: their 16 B are never used
        const float* src = dvalid ? Xb + (size_t)t * D : Xt;
        __builtin_amdgcn_global_load_lds((sv_gptr_t)src, (sv_lptr_t)(qbase + (p % SOFT_QD) * 1024), 16, 0, 0);
      };
      for (int q = 0; q < SOFT_QD && q < npairs; ++q) issue(q);
      for (int p = 0; p < npairs; ++p) {
        const int j = 2 * p + kk;
        sv_wait_queue<SOFT_QD>(npairs - 1 - p);   // (the DMAs issued after pair p's)
        f32x4 x;
        float rn, wt;
        uint32_t m;
        soft_step_read(sv_lds_addr(qbase + (p % SOFT_QD) * 1024 + l * 16), sv_lds_addr(rnl + j), sv_lds_addr(wl + j),
                       sv_lds_addr(mskl + j), x, rn, wt, m);
        // (the slot has been read -- lgkmcnt(0) inside -- before it is refilled)
        if (p + SOFT_QD < npairs) issue(p + SOFT_QD);
        if (!dvalid) x = f32x4{0.f, 0.f, 0.f, 0.f};
        const float b0 = wt * fmaf(x.x, rn, -c4.x), b1 = wt * fmaf(x.y, rn, -c4.y);
        const float b2 = wt * fmaf(x.z, rn, -c4.z), b3 = wt * fmaf(x.w, rn, -c4.w);
        const float a0 = ((m >> i) & 1u) ? 1.f : 0.f;
        acc[0] = MFMA32(a0, b0, acc[0]);
        acc[1] = MFMA32(a0, b1, acc[1]);
        acc[2] = MFMA32(a0, b2, acc[2]);
        acc[3] = MFMA32(a0, b3, acc[3]);
      }
    }
    sv_agg_block_epilogue(acc, reinterpret_cast<float*>(L.part), reinterpret_cast<float*>(L.alpha), Sc, nscale, s0 + r0, k, K, D, dcol, dvalid, out,
                          block_norms);
  }
}

int sv_launch_soft_aggregate(segvlad_ctx* ctx, const float* xt, const float* w, const uint64_t* colmask, const float* centres, int K, int D,
                             const int32_t* seg_off_dev, int B, int N, int SC, float* out, float* block_norms, const float* mean_centre) {
  SvAggLaunch g;
  const int rc = sv_agg_launch_geometry(ctx, "soft aggregate", reinterpret_cast<const void*>(soft_aggregate_kernel), false, SOFT_QD * 1024,
                                        K, D, B, N, SC, centres, mean_centre, &g);
  if (rc != SEGVLAD_OK) return rc;
  hipLaunchKernelGGL(soft_aggregate_kernel, g.grid, g.block, g.lds, ctx->stream, xt, w, ctx->s_rnsorted.as<float>(),
                     ctx->s_tokorder.as<int32_t>(), colmask, g.centres, seg_off_dev, N, D, K, SC, g.Ncap, out, block_norms, g.kpb, g.cstride,
                     g.nscale);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// finalize: out[s] = concat_k(block) / max(|| concat_k(block) ||, 1e-12).  A stored block has norm r_k = ||V|| / max(||V||, 1e-12)
// (exactly 1 unless ||V|| < 1e-12), so the row's norm is sqrt(sum_k r_k^2), summed k = 0 .. K-1: sqrt(#non-empty blocks) where the hard
// path's gscale counts them.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void soft_finalize_kernel(const float* __restrict__ block_norms, int K, int D, float* __restrict__ out) {
  __shared__ float g;
  const int s = blockIdx.x;
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const float nrm = block_norms[(size_t)s * K + k];
      const float r = nrm / fmaxf(nrm, 1e-12f);
      acc = fmaf(r, r, acc);
    }
    g = 1.0f / fmaxf(sqrtf(acc), 1e-12f);
  }
  __syncthreads();
  const float a = g;
  float4* row = reinterpret_cast<float4*>(out + (size_t)s * K * D);   // (D % 4 == 0: segvlad_set_vocab)
  const int n4 = K * D / 4;
  for (int j = threadIdx.x; j < n4; j += 256) {
    float4 v = row[j];
    v.x *= a, v.y *= a, v.z *= a, v.w *= a;
    row[j] = v;
  }
}

int sv_launch_soft_finalize(segvlad_ctx* ctx, const float* block_norms, int S_tot, int K, int D, float* out) {
  hipLaunchKernelGGL(soft_finalize_kernel, dim3(S_tot), dim3(256), 0, ctx->stream, block_norms, K, D, out);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
