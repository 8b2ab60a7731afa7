// Burst discount over a segment's own tokens (options vlad_burst=<a>:<b>:<p> with vlad_burst_scope=segment, include/segvlad.h): the
// weight of token n in segment s is divided by a soft count of the tokens of U(s) -- the segment's tokens after the neighbour union --
// that look like it,
//   g[s][n] = sum_{m in U(s)} sigmoid(a (2 <x^_n, x^_m> - 2) + b),      u[s][n] = g[s][n]^-p,      V[s][k] = sum_{n in U(s)} u[s][n] w[n][k] (x^_n - c_k).
//
//   burst_seg_gram_kernel        per (image, 128 tokens n, 64 segments): walks the 128 x 128 tiles of the self-similarity (sv_gram_tile,
//                                gram_tile_dev.h) down the image's tokens m on the fp32 MFMA, turns every tile into its sigmoid in the accumulators and feeds
//                                them, as they lie, to a second MFMA product with the 0/1 tile of the column masks; u = g^-p on the
//                                bits of U(s), 0 elsewhere, written once
//   burst_seg_aggregate_kernel   the aggregation frame of weighted_agg_dev.h with the A operand bit ? u[s][t] : 0 and a plain-load loop;
//                                under hard assignment cluster k walks label k's positions only, with weight 1
//
// Tokens are addressed by their POSITION in prep_kernel's label-grouped order throughout (the column masks, the sorted 1 / ||x|| and the
// rows of u are indexed by it): every sum runs in that order of ONE image, fixed, whatever the batch or the other segments hold.  An MFMA
// step is a k-ordered fmaf chain, a term with a zero mask bit adds an exact 0: g[s][n] is the chain over the tokens of U(s) alone.
#include "ctx.h"
#include "gram_tile_dev.h"
#include "weighted_agg_dev.h"

constexpr int BS_GLD = 65;     // row stride of the [128 tokens][64 segments] image of g in LDS

// ------------------------------------------------------------------------------------------------
// gram: workgroup = (image, column tile J, chunk of 64 segments).  It owns the 128 tokens n of tile J and walks the row tiles
// I = 0 .. T-1 (tokens m).  Tile (I, J) is sv_gram_tile's product (gram_tile_dev.h) with the tok_order entries of the positions as
// rows: rows m on the A side, columns n on the B side, the cosine = the raw dot product times the two 1 / ||x||.  In the C/D layout
// lane (i, kk) holds column i and the 16 rows sv_frag_row(r, kk); the matrix being symmetric that is the A operand of the product whose
// output rows are the tile's columns and whose contraction runs over its rows:
//   A[i][kk] = sigmoid tile[row(r, kk)][column i] = acc[r],      B[kk][j] = bit j of the column mask of the token in row(r, kk)
// so the accumulators feed the second product with no trip through LDS, and neither the Gram matrix nor its sigmoid reaches memory.
// A wave contracts over its own 64 rows of every tile; the two waves of a column half add their sums at the end, wr = 0 first: one
// fixed order, no atomics.  Rows beyond N have a zero mask, columns beyond N are not stored (a padded entry is sigmoid(b - 2 a), not 0).
// The full square runs: twice burst_gram_kernel's flops (the symmetric half would need the transposed tile as an operand too).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void burst_seg_gram_kernel(const float* __restrict__ Xt, const float* __restrict__ rn_sorted,
                                                             const int32_t* __restrict__ tok_order, const uint64_t* __restrict__ colmask,
                                                             const int32_t* __restrict__ seg_off, int B, int N, int D, int T, int SC,
                                                             int by_xcd, float a, float bb, float p, float* __restrict__ U) {
  __shared__ __attribute__((aligned(16))) float sAB[2 * SV_GRAM_TILE * SV_GRAM_LD];   // the two operand chunks; at the end the image of g
  __shared__ uint64_t smask[SV_GRAM_TILE];
  __shared__ float srn[SV_GRAM_TILE];
  float* sA = sAB;
  float* sB = sAB + SV_GRAM_TILE * SV_GRAM_LD;
  int img, t;
  sv_gram_deal(by_xcd, T * SC, img, t);
  if (img >= B) return;
  const int chunk = t / T, J = t % T;
  if (64 * chunk >= seg_off[img + 1] - seg_off[img]) return;   // no segment of the image in this chunk: nothing reads its columns
  const int n0 = J * SV_GRAM_TILE;

  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int wr = w >> 1, wc = w & 1;
  const float* Xb = Xt + (size_t)img * N * D;
  const int32_t* ord = tok_order + (size_t)img * N;
  const float* rns = rn_sorted + (size_t)img * N;
  const uint64_t* cm = colmask + (size_t)img * N * SC + chunk;
  const int lr = tid >> 3;   // this thread's first row of a tile's operand chunk (then + 32, 64, 96)

  int tb[4];   // the token rows of Xt behind this thread's four columns n (-1: beyond N)
#pragma unroll
  for (int j = 0; j < 4; ++j) tb[j] = n0 + lr + 32 * j < N ? ord[n0 + lr + 32 * j] : -1;
  float rn_col[2];
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int n = n0 + 64 * wc + 32 * tj + i;
    rn_col[tj] = n < N ? rns[n] : 0.f;
  }
  f32x16 gacc[2][2];   // [column subtile tj][segment half sj]: rows = the tile's columns n, columns = segments
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj)
#pragma unroll
      for (int r = 0; r < 16; ++r) gacc[tj][sj][r] = 0.f;

  for (int I = 0; I < T; ++I) {
    const int m0 = I * SV_GRAM_TILE;
    if (tid < SV_GRAM_TILE) {
      const bool ok = m0 + tid < N;
      smask[tid] = ok ? cm[(size_t)(m0 + tid) * SC] : 0ull;
      srn[tid] = ok ? rns[m0 + tid] : 0.f;
    }
    int ta[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ta[j] = m0 + lr + 32 * j < N ? ord[m0 + lr + 32 * j] : -1;
    f32x16 acc[2][2];
    sv_gram_tile(Xb, ta, tb, D, sA, sB, acc);

    // ---- the tile's sigmoid, register by register, straight into the mask product: rows (m) are the contraction ----
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 64 * wr + 32 * ti + sv_frag_row(r, kk);
        const float rn_row = srn[row];
        const uint64_t mk = smask[row];   // 0 beyond N: such a row adds an exact 0 (its sigmoid is finite)
        const float m_lo = ((mk >> i) & 1ull) ? 1.f : 0.f, m_hi = ((mk >> (32 + i)) & 1ull) ? 1.f : 0.f;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          const float cosv = acc[ti][tj][r] * rn_row * rn_col[tj];
          const float z = fmaf(a, fmaf(2.f, cosv, -2.f), bb);
          const float s = 1.0f / (1.0f + expf(-z));
          gacc[tj][0] = MFMA32(s, m_lo, gacc[tj][0]);
          gacc[tj][1] = MFMA32(s, m_hi, gacc[tj][1]);
        }
      }
    }
    __syncthreads();   // smask / srn are rewritten by the next row tile
  }

  // ---- g = the sums of the column half's two waves, wr = 0 + wr = 1; u = g^-p on the bits ----
  float* sg = sAB;   // [128][BS_GLD] (8320 floats of the 9216)
#pragma unroll
  for (int pass = 1; pass >= 0; --pass) {
    if (wr == pass) {
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int sj = 0; sj < 2; ++sj)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* dst = sg + (64 * wc + 32 * tj + sv_frag_row(r, kk)) * BS_GLD + 32 * sj + i;
            *dst = pass ? gacc[tj][sj][r] : gacc[tj][sj][r] + *dst;
          }
    }
    __syncthreads();
  }
  const int ldu = 64 * SC;
  for (int idx = tid; idx < SV_GRAM_TILE * 64; idx += 256) {
    const int c = idx >> 6, s = idx & 63, n = n0 + c;
    if (n >= N) break;   // (c grows with idx)
    const float g = sg[c * BS_GLD + s];
    const bool bit = (cm[(size_t)n * SC] >> s) & 1ull;
    U[((size_t)img * N + n) * ldu + 64 * chunk + s] = bit ? sv_burst_discount(g, p) : 0.f;
  }
}

int sv_launch_burst_seg_gram(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const int32_t* seg_off_dev, int B, int N, int D,
                             int SC, float a, float b, float p, float* u) {
  const int T = sv_burst_tiles(N);
  const long long nwg = sv_gram_grid(B, (long long)T * SC);
  if (nwg > 0x7fffffffll) return ctx->fail(SEGVLAD_ERR_LIMIT, "burst (segment scope): B=%d N=%d SC=%d give %lld workgroups", B, N, SC, nwg);
  hipLaunchKernelGGL(burst_seg_gram_kernel, dim3((unsigned)nwg), dim3(256), 0, ctx->stream, xt, ctx->s_rnsorted.as<float>(),
                     ctx->s_tokorder.as<int32_t>(), colmask, seg_off_dev, B, N, D, T, SC, sv_gram_by_xcd(B), a, b, p, u);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// aggregate: the frame of weighted_agg_dev.h (workgroup = (kpb consecutive clusters, image b, 32 segments of it); wave w owns d in
// [128 w, 128 w + 128)).  Per cluster k the MFMA product
//   (32 segments x 2 tokens) . (2 tokens x 32 d):  A[i][kk] = bit i of the position's half column mask ? u[position][segment i] : 0
//                                                  B[kk][j] = w[t_kk][k] * fma(Xt[t_kk][d], 1/||x||, -C[k][d])
// HARD: the list is every position of the image and cluster k walks [lab_off[k], lab_off[k + 1]) with w = 1 -- the hard aggregation's
// walk, so its matrix work.  Otherwise the list is the positions one of the 32 segments covers (sv_agg_covered_list)
// and every cluster walks all of it with W's column k.  The token rows and the rows of u are plain loads, one group of BS_G token pairs
// ahead of the MFMAs that use them.
// ------------------------------------------------------------------------------------------------
constexpr int BS_G = 2;   // token pairs per software-pipeline group (4 spills registers at 768 threads)

template <bool HARD>
__global__ __launch_bounds__(768) void burst_seg_aggregate_kernel(const float* __restrict__ Xt, const float* __restrict__ W,
                                                                  const float* __restrict__ U, const float* __restrict__ rn_sorted,
                                                                  const int32_t* __restrict__ tok_order, const int32_t* __restrict__ lab_off,
                                                                  const uint64_t* __restrict__ colmask, const float* __restrict__ C,
                                                                  const int32_t* __restrict__ seg_off, int N, int D, int K, int SC, int Ncap,
                                                                  float* __restrict__ out, float* __restrict__ block_norms, int kpb,
                                                                  int cstride, float nscale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const SvAggLds<unsigned char*> L(smem, Ncap, blockDim.x >> 6, true, 0);
  uint32_t* mskl = reinterpret_cast<uint32_t*>(L.mskl);
  int* tokl = reinterpret_cast<int*>(L.tokl);
  float* rnl = reinterpret_cast<float*>(L.rnl);
  float* wl = reinterpret_cast<float*>(L.wl);       // (!HARD)
  int* posl = reinterpret_cast<int*>(L.posl);       // (!HARD: the position behind a list entry)

  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  const int r0 = 32 * (int)blockIdx.z;   // first segment of this workgroup inside the image
  if (r0 >= S) return;
  const int Sc = min(32, S - r0);
  const int sc = r0 >> 6, half = (r0 >> 5) & 1;
  const int dcol = w * 128 + 4 * i;
  const bool dvalid = dcol < D;
  const float* Xb = Xt + (size_t)b * N * D + dcol;
  const int ldu = 64 * SC;
  const float* Ub = U + (size_t)b * N * ldu + r0 + i;   // this lane's segment column of u
  const int k_begin = (int)blockIdx.x * kpb, k_end = min(K, k_begin + kpb);

  // ---- the list: entry n is the zero entry every out-of-range step reads ----
  int n = 0;
  if (HARD) {
    for (int j = tid; j < N; j += (int)blockDim.x) {
      mskl[j] = (uint32_t)(colmask[((size_t)b * N + j) * SC + sc] >> (32 * half));
      tokl[j] = tok_order[(size_t)b * N + j];
      rnl[j] = rn_sorted[(size_t)b * N + j];
    }
    n = N;
  } else {
    n = sv_agg_covered_list<true>(colmask, tok_order, rn_sorted, b, N, SC, sc, half, mskl, tokl, rnl, posl, reinterpret_cast<int*>(L.wcount));
  }
  if (tid == 0) {
    sv_agg_zero_entry<true>(n, mskl, tokl, rnl, posl);
    wl[n] = 0.f;
  }
  __syncthreads();

  for (int k = k_begin; k < k_end; ++k) {
    int lo = 0, hi = n;
    if (HARD) {
      lo = lab_off[(size_t)b * (K + 1) + k], hi = lab_off[(size_t)b * (K + 1) + k + 1];
    } else {
      for (int j = tid; j < n; j += (int)blockDim.x) wl[j] = W[((size_t)b * N + tokl[j]) * K + k];
    }
    const int npairs = (hi - lo + 1) >> 1;
    float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (dvalid) c4 = *reinterpret_cast<const float4*>(C + (size_t)k * cstride + dcol);   // (cstride 0: the mean centre, whatever k)
    __syncthreads();
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    // one step's operands: the token row's 16 bytes, its 1 / ||x|| and weight, and this lane's u (0 where its segment's bit is off)
    auto load = [&](int pr, f32x4& x, float& rn, float& wt, float& av) {
      const int j = lo + 2 * pr + kk;
      const int jj = (pr < npairs && j < hi) ? j : n;
      const uint32_t m = mskl[jj];
      rn = rnl[jj];
      wt = HARD ? 1.f : wl[jj];
      x = f32x4{0.f, 0.f, 0.f, 0.f};
      if (dvalid) x = *reinterpret_cast<const f32x4*>(Xb + (size_t)tokl[jj] * D);
      av = 0.f;
      if ((m >> i) & 1u) av = Ub[(size_t)(HARD ? jj : posl[jj]) * ldu];
    };
    f32x4 x[BS_G], xn[BS_G];
    float rn[BS_G], wt[BS_G], av[BS_G], rnn[BS_G], wtn[BS_G], avn[BS_G];
#pragma unroll
    for (int g = 0; g < BS_G; ++g) load(g, x[g], rn[g], wt[g], av[g]);
    for (int p0 = 0; p0 < npairs; p0 += BS_G) {
#pragma unroll
      for (int g = 0; g < BS_G; ++g) load(p0 + BS_G + g, xn[g], rnn[g], wtn[g], avn[g]);   // (beyond the range: the zero entry)
#pragma unroll
      for (int g = 0; g < BS_G; ++g) {
        if (p0 + g < npairs) {
          const float b0 = wt[g] * fmaf(x[g].x, rn[g], -c4.x), b1 = wt[g] * fmaf(x[g].y, rn[g], -c4.y);
          const float b2 = wt[g] * fmaf(x[g].z, rn[g], -c4.z), b3 = wt[g] * fmaf(x[g].w, rn[g], -c4.w);
          acc[0] = MFMA32(av[g], b0, acc[0]);
          acc[1] = MFMA32(av[g], b1, acc[1]);
          acc[2] = MFMA32(av[g], b2, acc[2]);
          acc[3] = MFMA32(av[g], b3, acc[3]);
        }
      }
#pragma unroll
      for (int g = 0; g < BS_G; ++g) x[g] = xn[g], rn[g] = rnn[g], wt[g] = wtn[g], av[g] = avn[g];
    }
    sv_agg_block_epilogue(acc, reinterpret_cast<float*>(L.part), reinterpret_cast<float*>(L.alpha), Sc, nscale, s0 + r0, k, K, D, dcol, dvalid, out,
                          block_norms);
  }
}

int sv_launch_burst_seg_aggregate(segvlad_ctx* ctx, const float* xt, const float* w, const float* u, const uint64_t* colmask,
                                  const float* centres, int K, int D, const int32_t* seg_off_dev, int B, int N, int SC, float* out,
                                  float* block_norms, const float* mean_centre) {
  const void* fn = w ? reinterpret_cast<const void*>(burst_seg_aggregate_kernel<false>) : reinterpret_cast<const void*>(burst_seg_aggregate_kernel<true>);
  SvAggLaunch g;
  const int rc = sv_agg_launch_geometry(ctx, "burst aggregate", fn, true, 0, K, D, B, N, SC, centres, mean_centre, &g);
  if (rc != SEGVLAD_OK) return rc;
  if (w)
    hipLaunchKernelGGL(burst_seg_aggregate_kernel<false>, g.grid, g.block, g.lds, ctx->stream, xt, w, u, ctx->s_rnsorted.as<float>(),
                       ctx->s_tokorder.as<int32_t>(), ctx->s_laboff.as<int32_t>(), colmask, g.centres, seg_off_dev, N, D, K, SC, g.Ncap, out,
                       block_norms, g.kpb, g.cstride, g.nscale);
  else
    hipLaunchKernelGGL(burst_seg_aggregate_kernel<true>, g.grid, g.block, g.lds, ctx->stream, xt, w, u, ctx->s_rnsorted.as<float>(),
                       ctx->s_tokorder.as<int32_t>(), ctx->s_laboff.as<int32_t>(), colmask, g.centres, seg_off_dev, N, D, K, SC, g.Ncap, out,
                       block_norms, g.kpb, g.cstride, g.nscale);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
