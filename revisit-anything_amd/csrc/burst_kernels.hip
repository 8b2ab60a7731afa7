// Burst-discounted VLAD (option vlad_burst=<a>:<b>:<p>, include/segvlad.h): every token's assignment weight is divided by a soft count
// of the tokens of ITS image that look like it,
//   g[n] = sum_{m < N} sigmoid(a (2 <x^_n, x^_m> - 2) + b),      u[n] = g[n]^-p,      w[n][k] <- w[n][k] u[n].
//
//   burst_gram_kernel    one 128 x 128 tile of an image's N x N self-similarity on the fp32 MFMA (sv_gram_tile, gram_tile_dev.h, which
//                        the segment scope of burst_seg_kernels.hip runs too); the sigmoid and the row (and, off the
//                        diagonal, column) sums in the epilogue; the matrix itself never exists outside the accumulators
//   burst_finish_kernel  g = the tile sums added in tile order, u = g^-p, and the weights the soft aggregation reads: the one-hot of the
//                        labels times u (hard assignment), or the rows of soft_weights_kernel's w scaled by u
//
// The Gram matrix is symmetric: only the tiles (I, J) with I <= J run.  A tile's row sums go to part[b][J][rows of I]; an off-diagonal
// tile's column sums go to part[b][I][columns of J].  Slot (t, n) with n in tile row R is therefore written by tile (R, t)'s row sums
// when t >= R and by tile (t, R)'s column sums when t < R: every slot exactly once, no atomics, and burst_finish_kernel's sum over
// t = 0 .. T-1 has one fixed order whatever the batch holds.
#include "ctx.h"
#include "gram_tile_dev.h"

// Operands: both from the token-major copy Xt [B][N][D] (raw tokens; the cosine is the dot product times the two 1 / ||x|| in the
// epilogue), multiplied by sv_gram_tile (gram_tile_dev.h) with the positions themselves as rows.  Rows / columns beyond N are masked
// out of the sums (a padded column is not zero: it would add sigmoid(b - 2 a)).
__global__ __launch_bounds__(256) void burst_gram_kernel(const float* __restrict__ Xt, const float* __restrict__ rnorm, int B, int N, int D,
                                                         int T, int by_xcd, float a, float bb, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sA[SV_GRAM_TILE * SV_GRAM_LD];
  __shared__ __attribute__((aligned(16))) float sB[SV_GRAM_TILE * SV_GRAM_LD];
  __shared__ float rowp[2][SV_GRAM_TILE], colp[2][SV_GRAM_TILE];
  const int TP = T * (T + 1) / 2;
  int img, t;
  sv_gram_deal(by_xcd, TP, img, t);
  if (img >= B) return;
  int I = 0;
  while (t >= T - I) t -= T - I, ++I;
  const int J = I + t;
  const int n0 = I * SV_GRAM_TILE, m0 = J * SV_GRAM_TILE;

  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int wr = w >> 1, wc = w & 1;
  int ra[4], rb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (tid >> 3) + 32 * j;
    ra[j] = n0 + r < N ? n0 + r : -1;
    rb[j] = m0 + r < N ? m0 + r : -1;
  }
  f32x16 acc[2][2];
  sv_gram_tile(Xt + (size_t)img * N * D, ra, rb, D, sA, sB, acc);

  // ---- epilogue: sigmoid(a (2 cos - 2) + b), masked; row sums over the wave's 64 columns, column sums over its 64 rows ----
  float rn_col[2];
  bool ok_col[2];
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int m = m0 + 64 * wc + 32 * tj + i;
    ok_col[tj] = m < N;
    rn_col[tj] = ok_col[tj] ? rnorm[(size_t)img * N + m] : 0.f;
  }
  float csum[2] = {0.f, 0.f};
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 64 * wr + 32 * ti + sv_frag_row(r, kk);
      const int n = n0 + row;
      const bool ok_row = n < N;
      const float rn_row = ok_row ? rnorm[(size_t)img * N + n] : 0.f;
      float rsum = 0.f;
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const float cosv = acc[ti][tj][r] * rn_row * rn_col[tj];
        const float z = fmaf(a, fmaf(2.f, cosv, -2.f), bb);
        const float s = (ok_row && ok_col[tj]) ? 1.0f / (1.0f + expf(-z)) : 0.f;
        rsum += s;
        csum[tj] += s;
      }
      // over the 32 lanes of this half (the columns i): xor steps stay inside the half
      rsum += __shfl_xor(rsum, 16);
      rsum += __shfl_xor(rsum, 8);
      rsum += __shfl_xor(rsum, 4);
      rsum += __shfl_xor(rsum, 2);
      rsum += __shfl_xor(rsum, 1);
      if (i == 0) rowp[wc][row] = rsum;
    }
  }
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const float c = csum[tj] + __shfl_xor(csum[tj], 32);
    if (kk == 0) colp[wr][64 * wc + 32 * tj + i] = c;
  }
  __syncthreads();
  if (tid < SV_GRAM_TILE) {
    if (n0 + tid < N) part[((size_t)img * T + J) * N + n0 + tid] = rowp[0][tid] + rowp[1][tid];
  } else if (I != J) {
    const int c = tid - SV_GRAM_TILE;
    if (m0 + c < N) part[((size_t)img * T + I) * N + m0 + c] = colp[0][c] + colp[1][c];
  }
}

int sv_burst_tiles(int N) { return (N + SV_GRAM_TILE - 1) / SV_GRAM_TILE; }

int sv_launch_burst_gram(segvlad_ctx* ctx, const float* xt, const float* rnorm, int B, int N, int D, float a, float b, float* part) {
  const int T = sv_burst_tiles(N), TP = T * (T + 1) / 2;
  const long long nwg = sv_gram_grid(B, TP);
  if (nwg > 0x7fffffffll) return ctx->fail(SEGVLAD_ERR_LIMIT, "burst: B=%d N=%d give %lld tiles", B, N, nwg);
  hipLaunchKernelGGL(burst_gram_kernel, dim3((unsigned)nwg), dim3(256), 0, ctx->stream, xt, rnorm, B, N, D, T, sv_gram_by_xcd(B), a, b, part);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// workgroup = (64-token tile, image): u for the tile's tokens, then the tile's weights, one contiguous run of W: [64 tokens][K]
__global__ __launch_bounds__(256) void burst_finish_kernel(const float* __restrict__ part, const uint8_t* __restrict__ labels, int N, int K,
                                                           int T, float p, int one_hot, float* __restrict__ W) {
  __shared__ float su[64];
  __shared__ int slab[64];
  const int b = blockIdx.y, t0 = blockIdx.x * 64, tid = threadIdx.x;
  const int ntok = min(64, N - t0);
  if (tid < ntok) {
    const int n = t0 + tid;
    float g = 0.f;
    for (int t = 0; t < T; ++t) g += part[((size_t)b * T + t) * N + n];   // t = 0 .. T-1: fixed order
    su[tid] = sv_burst_discount(g, p);
    slab[tid] = one_hot ? (int)labels[(size_t)b * N + n] : 0;
  }
  __syncthreads();
  float* Wt = W + ((size_t)b * N + t0) * K;
  for (int idx = tid; idx < ntok * K; idx += 256) {
    const int tk = idx / K, k = idx - tk * K;
    Wt[idx] = one_hot ? (k == slab[tk] ? su[tk] : 0.f) : Wt[idx] * su[tk];
  }
}

int sv_launch_burst_finish(segvlad_ctx* ctx, const float* part, const uint8_t* labels, int B, int N, int K, float p, bool one_hot, float* w) {
  hipLaunchKernelGGL(burst_finish_kernel, dim3((N + 63) / 64, B), dim3(256), 0, ctx->stream, part, labels, N, K, sv_burst_tiles(N), p,
                     one_hot ? 1 : 0, w);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
