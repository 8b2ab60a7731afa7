// Vocabulary preparation and hard assignment of the describe stage, for gfx950 (MI355X).
//
//   vocab_norm_kernel   1 / max(||C_k||, 1e-12) of every centre
//   vocab_bt_kernel     the normalised centres in the order the MFMA B operand loads them (256 contiguous bytes per wave-load)
//   assign_wide_kernel  tokens [D][N] -> labels (first maximum of <x, c^_k>), 1/||x||, top-2 gap, and the token-major copy Xt [N][D]
//                       that the aggregations stream: 128-token tiles, 16-byte loads two chunks ahead, one sequential fp32 chain
//                       per score.  The default for K <= 64 and D % 32 == 0                       (func_vpr.py:1085,1145-1146)
//   assign_kernel       the same outputs from 64-token tiles whose four waves split D and combine their partial scores in LDS
//                       (a different summation order: different bits in the last place): every other shape, and assign_narrow=1
//
// Wave = 64 lanes.  The scores run on v_mfma_f32_32x32x2_f32 (exact fp32 fma chain); the score tile's store and the pick of a token's
// label are assign_dev.h's, shared with soft_weights_kernel (soft_vlad_kernels.hip), which reads vocab_bt_kernel's operand as well.
#include "ctx.h"
#include "assign_dev.h"

// ------------------------------------------------------------------------------------------------
// vocabulary: c^ = C / max(||C||, 1e-12), stored in MFMA B-operand order
//   bt[((dp * NT) + nt) * 64 + l] = c^[32 nt + (l & 31)][2 dp + (l >> 5)]   (0 outside K x D)
// ------------------------------------------------------------------------------------------------
__global__ void vocab_norm_kernel(const float* __restrict__ C, int K, int D, float* __restrict__ inv) {
  const int k = blockIdx.x;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float v = C[(size_t)k * D + d];
    s = fmaf(v, v, s);
  }
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) inv[k] = 1.0f / fmaxf(sqrtf(red[0]), 1e-12f);
}

__global__ void vocab_bt_kernel(const float* __restrict__ C, const float* __restrict__ inv, int K, int D, int NT,
                                int npairs, float* __restrict__ bt) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)npairs * NT * 64;
  if (idx >= total) return;
  const int l = idx & 63;
  const int nt = (idx >> 6) % NT;
  const int dp = (idx >> 6) / NT;
  const int k = 32 * nt + (l & 31), d = 2 * dp + (l >> 5);
  bt[idx] = (k < K && d < D) ? C[(size_t)k * D + d] * inv[k] : 0.f;
}

int sv_launch_vocab_prepare(segvlad_ctx* ctx) {
  const int K = ctx->K, D = ctx->D, NT = ctx->Kpad / 32;
  const int npairs = ((D + 63) / 64) * 32;
  SV_HIP(ctx->vocab_bt.reserve((size_t)npairs * NT * 64 * sizeof(float)));
  SV_HIP(ctx->s_misc.reserve((size_t)K * sizeof(float)));
  hipLaunchKernelGGL(vocab_norm_kernel, dim3(K), dim3(256), 0, ctx->stream, ctx->vocab.as<float>(), K, D,
                     ctx->s_misc.as<float>());
  const size_t total = (size_t)npairs * NT * 64;
  hipLaunchKernelGGL(vocab_bt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->vocab.as<float>(), ctx->s_misc.as<float>(), K, D, NT, npairs, ctx->vocab_bt.as<float>());
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// assign: workgroup = (image, 64-token tile), 4 waves split D in 64-wide chunks.
//   A operand  (32 tokens x 2 d):  lane (i = l&31, kk = l>>5) loads T[d0+kk][t0+2i .. 2i+1]  (8 B/lane,
//              256 B contiguous per half-wave) -> M-tile 0 = even tokens, M-tile 1 = odd tokens
//   B operand  (2 d x 32 centres): pre-swizzled bt, 256 B contiguous per wave-load
// The raw values are also staged through a wave-private LDS tile and written token-major (Xt).
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ T, int N, int D, int K,
                                                     const float* __restrict__ bt, float* __restrict__ Xt,
                                                     uint8_t* __restrict__ labels, float* __restrict__ rnorm,
                                                     float* __restrict__ gap) {
  __shared__ float lds[4 * 64 * 65];
  const int b = blockIdx.y, t0 = blockIdx.x * 64;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const float* Tb = T + (size_t)b * D * N;
  float* tile = lds + w * (64 * 65);
  f32x16 acc[2][NT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][n][r] = 0.f;
  float ss0 = 0.f, ss1 = 0.f;
  const int ta = t0 + 2 * i;
  const bool v0 = ta < N, v1 = ta + 1 < N;
  const bool evenN = (N & 1) == 0;
  const int nchunks = (D + 63) >> 6;
  for (int ch = w; ch < nchunks; ch += 4) {
    const int dbase = ch << 6;
#pragma unroll 8
    for (int st = 0; st < 32; ++st) {
      const int d = dbase + 2 * st + kk;
      float x0 = 0.f, x1 = 0.f;
      if (d < D) {
        const float* p = Tb + (size_t)d * N + ta;
        if (v1 && evenN) {
          const float2 v = *reinterpret_cast<const float2*>(p);
          x0 = v.x;
          x1 = v.y;
        } else {
          if (v0) x0 = p[0];
          if (v1) x1 = p[1];
        }
      }
      ss0 = fmaf(x0, x0, ss0);
      ss1 = fmaf(x1, x1, ss1);
      const float* bp = bt + ((size_t)((dbase >> 1) + st) * NT) * 64 + l;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float bv = bp[n * 64];
        acc[0][n] = MFMA32(x0, bv, acc[0][n]);
        acc[1][n] = MFMA32(x1, bv, acc[1][n]);
      }
      tile[(2 * i) * 65 + 2 * st + kk] = x0;
      tile[(2 * i + 1) * 65 + 2 * st + kk] = x1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int idx = it * 64 + l;
      const int tok = idx >> 4, c4 = (idx & 15) << 2;
      if (t0 + tok < N && dbase + c4 < D) {
        const float* q = tile + tok * 65 + c4;
        float4 v = make_float4(q[0], q[1], q[2], q[3]);
        *reinterpret_cast<float4*>(Xt + ((size_t)b * N + t0 + tok) * D + dbase + c4) = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // ---- combine the four D-slices (fixed order w = 0..3: deterministic) ---------------------------
  ss0 += __shfl_xor(ss0, 32);
  ss1 += __shfl_xor(ss1, 32);
  __syncthreads();
  constexpr int KP = NT * 32;
  float* sc = lds;                    // [64][KP+1]
  float* ssum = lds + 64 * (KP + 1);  // [4][64]
  if (kk == 0) {
    ssum[w * 64 + 2 * i] = ss0;
    ssum[w * 64 + 2 * i + 1] = ss1;
  }
  for (int rnd = 0; rnd < 4; ++rnd) {
    if (w == rnd) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int tok = 2 * sv_frag_row(r, kk) + mt;
            float* p = &sc[tok * (KP + 1) + n * 32 + i];
            *p = (rnd == 0) ? acc[mt][n][r] : (*p + acc[mt][n][r]);
          }
    }
    __syncthreads();
  }
  if (tid < 64 && t0 + tid < N) {
    const float s2 = ((ssum[tid] + ssum[64 + tid]) + ssum[128 + tid]) + ssum[192 + tid];
    SV_ASSIGN_TOKEN(sc, tid * (KP + 1), K, s2, (size_t)b * N + t0 + tid, labels, rnorm, gap);
  }
}

// ------------------------------------------------------------------------------------------------
// assign, wide-load variant (D % 32 == 0, K <= 64): workgroup = (image, 128-token tile), wave w owns tokens
// 32w..32w+31 for ALL d (no cross-wave reduction: one sequential fp32 chain per score, d = 0..D-1).
//   * the [32 d][128 token] chunk is fetched with 16-B loads (512 contiguous bytes per d row; the old kernel's
//     8-B loads ran at 1.25 TB/s) one chunk ahead into registers, then parked in a double-buffered LDS tile
//     (row stride 130 floats: conflict-free for both access patterns below);
//   * MFMA A operand = tile[d][token] (lanes = consecutive tokens), B = pre-swizzled centres from L2;
//   * the token-major copy Xt is written from the same tile: a lane gathers 4 consecutive d of one token
//     (banks 8 c4 + token: all 64 distinct) and stores 16 B; 8 lanes cover 128 contiguous bytes of a token row.
// ------------------------------------------------------------------------------------------------
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// one [32 d][128 token] chunk of assign_wide_kernel out of its LDS tile: scores (fp32 MFMA against the pre-swizzled centres),
// squared norms, and the token-major copy Xt
template <int NT>
__device__ __forceinline__ void assign_wide_chunk(const float* __restrict__ tl, const float* __restrict__ bt, float* __restrict__ Xt,
                                                  int b, int N, int D, int t0, int tid, int w, int l, int i, int kk, int c,
                                                  f32x16 (&acc)[NT], float& ss) {
  constexpr int DC = 32, TS = 128;
  auto rot = [](int d) { return 8 * (d >> 2) + 32 * (d & 1); };
#pragma unroll 8
  for (int st = 0; st < DC / 2; ++st) {
    const float x = tl[(2 * st + kk) * TS + ((32 * w + i + rot(2 * st + kk)) & 127)];
    ss = fmaf(x, x, ss);
    const float* bp = bt + ((size_t)(c * (DC / 2) + st) * NT) * 64 + l;
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = MFMA32(x, bp[n * 64], acc[n]);
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * 256 + tid;
    const int tok = idx >> 3, c4 = idx & 7;
    if (t0 + tok < N) {
      const float* q = tl + (4 * c4) * TS;   // rows 4 c4 + e: rotation 8 c4 + 32 (e & 1)
      const int t_a = (tok + 8 * c4) & 127, t_b = (tok + 8 * c4 + 32) & 127;
      const float4 o = make_float4(q[t_a], q[TS + t_b], q[2 * TS + t_a], q[3 * TS + t_b]);
      *reinterpret_cast<float4*>(Xt + ((size_t)b * N + t0 + tok) * D + c * DC + 4 * c4) = o;
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256) void assign_wide_kernel(const float* __restrict__ T, int N, int D, int K,
                                                          const float* __restrict__ bt, float* __restrict__ Xt,
                                                          uint8_t* __restrict__ labels, float* __restrict__ rnorm,
                                                          float* __restrict__ gap, int B) {
  // LDS tile [d][token], row stride 128 floats, row d ROTATED by rot(d) = 8 (d >> 2) + 32 (d & 1) tokens: the MFMA A
  // operand reads two rows d, d+1 per instruction (their rotations differ by 32 banks: disjoint), the transposed gather
  // that writes Xt reads (4 c4 + e, tok) for 8 values of c4 and 8 consecutive tokens (banks tok + 8 c4: all 64 distinct),
  // and the loader stores whole 16-B quads.  (PMC, round 2: with a plain stride of 130 floats 39 % of the LDS cycles of
  // this kernel were bank conflicts -- two-way on the A reads and on the 8-B stores.)
  constexpr int DC = 32, TS = 128;
  auto rot = [](int d) { return 8 * (d >> 2) + 32 * (d & 1); };
  __shared__ __attribute__((aligned(16))) float tile[2 * DC * TS + 128];   // also [128][NT*32+1] scores at the end (NT <= 2)
  __shared__ float ssum[128];
  // XCD-aware order (round 6): the workgroups are dealt to the eight XCDs round-robin by their linear id, so with (tile, image) read
  // straight off the grid the 12 token tiles of an image ran on 8 different XCDs -- and a token tile's 512-byte piece of a D-row
  // shares its first and last 128-byte line with its neighbours (rows of N = 1530 floats are not line aligned): every boundary line
  // crossed the fabric into two L2s, 2.36 GB fetched for 1.88 GB of tokens (rocprofv3 FETCH_SIZE, profiles/r06_pmc_traffic.json).
  // Consecutive LOGICAL tiles now share an XCD: logical id = (linear id % 8) * per + linear id / 8.
  const int gx = (N + 127) / 128;
  const int per = (int)((gridDim.x + 7) / 8);
  const int logical = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (logical >= gx * B) return;
  const int b = logical / gx, t0 = (logical - b * gx) * 128;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const float* Tb = T + (size_t)b * D * N;
  const int lr = tid >> 5, lq = tid & 31;        // loader: rows lr + 8 j, tokens t0 + 4 lq .. + 3
  const int tl0 = t0 + 4 * lq;
  const int nvalid = N - tl0;                    // tokens of this lane's quad inside the image
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  float ss = 0.f;
  const int nch = D / DC;
  // Two named register sets: chunks c + 1 AND c + 2 are in flight while chunk c is multiplied (one 16-KiB chunk per
  // workgroup in flight, four workgroups per CU, left the kernel at 3.8 TB/s of its read + write traffic; the loop is
  // unrolled by two so that the sets are never indexed dynamically).
  float4 va[4], vb[4];
#define SV_LOAD_CHUNK(V, c)                                                           \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                     \
    const float* p = Tb + (size_t)((c) * DC + lr + 8 * j) * N + tl0;                  \
    if (nvalid >= 4) {                                                                \
      const f32x4u u = *reinterpret_cast<const f32x4u*>(p);                           \
      V[j] = make_float4(u[0], u[1], u[2], u[3]);                                     \
    } else {                                                                          \
      V[j] = make_float4(nvalid > 0 ? p[0] : 0.f, nvalid > 1 ? p[1] : 0.f, nvalid > 2 ? p[2] : 0.f, 0.f); \
    }                                                                                 \
  }
#define SV_PARK_CHUNK(V, buf)                                                         \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                     \
    const int d_ = lr + 8 * j;                                                        \
    float* q = tile + (buf) * (DC * TS) + d_ * TS + ((4 * lq + rot(d_)) & 127);       \
    *reinterpret_cast<float4*>(q) = V[j];                                             \
  }
  SV_LOAD_CHUNK(va, 0)
  SV_PARK_CHUNK(va, 0)
  if (1 < nch) { SV_LOAD_CHUNK(va, 1) }
  __syncthreads();
  // chunk c + 1 waits in set A when c is even, in set B when c is odd
#define SV_ASSIGN_STEP(c, VNEXT, VFREE)                                               \
  {                                                                                   \
    if ((c) + 2 < nch) { SV_LOAD_CHUNK(VFREE, (c) + 2) }                              \
    assign_wide_chunk<NT>(tile + ((c) & 1) * (DC * TS), bt, Xt, b, N, D, t0, tid, w, l, i, kk, (c), acc, ss);  \
    if ((c) + 1 < nch) { SV_PARK_CHUNK(VNEXT, ((c) + 1) & 1) }                        \
    __syncthreads();                                                                  \
  }
  for (int c = 0; c < nch; c += 2) {
    SV_ASSIGN_STEP(c, va, vb)
    if (c + 1 < nch) SV_ASSIGN_STEP(c + 1, vb, va)
  }
#undef SV_ASSIGN_STEP
#undef SV_LOAD_CHUNK
#undef SV_PARK_CHUNK
  // ---- scores -> LDS [token][cluster]; one thread per token takes the first maximum and the runner-up ----------
  constexpr int KP = NT * 32;
  float* sc = tile;   // [128][KP+1]
  SV_SCORE_TILE_STORE(NT, acc, ss, sc, ssum, w, i, kk);
  __syncthreads();
  if (tid < 128 && t0 + tid < N) SV_ASSIGN_TOKEN(sc, tid * (KP + 1), K, ssum[tid], (size_t)b * N + t0 + tid, labels, rnorm, gap);
}

int sv_launch_assign(segvlad_ctx* ctx, const float* tokens, int B, int N, float* xt, uint8_t* labels, float* rnorm,
                     float* gap) {
  const int NT = ctx->Kpad / 32;
  dim3 grid((N + 63) / 64, B), block(256);
  const float* bt = ctx->vocab_bt.as<float>();
  if (NT <= 2 && ctx->D % 32 == 0 && !ctx->opt.assign_narrow) {
    // 1-D grid of (tiles x images) rounded up to a multiple of 8 (the kernel maps its linear id to a (tile, image) pair itself:
    // XCD-aware order)
    const unsigned tiles_total = (unsigned)((N + 127) / 128) * (unsigned)B;
    dim3 gridw((tiles_total + 7) / 8 * 8, 1);
    if (NT == 1)
      hipLaunchKernelGGL(assign_wide_kernel<1>, gridw, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, xt, labels, rnorm, gap, B);
    else
      hipLaunchKernelGGL(assign_wide_kernel<2>, gridw, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, xt, labels, rnorm, gap, B);
    SV_HIP(hipGetLastError());
    return SEGVLAD_OK;
  }
  switch (NT) {
    case 1:
      hipLaunchKernelGGL(assign_kernel<1>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, xt, labels, rnorm, gap);
      break;
    case 2:
      hipLaunchKernelGGL(assign_kernel<2>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, xt, labels, rnorm, gap);
      break;
    case 4:
      hipLaunchKernelGGL(assign_kernel<4>, grid, block, 0, ctx->stream, tokens, N, ctx->D, ctx->K, bt, xt, labels, rnorm, gap);
      break;
    default:
      return ctx->fail(SEGVLAD_ERR_LIMIT, "K=%d: supported cluster counts are 1..64 and 97..128 (Kpad in {32,64,128})", ctx->K);
  }
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
