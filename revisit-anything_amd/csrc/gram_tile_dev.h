// The 128 x 128 self-similarity tile of the burst discount (burst_kernels.hip: image scope; burst_seg_kernels.hip: segment scope):
// acc = the raw dot products of 128 token rows (A side) with 128 token rows (B side) of one image's token-major copy Xt [N][D], per pair
// the sequential fp32 chain over d = 0 .. D - 1 on v_mfma_f32_32x32x2_f32.  One definition: which row of Xt stands behind a tile row is
// the caller's (the position itself, or tok_order[position]), and so is what becomes of the products (the cosine is the product times the
// two 1 / ||x|| in the caller's epilogue); the chain between is this file's, so the two scopes agree on it by construction.
//
// Workgroup: 256 threads = 4 waves, wave (wr, wc) owns the 64 x 64 quadrant of rows 64 wr .. and columns 64 wc .. as 2 x 2 MFMA tiles.
// A chunk of SV_GRAM_KC d travels in one register stage (in flight under the previous chunk's MFMAs) and is parked in LDS between two
// barriers.  Lane (i, kk) of a wave reads 4 consecutive d of row i per ds_read_b128 -- d = 8 q + 4 kk + c feeds MFMA step (q, c) on both
// sides, so the contraction runs over every d once in one fixed order.
#pragma once
#include "mfma_f32_dev.h"

constexpr int SV_GRAM_TILE = 128;   // tokens per tile side
constexpr int SV_GRAM_KC = 32;      // d per LDS chunk
constexpr int SV_GRAM_LD = 36;      // LDS row stride in floats: lane i's 16 bytes start at bank 36 i mod 64 = 4 (9 i mod 16), and each of
                                    // the four 16-lane groups of a ds_read_b128 holds every i mod 16 once: no bank conflict

// Workgroups to images.  `per` workgroups belong to one image.  A batch of >= 8 images is dealt by the linear workgroup id, which is
// how the hardware deals workgroups to the 8 XCDs: image b on XCD b % 8, its workgroups share that XCD's L2 (the grid is padded to a
// multiple of 8 images; img >= B returns).  Fewer images: image-major, the tiles spread over every XCD.
inline int sv_gram_by_xcd(int B) { return B >= 8 ? 1 : 0; }
inline long long sv_gram_grid(int B, long long per) { return sv_gram_by_xcd(B) ? 8ll * ((B + 7) / 8) * per : (long long)B * per; }
__device__ __forceinline__ void sv_gram_deal(int by_xcd, int per, int& img, int& t) {
  if (by_xcd) {
    const int slot = (int)blockIdx.x >> 3;
    img = (slot / per) * 8 + ((int)blockIdx.x & 7), t = slot % per;
  } else {
    img = (int)blockIdx.x / per, t = (int)blockIdx.x % per;
  }
}

// u = g^-p
__device__ __forceinline__ float sv_burst_discount(float g, float p) { return p == 0.f ? 1.0f : p == 1.f ? 1.0f / g : powf(g, -p); }

// Called by all 256 threads.  Xb: the image's Xt.  ra / rb: the rows of Xt behind the A-side / B-side tile rows lr + 32 j of this
// thread, lr = threadIdx.x >> 3 (-1: beyond N, the row is zero in LDS; columns of d beyond D are zero too).  sA, sB: LDS,
// [SV_GRAM_TILE][SV_GRAM_LD] floats each, 16-byte aligned.  acc[ti][tj][r] = the chain of A-side row 64 wr + 32 ti + sv_frag_row(r, kk)
// with B-side row 64 wc + 32 tj + i.  D % 4 == 0: a float4 is inside or outside D as a whole.
// Barriers: on entry every wave is done with whatever sA / sB held; on return every wave has finished reading them.
__device__ __forceinline__ void sv_gram_tile(const float* Xb, const int (&ra)[4], const int (&rb)[4], int D, float* sA, float* sB,
                                             f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int lc = 4 * (tid & 7), lr = tid >> 3;   // this thread's float4 column of a chunk and its first row (then + 32, 64, 96)
  float4 pa[4], pb[4];
  auto fetch = [&](int d0) {
    const bool dok = d0 + lc < D;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pa[j] = (dok && ra[j] >= 0) ? *reinterpret_cast<const float4*>(Xb + (size_t)ra[j] * D + d0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
      pb[j] = (dok && rb[j] >= 0) ? *reinterpret_cast<const float4*>(Xb + (size_t)rb[j] * D + d0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;

  fetch(0);
  for (int d0 = 0; d0 < D; d0 += SV_GRAM_KC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<float4*>(sA + (lr + 32 * j) * SV_GRAM_LD + lc) = pa[j];
      *reinterpret_cast<float4*>(sB + (lr + 32 * j) * SV_GRAM_LD + lc) = pb[j];
    }
    __syncthreads();
    if (d0 + SV_GRAM_KC < D) fetch(d0 + SV_GRAM_KC);   // the next chunk's loads are in flight under this chunk's MFMAs
#pragma unroll
    for (int q = 0; q < SV_GRAM_KC / 8; ++q) {
      const int dc = 8 * q + 4 * kk;
      const float4 a0 = *reinterpret_cast<const float4*>(sA + (64 * wr + i) * SV_GRAM_LD + dc);
      const float4 a1 = *reinterpret_cast<const float4*>(sA + (64 * wr + 32 + i) * SV_GRAM_LD + dc);
      const float4 b0 = *reinterpret_cast<const float4*>(sB + (64 * wc + i) * SV_GRAM_LD + dc);
      const float4 b1 = *reinterpret_cast<const float4*>(sB + (64 * wc + 32 + i) * SV_GRAM_LD + dc);
#define SV_GRAM_STEP(c)                             \
  acc[0][0] = MFMA32(a0.c, b0.c, acc[0][0]);        \
  acc[0][1] = MFMA32(a0.c, b1.c, acc[0][1]);        \
  acc[1][0] = MFMA32(a1.c, b0.c, acc[1][0]);        \
  acc[1][1] = MFMA32(a1.c, b1.c, acc[1][1]);
      SV_GRAM_STEP(x) SV_GRAM_STEP(y) SV_GRAM_STEP(z) SV_GRAM_STEP(w)
#undef SV_GRAM_STEP
    }
    __syncthreads();
  }
}
