// Mask branch of the describe stage from dense masks, for gfx950 (MI355X): what the aggregation needs to know about the segments
// before a token is read.  (Run-length masks: rle_kernels.hip; encoding and cleaning them: rle_encode_kernels.hip, regions_kernels.hip.)
//
//   incidence_kernel        masks -> token-incidence bit rows, one wave per (segment, 64-token word)        (func_vpr.py:1088-1092)
//   incidence_fused_kernel  the same rows AND the centroids from one coalesced pass over a mask's bytes: the default, taken when
//                           the mask rows are multiples of 16 bytes and the mask's bitmap fits the LDS
//   centroid_kernel         mask centroids for the Delaunay adjacency, exact integer sums divided in fp64      (func_vpr.py:1314)
//   adjacency_kernel        Delaunay neighbours of an image's centroids + self loop, raised to `order`, one workgroup per image,
//                           fp64; non-generic inputs are reported, not guessed                            (func_vpr.py:1315-1345)
//
// Wave = 64 lanes.  The pixel -> token map and the nearest-neighbour source index are incidence_dev.h's.
#include "ctx.h"
#include "incidence_dev.h"

// ------------------------------------------------------------------------------------------------
// incidence: one wave per (segment, 64-token word); lane = token.  The up-sampled pixel block of a
// token is walked through its distinct SOURCE rows/cols (nearest: src = min(floor(dst*scale), in-1)).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void incidence_kernel(const uint8_t* __restrict__ masks, int Hm, int Wm, int H, int W,
                                                        int patch, int dh, int dw, float sh, float sw,
                                                        uint64_t* __restrict__ inc, int nw) {
  const int s = blockIdx.x;
  const int word = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (word >= nw) return;
  const int lane = threadIdx.x & 63;
  const int N = dh * dw;
  const int t = word * 64 + lane;
  bool any = false;
  if (t < N) {
    const SvTokenCell tc = sv_token_cell(t, dh, dw, patch, H, W);
    const int i0 = tc.i0, i1 = tc.i1, j0 = tc.j0, j1 = tc.j1;
    const uint8_t* m = masks + (size_t)s * Hm * Wm;
    int pr = -1;
    for (int i = i0; i <= i1 && !any; ++i) {
      int r = sv_src_index(i, sh, Hm);
      if (r == pr) continue;
      pr = r;
      const uint8_t* row = m + (size_t)r * Wm;
      int pc = -1;
      for (int j = j0; j <= j1; ++j) {
        int c = sv_src_index(j, sw, Wm);
        if (c == pc) continue;
        pc = c;
        if (row[c]) { any = true; break; }
      }
    }
  }
  const uint64_t b = __ballot(any);
  if (lane == 0) inc[(size_t)s * nw + word] = b;
}

// ------------------------------------------------------------------------------------------------
// fused incidence + centroid: one workgroup per mask, ONE coalesced 16-B/lane pass over the mask bytes.
//   phase 1: every 16-pixel chunk is reduced to a 16-bit "non-zero" word; non-empty chunks are OR-ed into an
//            LDS bitmap of the mask (Hm x Wm bits) and feed the exact integer centroid sums;
//   phase 2: lane = token: OR of the bitmap bits its up-sampled 14x14 cell samples (range test per source
//            row when the mask is not larger than the image, per-pixel walk otherwise); ballot -> u64 words.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nz_nibble(uint32_t w) {  // bit j = (byte j of w != 0)
  uint32_t t = w | (w >> 4);
  t |= t >> 2;
  t |= t >> 1;
  t &= 0x01010101u;
  return ((t * 0x01020408u) >> 24) & 0xfu;
}

__global__ __launch_bounds__(256) void incidence_fused_kernel(const uint8_t* __restrict__ masks, int Hm, int Wm, int H, int W,
                                                              int patch, int dh, int dw, float sh, float sw,
                                                              uint64_t* __restrict__ inc, int nw,
                                                              double* __restrict__ cent) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* bits = reinterpret_cast<uint32_t*>(smem);  // [Hm][wpr]
  __shared__ unsigned long long red[3][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int wpr = (Wm + 31) >> 5;  // u32 words per bitmap row
  const int cpr = Wm >> 4;         // 16-pixel chunks per row (Wm % 16 == 0)
  for (int j = tid; j < Hm * wpr; j += 256) bits[j] = 0;
  __syncthreads();
  const uint4* m16 = reinterpret_cast<const uint4*>(masks + (size_t)s * Hm * Wm);
  const int total = Hm * cpr;
  unsigned long long sr = 0, sc = 0, cnt = 0;
  for (int q = tid; q < total; q += 256) {
    const uint4 v = m16[q];
    if ((v.x | v.y | v.z | v.w) == 0) continue;
    const uint32_t nz = nz_nibble(v.x) | (nz_nibble(v.y) << 4) | (nz_nibble(v.z) << 8) | (nz_nibble(v.w) << 12);
    const int r = q / cpr, cc = q - r * cpr;
    atomicOr(&bits[r * wpr + (cc >> 1)], nz << (16 * (cc & 1)));
    const uint32_t pc = __popc(nz);
    const uint32_t pos = __popc(nz & 0xAAAAu) + 2 * __popc(nz & 0xCCCCu) + 4 * __popc(nz & 0xF0F0u) + 8 * __popc(nz & 0xFF00u);
    cnt += pc;
    sr += (unsigned long long)r * pc;
    sc += (unsigned long long)(16 * cc) * pc + pos;
  }
  if (cent) {  // exact integer sums -> bit-identical to np.nonzero(mask).mean(1)[::-1]
    for (int o = 32; o > 0; o >>= 1) {
      sr += __shfl_xor(sr, o);
      sc += __shfl_xor(sc, o);
      cnt += __shfl_xor(cnt, o);
    }
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = sr;
      red[1][tid >> 6] = sc;
      red[2][tid >> 6] = cnt;
    }
  }
  __syncthreads();
  if (cent && tid == 0) {
    const double c = (double)(red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    cent[2 * (size_t)s + 0] = (double)(red[1][0] + red[1][1] + red[1][2] + red[1][3]) / c;
    cent[2 * (size_t)s + 1] = (double)(red[0][0] + red[0][1] + red[0][2] + red[0][3]) / c;
  }
  const int N = dh * dw;
  const bool ranges = (sh <= 1.0f) && (sw <= 1.0f);  // up-sampling: a cell samples contiguous source rows/cols
  for (int t0 = 0; t0 < nw * 64; t0 += 256) {
    const int t = t0 + tid;
    bool any = false;
    if (t < N) {
      const SvTokenCell tc = sv_token_cell(t, dh, dw, patch, H, W);
      const int i0 = tc.i0, i1 = tc.i1, j0 = tc.j0, j1 = tc.j1;
      if (ranges) {
        const int rlo = sv_src_index(i0, sh, Hm), rhi = sv_src_index(i1, sh, Hm);
        const int clo = sv_src_index(j0, sw, Wm), chi = sv_src_index(j1, sw, Wm);
        const int w0 = clo >> 5, w1 = chi >> 5;
        for (int r = rlo; r <= rhi && !any; ++r) {
          for (int wv = w0; wv <= w1; ++wv) {
            const int lo = (wv == w0) ? (clo & 31) : 0, hi = (wv == w1) ? (chi & 31) : 31;
            const uint32_t msk = (hi == 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
            if (bits[r * wpr + wv] & msk) { any = true; break; }
          }
        }
      } else {
        int pr = -1;
        for (int i = i0; i <= i1 && !any; ++i) {
          const int r = sv_src_index(i, sh, Hm);
          if (r == pr) continue;
          pr = r;
          int pc = -1;
          for (int j = j0; j <= j1; ++j) {
            const int c = sv_src_index(j, sw, Wm);
            if (c == pc) continue;
            pc = c;
            if ((bits[r * wpr + (c >> 5)] >> (c & 31)) & 1u) { any = true; break; }
          }
        }
      }
    }
    const uint64_t b = __ballot(any);
    const int word = t >> 6;
    if ((tid & 63) == 0 && word < nw) inc[(size_t)s * nw + word] = b;
  }
}

int sv_launch_incidence(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int H, int W, int patch,
                        uint64_t* inc_bits, double* centroids) {
  const int dh = H / patch, dw = W / patch;
  const int N = dh * dw, nw = (N + 63) / 64;
  const float sh = (float)Hm / (float)H, sw = (float)Wm / (float)W;
  if (S == 0) return SEGVLAD_OK;
  const size_t lds = (size_t)Hm * ((Wm + 31) / 32) * 4;
  if ((Wm % 16) == 0 && (reinterpret_cast<uintptr_t>(masks) & 15) == 0 && lds <= 150 * 1024) {
    if (lds > 64 * 1024)
      SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(incidence_fused_kernel), (size_t)lds));
    hipLaunchKernelGGL(incidence_fused_kernel, dim3(S), dim3(256), lds, ctx->stream, masks, Hm, Wm, H, W, patch, dh, dw, sh, sw,
                       inc_bits, nw, centroids);
    SV_HIP(hipGetLastError());
    return SEGVLAD_OK;
  }
  if (centroids) SV_TRY(sv_launch_centroids(ctx, masks, S, Hm, Wm, centroids));
  hipLaunchKernelGGL(incidence_kernel, dim3(S, (nw + 3) / 4), dim3(256), 0, ctx->stream, masks, Hm, Wm, H, W, patch, dh,
                     dw, sh, sw, inc_bits, nw);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// centroids: exact integer sums of the non-zero (row, col), divided in fp64 -> bit-identical to
// np.nonzero(mask).mean(1)[::-1]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void centroid_kernel(const uint8_t* __restrict__ masks, int Hm, int Wm,
                                                       double* __restrict__ out) {
  const int s = blockIdx.x;
  const uint8_t* m = masks + (size_t)s * Hm * Wm;
  unsigned long long sr = 0, sc = 0, cnt = 0;
  const int total = Hm * Wm;
  for (int p = threadIdx.x; p < total; p += 256) {
    if (m[p]) {
      const int r = p / Wm;
      sr += r;
      sc += p - r * Wm;
      ++cnt;
    }
  }
  __shared__ unsigned long long red[3][256];
  red[0][threadIdx.x] = sr;
  red[1][threadIdx.x] = sc;
  red[2][threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
      red[2][threadIdx.x] += red[2][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double c = (double)red[2][0];
    out[2 * s + 0] = (double)red[1][0] / c;  // x = mean col
    out[2 * s + 1] = (double)red[0][0] / c;  // y = mean row
  }
}

int sv_launch_centroids(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, double* out) {
  if (S == 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(centroid_kernel, dim3(S), dim3(256), 0, ctx->stream, masks, Hm, Wm, out);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// adjacency: Delaunay neighbours of the mask centroids + self loop, raised to `order`
// (nbrMasksAGGFastSingle, func_vpr.py:1315-1345), one workgroup per image, no host round trip.
//
// Edge (u,v) belongs to the Delaunay triangulation iff some circle through u and v is empty.  The
// circles through u,v are a one-parameter family (centre on the bisector, parameter t); a point p
// on the left of u->v excludes t > tau_p, a point on the right excludes t < tau_p, with
//     tau_p = ((p-u).(p-v)) / cross(v-u, p-u)            (a cotangent of the angle u-p-v).
// So the edge exists iff max_{right} tau <= min_{left} tau, and a point strictly inside the segment
// blocks it.  O(S) per pair, fp64.  Generic inputs give exactly Qhull's triangulation.  Non-generic inputs -- exactly
// co-circular quadruples (max_right tau == min_left tau: the triangulation is not unique, both diagonals are kept here,
// Qhull picks one) and duplicate centroids (Qhull drops the coplanar duplicate) -- are REPORTED: every image that holds
// one adds 65536 to *n_bad and sets bit 1 of img_flags[b] (bit 0: an empty mask, i.e. a NaN centroid), so that the caller
// can route exactly those images through the reference's own Qhull path.  "Co-circular" includes quadruples whose two
// bounds agree to within a few ulps: there the sign of tmax - tmin is rounding noise, and either answer could differ from
// Qhull's (which decides such cases by its own perturbation rules).
// S <= 3 reproduces the reference's special case: every row = e0 (+ e1).
// ------------------------------------------------------------------------------------------------
// Threads per image (= blockDim.x, a launch parameter): up to 1024 -- S (S - 1) / 2 point pairs, ~1 per thread at S = 50 -- for
// small batches, where the launch is one image's latency (round 5: 256 threads walked ~10 pairs each, half of them skipped, one
// fp64 division chain after the other: 207 -> 39 us for 25 images); 256 for large batches, where 16-wave workgroups only wait for a
// whole CU beside the assignment pass they are overlapped with (717 us for 200 images, 1024 threads, under that pass).
__global__ __launch_bounds__(1024) void adjacency_kernel(const double* __restrict__ cent,
                                                        const int32_t* __restrict__ seg_off,
                                                        const int64_t* __restrict__ adj_off, int order, int S_max,
                                                        uint8_t* __restrict__ adj, uint32_t* __restrict__ n_bad,
                                                        uint8_t* __restrict__ img_flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  const int SW = (S_max + 63) >> 6;
  double* px = reinterpret_cast<double*>(smem);                  // [S_max]
  double* py = px + S_max;                                       // [S_max]
  uint64_t* A1 = reinterpret_cast<uint64_t*>(py + S_max);        // [S_max][SW]
  uint64_t* P = A1 + (size_t)S_max * SW;                         // [S_max][SW]
  uint64_t* Q = P + (size_t)S_max * SW;                          // [S_max][SW]
  int& degenerate = *reinterpret_cast<int*>(Q + (size_t)S_max * SW);   // the last SV_ADJ_LDS_TAIL bytes (sv_adjacency_lds)
  const int tid = threadIdx.x;
  if (S == 0) return;
  uint8_t* out = adj + adj_off[b];
  for (int s = tid; s < S; s += (int)blockDim.x) {
    px[s] = cent[2 * (size_t)(s0 + s)];
    py[s] = cent[2 * (size_t)(s0 + s) + 1];
    if (px[s] != px[s]) {  // NaN centroid = empty mask (reference: ValueError)
      if (n_bad) atomicAdd(n_bad, 1u);
      if (img_flags) img_flags[b] = (uint8_t)(img_flags[b] | 1u);   // (same value from every writer; bit 1 is set later, by one thread)
    }
  }
  for (int j = tid; j < S * SW; j += (int)blockDim.x) A1[j] = 0;
  if (tid == 0) degenerate = 0;
  __syncthreads();
  if (S <= 3) {
    for (int j = tid; j < S * S; j += (int)blockDim.x) {
      const int w = j % S;
      out[j] = (w == 0 || (w == 1 && S > 1)) ? 1 : 0;
    }
    return;
  }
  for (int u = tid; u < S; u += (int)blockDim.x) atomicOr(reinterpret_cast<unsigned long long*>(&A1[u * SW + (u >> 6)]), 1ull << (u & 63));
  const int npairs = S * (S - 1) / 2;
  for (int e = tid; e < npairs; e += (int)blockDim.x) {
    // pair e of the strict upper triangle, row-major: row u starts at u (2 S - u - 1) / 2
    int u = (int)(((double)(2 * S - 1) - sqrt((double)(2 * S - 1) * (double)(2 * S - 1) - 8.0 * (double)e)) * 0.5);
    while (u > 0 && u * (2 * S - u - 1) / 2 > e) --u;
    while ((u + 1) * (2 * S - u - 2) / 2 <= e) ++u;
    const int v = u + 1 + (e - u * (2 * S - u - 1) / 2);
    const double ux = px[u], uy = py[u], vx = px[v], vy = py[v];
    const double ex = vx - ux, ey = vy - uy;
    if (ex == 0.0 && ey == 0.0) degenerate = 1;   // duplicate centroid
    double tmin = INFINITY, tmax = -INFINITY, emin = 0.0, emax = 0.0;   // e*: rounding-error bounds of the two extremes
    bool blocked = false;
    for (int p = 0; p < S; ++p) {
      if (p == u || p == v) continue;
      const double ax = px[p] - ux, ay = py[p] - uy;
      const double bx = px[p] - vx, by = py[p] - vy;
      const double num = fma(ax, bx, ay * by);
      const double den = fma(ex, ay, -(ey * ax));
      if (den != 0.0) {
        const double t = num / den;
        // |computed tau - exact tau| for THESE coordinates: the differences, the two sums of products and the quotient
        // each carry a few 2^-53 relative to the magnitudes that entered them
        const double err = 9e-16 * ((fabs(ax * bx) + fabs(ay * by)) + fabs(t) * (fabs(ex * ay) + fabs(ey * ax))) / fabs(den);
        if (den > 0.0) {
          if (t < tmin) {
            tmin = t;
            emin = err;
          }
        } else if (t > tmax) {
          tmax = t;
          emax = err;
        }
      } else if (num < 0.0) {
        blocked = true;
      }
    }
    // an empty circle through four points (either diagonal is Delaunay): exactly (lattice centroids: every quantity above is
    // exact, equal taus compare equal), or so nearly that the sign of tmax - tmin is rounding noise
    if (!blocked && tmax > -INFINITY && tmin < INFINITY && fabs(tmax - tmin) <= emin + emax) degenerate = 1;
    if (!blocked && tmax <= tmin) {
      atomicOr(reinterpret_cast<unsigned long long*>(&A1[u * SW + (v >> 6)]), 1ull << (v & 63));
      atomicOr(reinterpret_cast<unsigned long long*>(&A1[v * SW + (u >> 6)]), 1ull << (u & 63));
    }
  }
  __syncthreads();
  if (tid == 0 && degenerate) {
    if (n_bad) atomicAdd(n_bad, 65536u);
    if (img_flags) img_flags[b] = (uint8_t)(img_flags[b] | 2u);
  }
  for (int j = tid; j < S * SW; j += (int)blockDim.x) P[j] = A1[j];
  __syncthreads();
  for (int it = 1; it < order; ++it) {  // P <- (P . A1) > 0
    for (int j = tid; j < S * SW; j += (int)blockDim.x) {
      const int v = j / SW, w = j - v * SW;
      uint64_t acc = 0;
      for (int uw = 0; uw < SW; ++uw) {
        uint64_t m = P[v * SW + uw];
        while (m) {
          const int u = (uw << 6) + __ffsll((unsigned long long)m) - 1;
          m &= m - 1;
          acc |= A1[u * SW + w];
        }
      }
      Q[j] = acc;
    }
    __syncthreads();
    for (int j = tid; j < S * SW; j += (int)blockDim.x) P[j] = Q[j];
    __syncthreads();
  }
  for (int j = tid; j < S * S; j += (int)blockDim.x) {
    const int v = j / S, w = j - v * S;
    out[j] = (uint8_t)((P[v * SW + (w >> 6)] >> (w & 63)) & 1ull);
  }
}

// Every byte of LDS the kernel uses for an image of S_max segments: the coordinates, the three bit matrices and the flag word.  The
// kernel declares no __shared__ variable, so this is the whole workgroup's allocation and the one figure compared with the 160 KiB
// of a CU (a static variable beside the dynamic block would be allocated on top of it, unseen by that comparison).
constexpr size_t SV_ADJ_LDS_TAIL = 16;   // `degenerate`, padded to the block's alignment
static size_t sv_adjacency_lds(int S_max) {
  const size_t SW = ((size_t)S_max + 63) / 64;
  return (size_t)S_max * 16 + (size_t)3 * S_max * SW * 8 + SV_ADJ_LDS_TAIL;
}
bool sv_adjacency_fits(int S_max) { return sv_adjacency_lds(S_max) <= 160 * 1024; }

int sv_launch_adjacency(segvlad_ctx* ctx, const double* cent, const int32_t* seg_off_dev, const int64_t* adj_off_dev,
                        int B, int S_max, int order, uint8_t* adj, uint32_t* n_bad, uint8_t* img_flags) {
  if (B <= 0 || S_max <= 0) return SEGVLAD_OK;
  const size_t lds = sv_adjacency_lds(S_max);
  if (!sv_adjacency_fits(S_max))
    return ctx->fail(SEGVLAD_ERR_LIMIT, "adjacency: %d segments in one image exceed the LDS budget (%zu B)", S_max, lds);
  if (lds > 64 * 1024)
    SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(adjacency_kernel), (size_t)lds));
  hipLaunchKernelGGL(adjacency_kernel, dim3(B), dim3(B <= 64 ? 1024 : 256), lds, ctx->stream, cent, seg_off_dev, adj_off_dev, order, S_max,
                     adj, n_bad, img_flags);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
