// Hard-assignment segment VLAD for gfx950 (MI355X): from the labels and the incidence rows to the descriptor.  Reference semantics:
// func_vpr.py:1065-1210.  (Before it: mask_kernels.hip, assign_kernels.hip; the PCA "project" form runs block_norm_kernels.hip and
// project_kernels.hip in the place of aggregate_kernel; soft and burst-weighted VLAD: soft_vlad_kernels.hip, burst_seg_kernels.hip.)
//
//   prep_kernel        per image: neighbour union (adj . inc) > 0, the token order grouped by label with its 1/||x|| and column
//                      masks, 1/sqrt(#non-empty blocks) per segment, and for the project form each position's row among its
//                      list's covered positions                                                  (func_vpr.py:1199-1200,1205)
//   aggregate_kernel   per (image, cluster): masked residual sums on the fp32 MFMA, intra-norm, global norm, packed store;
//                      <true>: additionally / instead the two fp16 planes of the descriptor that the projection GEMM reads
//                                                                                                 (func_vpr.py:1151,1195-1205)
//
// Wave = 64 lanes.  The aggregation runs on v_mfma_f32_32x32x2_f32 (exact fp32 fma chain), its token rows through a wave-private
// queue of global->LDS DMAs with counted waits (mfma_f32_dev.h, waitcnt_dev.h).
#include "ctx.h"
#include "mfma_f32_dev.h"

// ------------------------------------------------------------------------------------------------
// prep: one workgroup per image.
//   inc2[s] = OR_{u : adj[s][u]} inc[u]                       (adj . inc) > 0
//   colmask[t][sc] bit (s - 64 sc) = inc2[s][t]               column form consumed by the aggregation
//   gscale[s] = 1/sqrt(#clusters k with a token t: label_t = k and inc2[s][t])
//   phys[p], cov_cnt[k]   (phys != null: the "project" form) the PHYSICAL row of position p inside its (image, cluster) list
//                         of the grouped planes and of Z: its rank among the list's COVERED positions (a position is covered
//                         when some segment's inc2 holds its token), -1 for an uncovered one -- no segment reads its projected
//                         row, so it gets none; cov_cnt = covered positions of the list.  cover == 0: every position counts as
//                         covered (phys = p - lab_off[k], cov_cnt = the list's length).  Logical positions stay what they are.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(const uint8_t* __restrict__ labels, const uint64_t* __restrict__ inc,
                                                   const int32_t* __restrict__ seg_off,
                                                   const int64_t* __restrict__ adj_off, const uint8_t* __restrict__ adj,
                                                   int N, int K, int S_max, int SC, uint64_t* __restrict__ colmask,
                                                   float* __restrict__ gscale, int32_t* __restrict__ tok_order,
                                                   int32_t* __restrict__ lab_off, const float* __restrict__ rnorm,
                                                   float* __restrict__ rn_sorted, int stage, int ord_n,
                                                   int32_t* __restrict__ phys, int32_t* __restrict__ cov_cnt, int cover) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int nw = (N + 63) >> 6;
  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  uint64_t* inc2 = reinterpret_cast<uint64_t*>(smem);  // [S_max][nw]
  uint64_t* lbits = inc2 + (size_t)S_max * nw;         // [K][nw]
  const int tid = threadIdx.x;
  if (adj && stage) {
    // neighbour-union of the incidence rows, from LDS: the image's own rows and its adjacency (as bit rows) are staged
    // with coalesced loads first -- walking the S adjacency bytes of a row in global memory with a conditional 8-B load
    // behind each (S x nw x S dependent round trips spread over 256 threads) was 0.1 of this kernel's 0.16 ms
    const int SW = (S_max + 63) >> 6;
    uint64_t* inc0 = reinterpret_cast<uint64_t*>(reinterpret_cast<int*>(lbits + (size_t)K * nw) + ord_n);   // [S_max][nw]
    uint64_t* nbr = inc0 + (size_t)S_max * nw;                                                                       // [S_max][SW]
    for (int idx = tid; idx < S * nw; idx += 256) inc0[idx] = inc[(size_t)s0 * nw + idx];
    for (int idx = tid; idx < S * SW; idx += 256) nbr[idx] = 0;
    __syncthreads();
    const uint8_t* a = adj + adj_off[b];
    for (int e = tid; e < S * S; e += 256)
      if (a[e]) {
        const int s = e / S, u = e - s * S;
        atomicOr(reinterpret_cast<unsigned long long*>(&nbr[s * SW + (u >> 6)]), 1ull << (u & 63));
      }
    __syncthreads();
    for (int idx = tid; idx < S * nw; idx += 256) {
      const int s = idx / nw, w = idx - s * nw;
      uint64_t v = 0;
      for (int uw = 0; uw < SW; ++uw) {
        uint64_t m = nbr[s * SW + uw];
        while (m) {
          const int u = (uw << 6) + __builtin_ctzll(m);
          m &= m - 1;
          v |= inc0[u * nw + w];
        }
      }
      inc2[idx] = v;
    }
  } else {
    for (int idx = tid; idx < S * nw; idx += 256) {
      const int s = idx / nw, w = idx - s * nw;
      uint64_t v = 0;
      if (adj) {
        const uint8_t* a = adj + adj_off[b] + (size_t)s * S;
        for (int u = 0; u < S; ++u)
          if (a[u]) v |= inc[(size_t)(s0 + u) * nw + w];
      } else {
        v = inc[(size_t)(s0 + s) * nw + w];
      }
      inc2[idx] = v;
    }
  }
  for (int idx = tid; idx < K * nw; idx += 256) lbits[idx] = 0;
  __syncthreads();
  for (int t = tid; t < N; t += 256) {
    const int lab = labels[(size_t)b * N + t];
    atomicOr(reinterpret_cast<unsigned long long*>(&lbits[lab * nw + (t >> 6)]), 1ull << (t & 63));
  }
  __syncthreads();
  // token order grouped by label (ascending token id inside a label): the aggregation workgroup of (k, b) reads its
  // token list, the tokens' 1/||x|| and their segment masks from CONTIGUOUS ranges instead of re-scanning all N
  // labels and gathering per token (one dependent global round trip instead of four)
  __shared__ int kcnt[257];
  int* ord = reinterpret_cast<int*>(lbits + (size_t)K * nw);   // [ord_n >= max(N, S)]
  for (int k = tid; k < K; k += 256) {
    int c = 0;
    for (int w = 0; w < nw; ++w) c += __popcll(lbits[k * nw + w]);
    kcnt[k] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int k = 0; k < K; ++k) {
      const int c = kcnt[k];
      kcnt[k] = a;
      a += c;
    }
    kcnt[K] = a;
  }
  __syncthreads();
  for (int k = tid; k <= K; k += 256) lab_off[(size_t)b * (K + 1) + k] = kcnt[k];
  for (int k = tid; k < K; k += 256) {
    int pos = kcnt[k];
    for (int w = 0; w < nw; ++w) {
      uint64_t m = lbits[k * nw + w];
      while (m) {
        ord[pos++] = 64 * w + __builtin_ctzll(m);
        m &= m - 1;
      }
    }
  }
  __syncthreads();
  // covered positions as bit rows (word q = positions 64 q .. 64 q + 63: one wave's ballot) and their running counts, behind the
  // token order (the staged union's rows, dead by now, or the launcher's extra bytes)
  uint64_t* cbits = reinterpret_cast<uint64_t*>(ord + ord_n);   // [nw]
  int* cpre = reinterpret_cast<int*>(cbits + nw);               // [nw + 1] covered positions before word q
  for (int p = tid; p < N; p += 256) {
    const int t = ord[p];
    const int w = t >> 6, bit = t & 63;
    tok_order[(size_t)b * N + p] = t;
    rn_sorted[(size_t)b * N + p] = rnorm[(size_t)b * N + t];
    uint64_t any = 0;
    for (int sc = 0; sc < SC; ++sc) {
      uint64_t m = 0;
      const int lo = sc * 64, hi = min(S, lo + 64);
      for (int s = lo; s < hi; ++s) m |= ((inc2[s * nw + w] >> bit) & 1ull) << (s - lo);
      colmask[((size_t)b * N + p) * SC + sc] = m;   // indexed by POSITION in the label-grouped order
      any |= m;
    }
    if (phys) {   // (p = tid + 256 it: the wave's active lanes are the positions of ONE word)
      const uint64_t cw = __builtin_amdgcn_ballot_w64(any != 0 || !cover);
      if ((tid & 63) == 0) cbits[p >> 6] = cw;
    }
  }
  __syncthreads();
  if (phys && tid == 0) {
    int a = 0;
    for (int q = 0; q < nw; ++q) {
      cpre[q] = a;
      a += __popcll(cbits[q]);
    }
    cpre[nw] = a;
  }
  // number of non-empty (segment, cluster) blocks per segment: one thread per PAIR (a thread per segment walked K * nw
  // word pairs alone while 200 threads idled), counted in the (now free) token-order array
  int* nnz = ord;
  for (int s = tid; s < S; s += 256) nnz[s] = 0;
  __syncthreads();
  if (phys) {
    // covered positions before position p (p <= N)
    auto crank = [&](int p) { return (p >> 6) < nw ? cpre[p >> 6] + __popcll(cbits[p >> 6] & ((1ull << (p & 63)) - 1ull)) : cpre[nw]; };
    for (int p = tid; p < N; p += 256) {
      int lo = 0, hi = K - 1;   // the list of p: the last k with kcnt[k] <= p (an empty list shares its start with the next one)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (kcnt[mid] <= p) lo = mid;
        else hi = mid - 1;
      }
      phys[(size_t)b * N + p] = ((cbits[p >> 6] >> (p & 63)) & 1ull) ? crank(p) - crank(kcnt[lo]) : -1;
    }
    for (int k = tid; k < K; k += 256) cov_cnt[(size_t)b * K + k] = crank(kcnt[k + 1]) - crank(kcnt[k]);
  }
  for (int idx = tid; idx < S * K; idx += 256) {
    const int s = idx / K, k = idx - s * K;
    uint64_t any = 0;
    for (int w = 0; w < nw; ++w) any |= inc2[s * nw + w] & lbits[k * nw + w];
    if (any != 0) atomicAdd(&nnz[s], 1);
  }
  __syncthreads();
  for (int s = tid; s < S; s += 256) gscale[s0 + s] = nnz[s] > 0 ? (float)(1.0 / sqrt((double)nnz[s])) : 0.f;
}

int sv_launch_prep(segvlad_ctx* ctx, const uint8_t* labels, const uint64_t* inc_bits, const int32_t* seg_off_dev,
                   const int64_t* adj_off_dev, const uint8_t* adj, int B, int N, int K, int S_max, int SC,
                   uint64_t* colmask, float* gscale, int32_t* phys, int32_t* cov_cnt, int cover) {
  const int nw = (N + 63) / 64;
  if (K > 256) return ctx->fail(SEGVLAD_ERR_LIMIT, "prep: K=%d > 256", K);
  SV_HIP(ctx->s_tokorder.reserve((size_t)B * N * sizeof(int32_t)));
  SV_HIP(ctx->s_laboff.reserve((size_t)B * (K + 1) * sizeof(int32_t)));
  SV_HIP(ctx->s_rnsorted.reserve((size_t)B * N * sizeof(float)));
  const int ord_n = ((N > S_max ? N : S_max) + 1) & ~1;   // token order, later the per-segment block counts
  // (+ the covered-position words and their running counts, behind the token order)
  size_t lds = ((size_t)S_max + K) * nw * sizeof(uint64_t) + (size_t)ord_n * sizeof(int) + (size_t)nw * 8 + (size_t)(nw + 2) * 4;
  if (lds > 160 * 1024)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "prep: (S_max=%d + K=%d) x %d token words needs %zu B of LDS (limit 160 KiB)", S_max,
                     K, nw, lds);
  // staged neighbour union (the image's incidence rows + adjacency bit rows in LDS) when it fits beside the rest
  const size_t lds_staged = ((size_t)S_max + K) * nw * 8 + (size_t)ord_n * 4 + (size_t)S_max * nw * 8 +
                            (size_t)S_max * ((S_max + 63) / 64) * 8;
  const int stage = (adj != nullptr && lds_staged <= 150 * 1024) ? 1 : 0;
  if (stage && lds_staged > lds) lds = lds_staged;
  if (lds > 64 * 1024)
    SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(prep_kernel), (size_t)lds));
  hipLaunchKernelGGL(prep_kernel, dim3(B), dim3(256), lds, ctx->stream, labels, inc_bits, seg_off_dev, adj_off_dev, adj, N,
                     K, S_max, SC, colmask, gscale, ctx->s_tokorder.as<int32_t>(), ctx->s_laboff.as<int32_t>(),
                     ctx->s_rnorm.as<float>(), ctx->s_rnsorted.as<float>(), stage, ord_n, phys, cov_cnt, cover);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ------------------------------------------------------------------------------------------------
// aggregate: workgroup = (cluster k, image b); wave w owns d in [128 w, 128 w + 128).
//   V[s][k][d] = sum_{t in L_k} inc2[s][t] * (x_t[d] * rn_t - C[k][d])
// as an MFMA product  (32 segments x 2 tokens) . (2 tokens x 32 d):
//   A[i][kk] = bit (32 mt + i) of colmask[t_kk]   (0/1 exact)
//   B[kk][j] = fma(Xt[t_kk][dcol + 4 j + q], rn, -C[k][...])   q = N-tile; one 16-B load feeds 4 N-tiles
// then ||V[s,k,:]|| (LDS reduction across the waves), scale by gscale[s]/max(norm,1e-12), store packed.
// ------------------------------------------------------------------------------------------------
// PLANES: additionally (or instead: out may be NULL) emit the PCA input planes of the block,
//   (v - mean) * xscale = h1 + h2 (two fp16 terms, see gemm_f16x3_kernels.hip), so that the projection GEMM reads the
//   descriptor without a separate max-abs + split pass and the fp32 descriptor need not reach HBM at all
//   (|v| <= 1 by construction, which is what makes the scale known in advance).
//   The planes go out in the blocked layout the projection GEMM reads (sv_x3_off, ctx.h).  This is the "planes" form of
//   segvlad_images_pca; its "project" form runs token_norms_kernel (block_norm_kernels.hip) instead of this kernel.
constexpr int AGG_QD = 6;   // token-pair rows in flight per wave

template <bool PLANES>
__global__ __launch_bounds__(768) void aggregate_kernel(const float* __restrict__ Xt, const float* __restrict__ rnorm,
                                                        const int32_t* __restrict__ tok_order,
                                                        const int32_t* __restrict__ lab_off,
                                                        const uint64_t* __restrict__ colmask,
                                                        const float* __restrict__ C, const int32_t* __restrict__ seg_off,
                                                        const float* __restrict__ gscale, int N, int D, int K, int SC,
                                                        int Ncap, float* __restrict__ out,
                                                        float* __restrict__ block_norms, const float* __restrict__ mean,
                                                        float xscale, _Float16* __restrict__ h1, _Float16* __restrict__ h2,
                                                        int kpb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int nwaves = blockDim.x >> 6;
  const int PW = nwaves * 2 + 1;
  uint64_t* mskl = reinterpret_cast<uint64_t*>(smem);         // [Ncap]
  int* tokl = reinterpret_cast<int*>(mskl + Ncap);            // [Ncap]
  float* rnl = reinterpret_cast<float*>(tokl + Ncap);         // [Ncap]
  float* part = rnl + Ncap;                                   // [64][PW]
  float* alpha = part + 64 * PW;                              // [64]
  int* wcount = reinterpret_cast<int*>(alpha + 64);           // [16]
  constexpr int QD = AGG_QD;
  unsigned char* xq = reinterpret_cast<unsigned char*>(wcount + 16);  // [nwaves][QD][1 KiB] DMA queue (16-B aligned)

  // a workgroup walks kpb consecutive clusters of its image: the (fire-and-forget) block stores of cluster k drain
  // while the lists and token rows of cluster k+1 are fetched -- with one workgroup per CU (registers) nothing else
  // would overlap the two
  const int k_end = min(K, ((int)blockIdx.x + 1) * kpb);
  for (int k = (int)blockIdx.x * kpb; k < k_end; ++k) {
  // ---- L_k: the tokens assigned to cluster k, ascending (grouped by prep_kernel) ---------------------
  const int o0 = lab_off[(size_t)b * (K + 1) + k];
  const int n = lab_off[(size_t)b * (K + 1) + k + 1] - o0;
  for (int j = tid; j < n; j += blockDim.x) {
    tokl[j] = tok_order[(size_t)b * N + o0 + j];
    rnl[j] = rnorm[(size_t)b * N + o0 + j];   // 1/||x|| in the label-grouped order (prep_kernel)
  }
  if (tid == 0 && (n & 1)) {  // pad to an even count with a zero-weight entry
    tokl[n] = 0;
    rnl[n] = 0.f;
  }
  const int npairs = (n + 1) >> 1;
  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  const int dcol = w * 128 + 4 * i;
  const bool dvalid = dcol < D;
  float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (dvalid && C != nullptr) c4 = *reinterpret_cast<const float4*>(C + (size_t)k * D + dcol);
  float4 mu4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (PLANES && dvalid && mean != nullptr) mu4 = *reinterpret_cast<const float4*>(mean + (size_t)k * D + dcol);
  const float* Xb = Xt + (size_t)b * N * D + dcol;
  const size_t KD = (size_t)K * D;
  const int SCb = (S + 63) >> 6;

  for (int sc = 0; sc < SCb; ++sc) {
    for (int j = tid; j < n; j += blockDim.x) mskl[j] = colmask[((size_t)b * N + o0 + j) * SC + sc];
    if (tid == 0 && (n & 1)) mskl[n] = 0;
    __syncthreads();
    const int Sc = min(64, S - 64 * sc);
    const bool two = Sc > 32;
    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][q][r] = 0.f;

    // token rows reach the MFMA through a wave-private LDS queue filled by global->LDS DMA (lane l's 16 B land at
    // slot + 16 l and are read back by the same lane): QD pairs in flight per wave without spending VGPRs on them --
    // with two register-staged loads in flight the loop was one HBM round trip per two token pairs
    {
      unsigned char* qbase = xq + (size_t)__builtin_amdgcn_readfirstlane(w) * (QD * 1024);   // wave-uniform: lives in M0
      auto issue = [&](int p) {
        const int t = sv_lds_read_i32(sv_lds_addr(tokl + 2 * p + kk));
        // lanes beyond D (a partial last wave) fetch a valid dummy address: their 16 B are never used
        const float* src = dvalid ? Xb + (size_t)t * D : Xt;
        __builtin_amdgcn_global_load_lds((sv_gptr_t)src, (sv_lptr_t)(qbase + (p % QD) * 1024), 16, 0, 0);
      };
      for (int q = 0; q < QD && q < npairs; ++q) issue(q);
      for (int p = 0; p < npairs; ++p) {
        const int j = 2 * p + kk;
        sv_wait_queue<QD>(npairs - 1 - p);   // (the DMAs issued after pair p's)
        f32x4 x;
        float rn;
        uint64_t m;
        lds_step_read(sv_lds_addr(qbase + (p % QD) * 1024 + l * 16), sv_lds_addr(rnl + j), sv_lds_addr(mskl + j), x, rn, m);
        // (the slot has been read -- lgkmcnt(0) inside -- before it is refilled)
        if (p + QD < npairs) issue(p + QD);
        if (!dvalid) x = f32x4{0.f, 0.f, 0.f, 0.f};
        const float b0 = fmaf(x.x, rn, -c4.x), b1 = fmaf(x.y, rn, -c4.y);
        const float b2 = fmaf(x.z, rn, -c4.z), b3 = fmaf(x.w, rn, -c4.w);
        const float a0 = ((m >> i) & 1ull) ? 1.f : 0.f;
        acc[0][0] = MFMA32(a0, b0, acc[0][0]);
        acc[0][1] = MFMA32(a0, b1, acc[0][1]);
        acc[0][2] = MFMA32(a0, b2, acc[0][2]);
        acc[0][3] = MFMA32(a0, b3, acc[0][3]);
        if (two) {
          const float a1 = ((m >> (32 + i)) & 1ull) ? 1.f : 0.f;
          acc[1][0] = MFMA32(a1, b0, acc[1][0]);
          acc[1][1] = MFMA32(a1, b1, acc[1][1]);
          acc[1][2] = MFMA32(a1, b2, acc[1][2]);
          acc[1][3] = MFMA32(a1, b3, acc[1][3]);
        }
      }
    }
    // ---- block norms: quad reduce in registers, then across lanes/waves through LDS ----------------
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (mt == 1 && !two) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = acc[mt][0][r] * acc[mt][0][r];
        p = fmaf(acc[mt][1][r], acc[mt][1][r], p);
        p = fmaf(acc[mt][2][r], acc[mt][2][r], p);
        p = fmaf(acc[mt][3][r], acc[mt][3][r], p);
        p = sv_dpp_row_sum(p);
        if ((l & 15) == 0) part[(32 * mt + sv_frag_row(r, kk)) * PW + w * 2 + ((l >> 4) & 1)] = p;
      }
    }
    __syncthreads();
    if (tid < Sc) {
      float sum = 0.f;
      const int cnt = nwaves * 2;
      for (int c = 0; c < cnt; ++c) sum += part[tid * PW + c];
      const float nrm = sqrtf(sum);
      const int sg = s0 + 64 * sc + tid;
      alpha[tid] = gscale[sg] / fmaxf(nrm, 1e-12f);
      if (block_norms) block_norms[(size_t)sg * K + k] = nrm;
    }
    __syncthreads();
    if (dvalid) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        if (mt == 1 && !two) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * mt + sv_frag_row(r, kk);
          if (row < Sc) {
            const float a = alpha[row];
            float4 v = make_float4(acc[mt][0][r] * a, acc[mt][1][r] * a, acc[mt][2][r] * a, acc[mt][3][r] * a);
            const size_t o = (size_t)(s0 + 64 * sc + row) * KD + (size_t)k * D + dcol;
            if (!PLANES || out != nullptr) *reinterpret_cast<float4*>(out + o) = v;
            if (PLANES) {
              typedef _Float16 h4 __attribute__((ext_vector_type(4)));
              const float f[4] = {(v.x - mu4.x) * xscale, (v.y - mu4.y) * xscale, (v.z - mu4.z) * xscale, (v.w - mu4.w) * xscale};
              h4 p1, p2;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                p1[e] = (_Float16)f[e];
                p2[e] = (_Float16)(f[e] - (float)p1[e]);
              }
              const size_t ob = sv_x3_off(s0 + 64 * sc + row, (int64_t)k * D + dcol, KD);   // blocked plane layout (ctx.h)
              *reinterpret_cast<h4*>(h1 + ob) = p1;
              *reinterpret_cast<h4*>(h2 + ob) = p2;
            }
          }
        }
      }
    }
    __syncthreads();
  }
  }
}

// (the token lists and their 1/||x|| are prep_kernel's label-grouped copies: ctx->s_tokorder, s_laboff, s_rnsorted)
int sv_launch_aggregate(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const float* centres, int K, int D,
                        const int32_t* seg_off_dev, const float* gscale, int B, int N, int SC, float* out, float* block_norms,
                        const float* mean, float xscale, uint16_t* h1, uint16_t* h2) {
  const int nwaves = (D + 127) / 128;
  if (nwaves > 12)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "aggregate: D=%d exceeds the 1536-wide workgroup of this build", D);
  const int Ncap = (N + 2) & ~1;
  const int PW = nwaves * 2 + 1;
  size_t lds = (size_t)Ncap * 16 + (size_t)(64 * PW + 64) * sizeof(float) + 16 * sizeof(int);
  lds = (lds + 15) & ~(size_t)15;
  lds += (size_t)nwaves * AGG_QD * 1024;   // DMA queue
  if (lds > 160 * 1024) return ctx->fail(SEGVLAD_ERR_LIMIT, "aggregate: N=%d tokens need %zu B of LDS (limit 160 KiB)", N, lds);
  auto kern = (h1 != nullptr) ? aggregate_kernel<true> : aggregate_kernel<false>;
  if (lds > 64 * 1024)
    SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), (size_t)lds));
  int kpb = ctx->opt.agg_kpb;   // clusters per workgroup
  if (kpb < 1) kpb = 1;
  hipLaunchKernelGGL(kern, dim3((K + kpb - 1) / kpb, B), dim3(nwaves * 64), lds, ctx->stream, xt, ctx->s_rnsorted.as<float>(),
                     ctx->s_tokorder.as<int32_t>(),
                     ctx->s_laboff.as<int32_t>(), colmask, centres, seg_off_dev,
                     gscale, N, D, K, SC, Ncap, out, block_norms, mean, xscale, reinterpret_cast<_Float16*>(h1),
                     reinterpret_cast<_Float16*>(h2), kpb);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
