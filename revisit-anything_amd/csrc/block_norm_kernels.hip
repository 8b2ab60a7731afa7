// Block norms and grouped token planes for gfx950 (MI355X): the D-space half of the PCA "project" form of the describe stage
// ("project then aggregate"; the P-space half is project_kernels.hip), which the headline path runs in the place of
// aggregate_kernel (vlad_kernels.hip).  One launcher, sv_launch_token_norms, deals an image's (image, cluster) tasks by their size:
//
//   gram_norms_kernel<1, 3>   tasks of <= 32 tokens: ||V_sk|| as a bit-masked quadratic form over the Gram matrix of the task's
//   gram_norms_kernel<2, 2>   residuals, 33 .. 64 tokens: three Gram tiles -- on the 16-bit matrix pipe, from the very fp16
//                             fragments that are the planes' bytes; a task whose residuals nearly cancel is flagged for the
//                             fp32 kernel (option tnk_gram, default on; D % 32 == 0)
//   token_norms_kernel<false> every other task (and the flagged ones): fp32 block sums on v_mfma_f32_32x32x2_f32, one wave per task
//   token_norms_kernel<true>  tasks of >= 256 tokens, whose lists do not fit the wave's LDS
//
// Every kernel also writes the fp16 planes of its tokens' residuals (x^_t - C_k) * xscale = h1 + h2, grouped by cluster, in the
// blocked layout the grouped GEMM reads (sv_x3_off, ctx.h).  Wave = 64 lanes, one wave per task, no barrier anywhere; tokens stream
// through wave-private queues of global->LDS DMAs under counted waits (mfma_f32_dev.h, waitcnt_dev.h), and the plane stores between two
// DMAs are part of the count.
#include "ctx.h"
#include "mfma_f32_dev.h"

// ---- fp32 block sums --------------------------------------------------------------------------------------------------------
// What segvlad_images_pca needs from the D-space when the projection runs per token: the block norms ||V_sk|| and the fp16
// planes of the token residuals x^_t - C_k(t), grouped by cluster.  No descriptor is stored, so nothing forces the workgroup-wide
// geometry of aggregate_kernel (12 waves side by side over D, two barriers per cluster): here ONE WAVE owns a whole
// (image, cluster) task and walks D in 128-column chunks, tokens streaming through a wave-private DMA queue that never
// drains between chunks; squared sums stay in registers until the task ends.  No barrier anywhere.
constexpr int TNK_QD = 8, TNK_LCAP = 256, TNK_WAVES = 4;

template <bool BIG>   // BIG: the (rare) clusters with >= TNK_LCAP tokens of one image, lists read from global memory step by step
__global__ __launch_bounds__(64 * TNK_WAVES, 2) void token_norms_kernel(const float* __restrict__ Xt, const float* __restrict__ rnorm,
                                                                    const int32_t* __restrict__ tok_order,
                                                                    const int32_t* __restrict__ lab_off,
                                                                    const uint64_t* __restrict__ colmask,
                                                                    const float* __restrict__ C,
                                                                    const int32_t* __restrict__ seg_off, int N, int D, int K, int SC,
                                                                    int Dpad, float* __restrict__ block_norms, float xscale,
                                                                    _Float16* __restrict__ h1, _Float16* __restrict__ h2,
                                                                    const int32_t* __restrict__ rowbase, int64_t dummy_row,
                                                                    int skip_le, const uint8_t* __restrict__ redo_task,
                                                                    const int32_t* __restrict__ phys) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, l = tid & 63, i = l & 31, kk = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = (int)blockIdx.x * TNK_WAVES + w;
  if (k >= K) return;   // (no barriers in this kernel)
  const size_t wsz = (size_t)TNK_QD * 1024 + (size_t)TNK_LCAP * 20 + (size_t)Dpad * 4;
  unsigned char* qbase = smem + (size_t)w * wsz;                                  // [QD][1 KiB] DMA queue
  uint64_t* mskl = reinterpret_cast<uint64_t*>(qbase + TNK_QD * 1024);            // [LCAP]
  int* tokl = reinterpret_cast<int*>(mskl + TNK_LCAP);                            // [LCAP]
  float* rnl = reinterpret_cast<float*>(tokl + TNK_LCAP);                         // [LCAP]
  int* rowl = reinterpret_cast<int*>(rnl + TNK_LCAP);                             // [LCAP] plane row of the token, -1: it has none
  float* cl = reinterpret_cast<float*>(rowl + TNK_LCAP);                          // [Dpad] centre k
  const int o0 = lab_off[(size_t)b * (K + 1) + k];
  const int n = lab_off[(size_t)b * (K + 1) + k + 1] - o0;
  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  const int SCb = (S + 63) >> 6;
  const int npairs = (n + 1) >> 1;
  const int nd = Dpad >> 7, total = nd * npairs;
  const size_t tb = (size_t)b * N + o0;
  if ((n >= TNK_LCAP) != BIG) return;   // the other instantiation's task
  // gram_norms_kernel's task (skip_le = -1: none) -- unless that kernel found one of the task's segments CANCELLING (redo_task)
  if (n <= skip_le && !(redo_task && n > 0 && redo_task[(size_t)b * K + k])) return;
  if (n == 0) {   // an empty cluster: zero norms, no rows
    for (int s = l; s < S; s += 64) block_norms[(size_t)(s0 + s) * K + k] = 0.f;
    return;
  }
  for (int d = 4 * l; d < Dpad; d += 256)
    *reinterpret_cast<float4*>(cl + d) = d < D ? *reinterpret_cast<const float4*>(C + (size_t)k * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr bool single = !BIG;   // the token list fits the wave's LDS lists
  // a token's plane row: rowbase + its rank among the task's covered tokens (prep_kernel's phys; -1: no segment covers it --
  // nothing reads its row, it has none)
  const int grow0 = rowbase[(size_t)b * K + k];
  if (single) {
    for (int j = l; j < n; j += 64) {
      tokl[j] = tok_order[tb + j];
      rnl[j] = rnorm[tb + j];
      const int ph = phys[tb + j];
      rowl[j] = ph >= 0 ? grow0 + ph : -1;
    }
    if (l == 0 && (n & 1)) {
      tokl[n] = 0;
      rnl[n] = 0.f;
      rowl[n] = -1;
    }
  }
  const size_t nkb_d = (size_t)(D >> 5);
  // lanes without a row store to the dummy tile (256 rows behind the planes; spread over its rows: one address would be a hot spot)
  const size_t ob_dummy = sv_x3_off((dummy_row < 0 ? -dummy_row : dummy_row) + ((64 * k + l) & 255), (4 * i) % D, D);
  const float* Xb = Xt + (size_t)b * N * D;

  for (int sc = 0; sc < SCb; ++sc) {
    if (single) {
      for (int j = l; j < n; j += 64) mskl[j] = colmask[(tb + j) * SC + sc];
      if (l == 0 && (n & 1)) mskl[n] = 0;
    }
    const int Sc = min(64, S - 64 * sc);
    const bool two = Sc > 32;
    f32x16 acc[2][4];
    float nsq[2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        nsq[a][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][q][r] = 0.f;
      }
    // step f = (chunk dc, pair p), dc-major; the DMA of step f + QD is issued when step f's slot has been read
    int idc = 0, ip = 0, fi = 0;   // issue cursor
    auto issue = [&]() {
      const int j = 2 * ip + kk;
      const int t = single ? sv_lds_read_i32(sv_lds_addr(tokl + j)) : (j < n ? tok_order[tb + j] : 0);
      const int dcol = idc * 128 + 4 * i;
      const float* src = dcol < D ? Xb + (size_t)t * D + dcol : Xt;   // lanes beyond D fetch a valid dummy address
      __builtin_amdgcn_global_load_lds((sv_gptr_t)src, (sv_lptr_t)(qbase + (fi % TNK_QD) * 1024), 16, 0, 0);
      ++fi;
      if (++ip == npairs) {
        ip = 0;
        ++idc;
      }
    };
    for (int q = 0; q < TNK_QD && q < total; ++q) issue();
    int f = 0;
    for (int dc = 0; dc < nd; ++dc) {
      const int dcol = dc * 128 + 4 * i;
      const bool dvalid = dcol < D;
      const f32x4 c4 = sv_lds_read_f32x4(sv_lds_addr(cl + dcol));
      const size_t kb_dc = (size_t)(dcol >> 5);                       // k-block of this lane's four columns
      const unsigned lane_c = (unsigned)((dcol & 31) >> 3), lane_o = (unsigned)(dcol & 7);
      for (int p = 0; p < npairs; ++p, ++f) {
        const int j = 2 * p + kk;
        float rn = 0.f;
        uint64_t m = 0ull;
        f32x4 x;
        int prw = -1;   // the token's plane row (first segment chunk)
        if (!single) {
          rn = j < n ? rnorm[tb + j] : 0.f;
          m = j < n ? colmask[(tb + j) * SC + sc] : 0ull;
          const int ph = (sc == 0 && j < n) ? phys[tb + j] : -1;
          prw = ph >= 0 ? grow0 + ph : -1;
        }
        // ops issued after step f's DMA: min(QD - 1, rem) later DMAs and, on the first segment chunk, two plane stores for
        // each of the last min(QD, f) steps (always issued: lanes without a valid element or without a row write the dummy tile)
        const int rem = total - 1 - f;
        if (single && dummy_row >= 0) {
          // steady state (a full queue behind and ahead): the count is the constant QD - 1 (+ 2 QD plane stores)
          if (f >= TNK_QD && rem >= TNK_QD - 1) {
            if (sc == 0) asm volatile("s_waitcnt vmcnt(23)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
          } else {
            sv_wait_vm((rem < TNK_QD - 1 ? rem : TNK_QD - 1) + (sc == 0 ? 2 * (f < TNK_QD ? f : TNK_QD) : 0));
          }
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // list entries come from global memory on this path
        }
        if (single)
          lds_step_read(sv_lds_addr(qbase + (f % TNK_QD) * 1024 + l * 16), sv_lds_addr(rnl + j), sv_lds_addr(mskl + j), x, rn, m);
        else
          x = sv_lds_read_f32x4(sv_lds_addr(qbase + (f % TNK_QD) * 1024 + l * 16));
        // (the slot has been read -- lgkmcnt(0) inside -- before it is refilled)
        if (fi < total) issue();
        if (!dvalid) x = f32x4{0.f, 0.f, 0.f, 0.f};
        const float b0 = fmaf(x.x, rn, -c4.x), b1 = fmaf(x.y, rn, -c4.y);
        const float b2 = fmaf(x.z, rn, -c4.z), b3 = fmaf(x.w, rn, -c4.w);
        if (sc == 0) {   // the residual's fp16 planes, grouped row grow0 + j
          typedef _Float16 h4 __attribute__((ext_vector_type(4)));
          const float fv[4] = {b0 * xscale, b1 * xscale, b2 * xscale, b3 * xscale};
          h4 p1, p2;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            p1[e] = (_Float16)fv[e];
            p2[e] = (_Float16)(fv[e] - (float)p1[e]);
          }
          // (the row list is read on the first chunk only; these stores are never predicated away: the counted waits count them)
          if (single) prw = sv_lds_read_i32(sv_lds_addr(rowl + j));
          const bool real = dvalid && prw >= 0;
          // sv_x3_off(row, dcol, D) with the lane / chunk constants of this 128-column chunk taken out of the loop
          const unsigned rr = (unsigned)prw;
          const size_t ob = real ? ((size_t)(rr >> 7) * nkb_d + kb_dc) * 4096 + (size_t)(((rr & 127u) << 5) + (((lane_c ^ (unsigned)sv_x3_swz(rr)) << 3) | lane_o))
                                 : ob_dummy;
          *reinterpret_cast<h4*>(h1 + ob) = p1;
          *reinterpret_cast<h4*>(h2 + ob) = p2;
        }
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
      // this chunk's 128 columns of every block row: square, add, restart the accumulators
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        if (mt == 1 && !two) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float q2 = nsq[mt][r];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            q2 = fmaf(acc[mt][q][r], acc[mt][q][r], q2);
            acc[mt][q][r] = 0.f;
          }
          nsq[mt][r] = q2;
        }
      }
    }
    // row sums over the 32 lanes of each half-wave (DPP inside the 16-lane rows, one cross-row exchange)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (mt == 1 && !two) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = nsq[mt][r];
        p = sv_dpp_row_sum(p);
        p += __shfl_xor(p, 16);
        const int row = 32 * mt + sv_frag_row(r, kk);
        if (i == 0 && row < Sc) block_norms[(size_t)(s0 + 64 * sc + row) * K + k] = sqrtf(p);
      }
    }
  }
}

// ---- block norms from the Gram matrix of a task's residuals (round 4) ---------------------------------------------------------
// ||sum_t m_t r_t||^2 = m^T (R R^T) m: a task (image, cluster) with n <= 32 tokens needs the n x n Gram matrix G of its token
// residuals -- ONE 32 x 32 accumulator tile instead of the 64 x 128 block sums of token_norms_kernel (128 accumulator registers,
// eight fp32 MFMAs per pair of tokens: that kernel is bound by the fp32 matrix pipe, 8 B/clk/CU of tokens) -- and, per segment,
// a bit-masked quadratic form over G.  G runs on the 16-bit pipe: the residuals are split r * xscale = h + l + e exactly as the
// planes want them (|e| <= 2^-22 |r|), G += l h^T + h l^T + h h^T with the A and B fragments being the SAME registers
// (v_mfma_f32_32x32x16_f16: lane (i, kk) holds token i, columns 8 kk .. 8 kk + 7 of a 16-column k-step), and those fragments
// are, byte for byte, the planes' 16-byte chunks.  One wave per task; tokens stream through a two-slot wave-private DMA queue,
// 32 tokens x 32 columns (4 KiB, four pieces of 8 tokens x 128 B, source-side swizzled: chunk ^ ((token >> 1) & 7)) per step.
// Tasks with more than 64 tokens of one image in one cluster stay with token_norms_kernel (skip_le).
// T = 2: tasks of 33 .. 64 tokens -- two token tiles, the three Gram tiles G00, G01, G11 (G10 = G01^T is not formed), 8 KiB per
// step and queue slot, two waves per workgroup.
constexpr int GNK_SLOT = 4096;   // one token tile of a step: 32 tokens x 128 B

template <int T, int QS>   // token tiles of a task, slots of the DMA queue (steps in flight + the one being read)
__global__ __launch_bounds__(T == 1 ? 256 : 128, 2) void gram_norms_kernel(const float* __restrict__ Xt, const float* __restrict__ rnorm,
                                                                         const int32_t* __restrict__ tok_order,
                                                                         const int32_t* __restrict__ lab_off,
                                                                         const uint64_t* __restrict__ colmask,
                                                                         const float* __restrict__ C,
                                                                         const int32_t* __restrict__ seg_off, int N, int D, int K, int SC,
                                                                         float* __restrict__ block_norms, float xscale,
                                                                         _Float16* __restrict__ h1, _Float16* __restrict__ h2,
                                                                         const int32_t* __restrict__ rowbase, int safe_waits,
                                                                         uint8_t* __restrict__ redo_task,
                                                                         const int32_t* __restrict__ phys, int64_t dummy_row) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
  constexpr int WAVES = T == 1 ? 4 : 2;
  constexpr int NG = T * (T + 1) / 2;   // Gram tiles held: (0,0) | (0,0), (0,1), (1,1)
  const int b = blockIdx.y;
  const int tid = threadIdx.x, l = tid & 63, i = l & 31, kk = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = (int)blockIdx.x * WAVES + w;
  if (k >= K) return;   // (no barriers in this kernel)
  const size_t wsz = (size_t)QS * T * GNK_SLOT + (size_t)D * 4;
  unsigned char* qbase = smem + (size_t)w * wsz;                      // [QS][T x 4 KiB] DMA queue
  float* cl = reinterpret_cast<float*>(qbase + QS * T * GNK_SLOT);    // [D] centre k
  const int o0 = lab_off[(size_t)b * (K + 1) + k];
  const int n = lab_off[(size_t)b * (K + 1) + k + 1] - o0;
  if (n > 32 * T || (T == 2 && n <= 32)) return;   // the other instantiation's / token_norms_kernel's task
  const int s0 = seg_off[b], S = seg_off[b + 1] - s0;
  if (n == 0) {   // an empty cluster: zero norms, no rows
    for (int s = l; s < S; s += 64) block_norms[(size_t)(s0 + s) * K + k] = 0.f;
    return;
  }
  const size_t tb = (size_t)b * N + o0;
  for (int d = 4 * l; d < D; d += 256) *reinterpret_cast<float4*>(cl + d) = *reinterpret_cast<const float4*>(C + (size_t)k * D + d);
  bool real[T];
  float rn[T];
#pragma unroll
  for (int tt = 0; tt < T; ++tt) {
    real[tt] = 32 * tt + i < n;
    rn[tt] = real[tt] ? rnorm[tb + 32 * tt + i] : 0.f;
  }
  const float* Xb = Xt + (size_t)b * N * D;
  // DMA sources of this lane: piece pz = tokens 8 pz .. 8 pz + 7, lane -> token 8 pz + (l >> 3), LDS position l & 7
  const float* src[4 * T];
#pragma unroll
  for (int pz = 0; pz < 4 * T; ++pz) {
    const int jj = 8 * pz + (l >> 3);
    const int t = jj < n ? tok_order[tb + jj] : tok_order[tb];   // (rows beyond n: a valid address, never used)
    src[pz] = Xb + (size_t)t * D + 4 * ((l & 7) ^ ((jj >> 1) & 7));
  }
  const int steps = D >> 5;
  // only the pieces that hold a token are requested (NP of them, wave-uniform), and of the last one only its tokens' lanes: a task
  // holds ~24 of its tile's 32 rows on average
  const int NP = (n + 7) >> 3;
  auto issue = [&](int f) {
#pragma unroll
    for (int pz = 0; pz < 4 * T; ++pz)
      if (pz < NP) {   // (wave-uniform: the instruction is issued, and counted, exactly NP times per step)
        if (8 * pz + (l >> 3) < n)
          __builtin_amdgcn_global_load_lds((sv_gptr_t)(src[pz] + 32 * f), (sv_lptr_t)(qbase + (f % QS) * (T * GNK_SLOT) + pz * 1024), 16, 0, 0);
      }
  };
#pragma unroll
  for (int q = 0; q < QS; ++q)
    if (q < steps) issue(q);
  f32x16 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
  size_t prow[T];
  unsigned pswz[T];
#pragma unroll
  for (int tt = 0; tt < T; ++tt) {
    // this lane's row of the grouped planes: rowbase + the token's rank among the task's covered tokens (prep_kernel's phys).  A
    // token no segment covers has no row -- nothing reads it -- and stores to the dummy tile behind the planes (spread over its 256
    // rows), NOT nowhere: a tile whose tokens are all uncovered would skip the store instruction, and the counted waits count it
    const int ph = real[tt] ? phys[tb + 32 * tt + i] : 0;
    const int64_t rr = ph >= 0 ? (int64_t)rowbase[(size_t)b * K + k] + ph : dummy_row + ((32 * (k + tt) + i) & 255);
    prow[tt] = (size_t)(rr >> 7) * (size_t)(D >> 5) * 4096 + (size_t)(rr & 127) * 32;
    pswz[tt] = (unsigned)sv_x3_swz(rr);
  }
  const unsigned fsw = (unsigned)((i >> 1) & 7);
  const unsigned a_tok = sv_lds_addr(qbase) + (unsigned)i * 128u;
  for (int f = 0; f < steps; ++f) {
    // the DMAs of step f have landed: behind them were issued, for each of the QS - 1 steps in between, 4 T plane stores and NP
    // DMAs, and the 4 T stores of step f - 1 (loads and stores retire in issue order)
    // (safe_waits: the development switch debug_search = 7 -- everything, at every step; the test compares the two bit for bit)
    if (f >= QS && f + QS - 1 < steps && !safe_waits) sv_wait_vm(QS * 4 * T + (QS - 1) * NP);   // (<= 23 by the helper: stricter beyond)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f32x4 x[T][4], c[4];
    {
      const unsigned ac = sv_lds_addr(cl) + (unsigned)(32 * f + 8 * kk) * 4u;
      // chunks 2 kk, 2 kk + 1 (k-step 0) and 4 + 2 kk, 5 + 2 kk (k-step 1) of token i, at their swizzled positions
      const unsigned p0 = ((unsigned)(2 * kk) ^ fsw) << 4, p1 = ((unsigned)(2 * kk + 1) ^ fsw) << 4;
      const unsigned p2 = ((unsigned)(4 + 2 * kk) ^ fsw) << 4, p3 = ((unsigned)(5 + 2 * kk) ^ fsw) << 4;
#pragma unroll
      for (int tt = 0; tt < T; ++tt) {
        const unsigned a0 = a_tok + (unsigned)(f % QS) * (T * GNK_SLOT) + (unsigned)tt * GNK_SLOT;
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7"
                     : "=&v"(x[tt][0]), "=&v"(x[tt][1]), "=&v"(x[tt][2]), "=&v"(x[tt][3])
                     : "v"(a0 + p0), "v"(a0 + p1), "v"(a0 + p2), "v"(a0 + p3)
                     : "memory");
      }
      asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:64\n\tds_read_b128 %3, %4 offset:80\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3])
                   : "v"(ac)
                   : "memory");
#pragma unroll
      for (int tt = 0; tt < T; ++tt) asm volatile("" : "+v"(x[tt][0]), "+v"(x[tt][1]), "+v"(x[tt][2]), "+v"(x[tt][3]));   // (final behind the wait)
    }
    if (f + QS < steps) issue(f + QS);   // the slot has been read
    asm volatile("" ::: "memory");     // (the plane stores below stay behind these DMAs: the counted wait relies on the order)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f16x8 hh[T], ll[T];
#pragma unroll
      for (int tt = 0; tt < T; ++tt) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xv = x[tt][2 * ks + (e >> 2)][e & 3], cv = c[2 * ks + (e >> 2)][e & 3];
          const float fv = real[tt] ? fmaf(xv, rn[tt], -cv) * xscale : 0.f;
          hh[tt][e] = (_Float16)fv;
          ll[tt][e] = (_Float16)(fv - (float)hh[tt][e]);
        }
        // the planes' 16-byte chunk (row, columns 32 f + 16 ks + 8 kk ..): issued by every step (the counted waits above;
        // lane 0 of tile 0 is always a real token, tile 1 of a T = 2 task always holds one)
        const size_t ob = prow[tt] + (size_t)f * 4096 + (size_t)((((unsigned)(2 * ks + kk)) ^ pswz[tt]) << 3);
        if (real[tt]) {
          *reinterpret_cast<f16x8*>(h1 + ob) = hh[tt];
          *reinterpret_cast<f16x8*>(h2 + ob) = ll[tt];
        }
      }
      // G(a, b) += l_a h_b^T + h_a l_b^T + h_a h_b^T, small terms first
#pragma unroll
      for (int ta = 0, g = 0; ta < T; ++ta)
#pragma unroll
        for (int tb2 = ta; tb2 < T; ++tb2, ++g) {
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ll[ta], hh[tb2], acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hh[ta], ll[tb2], acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hh[ta], hh[tb2], acc[g], 0, 0, 0);
        }
    }
  }
  // ---- per segment: m^T G m over this lane's 16 entries G(a, b)[sv_frag_row(r, kk)][i] of every tile, then across the wave ------
  // CANCELLATION: the quadratic form carries ~n 2^-22 of the COVERED DIAGONAL sum_t m_t G_tt, not of its own value;
  // when a segment's residuals nearly cancel (m^T G m << the diagonal sum) that is no longer small against the norm it divides
  // by.  Such a task is flagged (redo_task) and token_norms_kernel recomputes it with the fp32 block sums, which have no such
  // term (1/16: relative error of the norm <= ~1e-4 at 64 tokens on this side of the threshold).
  float dgl[T];   // this lane's diagonal entry G_tt of token 32 tt + i, if the lane holds it (one of the two half-waves does)
#pragma unroll
  for (int tt = 0; tt < T; ++tt) {
    dgl[tt] = 0.f;
    const int gd = tt == 0 ? 0 : NG - 1;   // tiles (0,0) and (T-1,T-1)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (sv_frag_row(r, kk) == i) dgl[tt] = acc[gd][r];
  }
  bool cancels = false;
  const float inv_x2 = 1.f / (xscale * xscale);
  const int SCb = (S + 63) >> 6;
  for (int sc = 0; sc < SCb; ++sc) {
    const int Sc = min(64, S - 64 * sc);
    uint64_t mt[T];
#pragma unroll
    for (int tt = 0; tt < T; ++tt) mt[tt] = real[tt] ? colmask[(tb + 32 * tt + i) * SC + sc] : 0ull;   // (lanes 32..63 repeat lanes 0..31)
    for (int s = 0; s < Sc; ++s) {
      uint32_t W[T];   // bit t: token 32 tt + t covered by segment s
      bool any = false;
#pragma unroll
      for (int tt = 0; tt < T; ++tt) {
        W[tt] = (uint32_t)__builtin_amdgcn_ballot_w64(((mt[tt] >> s) & 1ull) != 0ull);
        any |= W[tt] != 0u;
      }
      float p = 0.f;
      if (any) {   // (wave-uniform)
#pragma unroll
        for (int ta = 0, g = 0; ta < T; ++ta)
#pragma unroll
          for (int tb2 = ta; tb2 < T; ++tb2, ++g) {
            float q = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) q += ((W[ta] >> sv_frag_row(r, kk)) & 1u) ? acc[g][r] : 0.f;
            q = ((W[tb2] >> i) & 1u) ? q : 0.f;
            p += (ta == tb2) ? q : 2.f * q;   // the off-diagonal tile stands for its transpose as well
          }
        p = sv_dpp_row_sum(p);
        p += __shfl_xor(p, 16);
        p += __shfl_xor(p, 32);
        float dg = 0.f;   // the covered diagonal
#pragma unroll
        for (int tt = 0; tt < T; ++tt) dg += ((W[tt] >> i) & 1u) ? dgl[tt] : 0.f;
        dg = sv_dpp_row_sum(dg);
        dg += __shfl_xor(dg, 16);
        dg += __shfl_xor(dg, 32);
        cancels = cancels || (p < 0.0625f * dg);
      }
      if (l == 0) block_norms[(size_t)(s0 + 64 * sc + s) * K + k] = sqrtf(fmaxf(p, 0.f) * inv_x2);
    }
  }
  if (cancels && l == 0 && redo_task) redo_task[(size_t)b * K + k] = 1;   // (wave-uniform: p and dg are wave sums)
}

int sv_launch_token_norms(segvlad_ctx* ctx, const float* xt, const uint64_t* colmask, const float* centres, int K, int D,
                          const int32_t* seg_off_dev, int B, int N, int SC, float* block_norms, float xscale, uint16_t* h1,
                          uint16_t* h2, const int32_t* rowbase, int64_t dummy_row, const int32_t* phys) {
  if (D % 4) return ctx->fail(SEGVLAD_ERR_ARG, "token_norms: D=%d must be a multiple of 4", D);
  const int Dpad = (D + 127) & ~127;
  const size_t lds = (size_t)TNK_WAVES * ((size_t)TNK_QD * 1024 + (size_t)TNK_LCAP * 20 + (size_t)Dpad * 4);
  if (lds > 160 * 1024) return ctx->fail(SEGVLAD_ERR_LIMIT, "token_norms: D=%d needs %zu B of LDS", D, lds);
  // tasks of <= 64 tokens: the Gram kernels (option tnk_gram, default on; D a multiple of 32); the rest: the block-sum kernels
  const bool gram = ctx->opt.tnk_gram != 0 && (D % 32) == 0;
  const int skip_le = gram ? 64 : -1;
  uint8_t* redo_task = nullptr;   // [B][K]: Gram tasks with a cancelling segment, recomputed by the block-sum kernel below
  if (gram) {
    SV_HIP(ctx->s_tnk_redo.reserve((size_t)B * K));
    redo_task = ctx->s_tnk_redo.as<uint8_t>();
    SV_HIP(hipMemsetAsync(redo_task, 0, (size_t)B * K, ctx->stream));
    // the two-tile tasks are few (6 % of the tokens at 24 per cluster): their launch is one task's latency with most of the chip
    // idle -- on the context's side stream it runs beside the one-tile launch instead of in front of it (tnk_fork)
    const bool fork = N > 32 && ctx->opt.tnk_fork != 0;
    if (fork) SV_TRY(sv_fork_side(ctx));
    for (int T = 2; T >= 1; --T) {
      if (T == 2 && N <= 32) continue;
      const int waves = T == 1 ? 4 : 2;
      const int qs = T == 1 ? 3 : 2;   // (three slots of 4 KiB, or two of 8)
      const size_t glds = (size_t)waves * ((size_t)qs * T * GNK_SLOT + (size_t)D * 4);
      auto gk = T == 1 ? gram_norms_kernel<1, 3> : gram_norms_kernel<2, 2>;
      if (glds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(gk), glds));
      hipLaunchKernelGGL(gk, dim3((K + waves - 1) / waves, B), dim3(64 * waves), glds, (T == 2 && fork) ? ctx->side : ctx->stream, xt,
                         ctx->s_rnsorted.as<float>(), ctx->s_tokorder.as<int32_t>(), ctx->s_laboff.as<int32_t>(), colmask, centres,
                         seg_off_dev, N, D, K, SC, block_norms, xscale, reinterpret_cast<_Float16*>(h1),
                         reinterpret_cast<_Float16*>(h2), rowbase, dummy_row < 0 ? 1 : 0, redo_task, phys,
                         dummy_row < 0 ? -dummy_row : dummy_row);
      SV_HIP(hipGetLastError());
    }
    if (fork) SV_TRY(sv_join_side(ctx));
  }
  for (int big = 0; big < 2; ++big) {
    if (big && N < TNK_LCAP) break;
    auto kern = big ? token_norms_kernel<true> : token_norms_kernel<false>;
    if (lds > 64 * 1024)
      SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), (size_t)lds));
    hipLaunchKernelGGL(kern, dim3((K + TNK_WAVES - 1) / TNK_WAVES, B), dim3(64 * TNK_WAVES), lds, ctx->stream, xt,
                       ctx->s_rnsorted.as<float>(), ctx->s_tokorder.as<int32_t>(), ctx->s_laboff.as<int32_t>(), colmask, centres,
                       seg_off_dev, N, D, K, SC, Dpad, block_norms, xscale, reinterpret_cast<_Float16*>(h1),
                       reinterpret_cast<_Float16*>(h2), rowbase, dummy_row, skip_le, redo_task, phys);
    SV_HIP(hipGetLastError());
  }
  return SEGVLAD_OK;
}
