// The gathered-row exact-distance tile: <= 64 consecutive query rows x 128 index rows named by an id list, per pair the sequential
// fp32 chain acc = fma(q[k], r[k], acc), k = 0 .. d - 1, from acc = 0, on v_mfma_f32_32x32x2_f32 in k order -- bit for bit the chain
// of refine_exact_kernel and of the distance-matrix path (gemm_kernels.hip: same instruction, same k order).  One definition for the
// three kernels that evaluate it (refine_group_gemm_kernel, sl_gemm_kernel, mp_gemm_kernel): how the id list is filled and what becomes
// of the dot products is theirs, the chain between is this file's, so that "the same bits on every path" holds by construction.
//
// Workgroup: 256 threads, wave w owns 32 index rows (MT = 1 or 2 accumulator tiles of 32 x 32: groups of <= 32 / <= 64 query rows),
// the query rows are shared through LDS.  d % 32 == 0, Q and R 16-byte aligned.
//
// Every row is fetched in pieces of KS floats (128 B): one load instruction of a wave covers eight rows x 128 contiguous
// bytes.  A super-tile of KS k travels in ONE register stage ((MT + 4) x 4 / 4 sixteen-byte loads per thread, in flight
// while the previous super-tile is multiplied out of LDS) and is parked in a single LDS buffer between two barriers; with
// 27 KiB of LDS a CU holds five workgroups, which hide each other's load / store / barrier phases.  (Measured, 200 groups of
// 200-row unions: 512-byte pieces and one workgroup per CU 8.63 ms at d = 98 304 / 0.384 ms at d = 1024, 256-byte pieces
// 7.70 / 0.378, 128-byte pieces 7.51 / 0.362.)  The loads are inline asm with an explicit wait: a compiler-visible load with
// a condition on it makes every LDS access behind it wait for all of them.
// LDS image: ROW-major, row stride KS + 4 floats, and inside every group of 8 k the even k first, then the odd:
// [k0 k2 k4 k6 | k1 k3 k5 k7].  v_mfma_f32_32x32x2_f32 takes k = 2 s from lanes 0-31 and k = 2 s + 1 from lanes 32-63, so a
// lane's operands of FOUR consecutive k-steps are one aligned 16-byte read (rows 16 apart share a bank group, which the
// 16-lane service groups of a ds_read_b128 never hold together), and a loaded float4 goes out as two 8-byte writes.
// (Measured on the way, 10 000 x 200-row bands of 98 304-d rows: k-major [k][row] tiles fed by ds_read_b32 -- one or two reads,
//  a wait and one or two MFMAs per k-step, one wave per SIMD -- 63 ms with the matrix pipes 8 % busy: a chain of LDS latencies,
//  half of the LDS cycles bank conflicts of the transposing 4-byte stores; 128-byte row pieces three tiles ahead: 32-40 ms.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "mfma_f32_dev.h"   // f32x16, f32x4, f32x2, sv_frag_row

constexpr int SV_GT_KS = 32;   // floats of a row piece = k of a super-tile

template <int MT>
struct SvGroupTile {
  static constexpr int KS = SV_GT_KS;
  static constexpr int LDR = KS + 4;         // row stride of the LDS image
  static constexpr int LPR = KS / 4;         // lanes (16-byte loads) per row piece
  static constexpr int RPI = 64 / LPR;       // rows per load instruction of a wave
  static constexpr int NR = 32 * MT + 128;   // rows of a super-tile: the group's query rows, then 128 index rows
  static constexpr int NLD = NR / (4 * RPI); // 16-byte loads per thread and super-tile
  static_assert(MT == 1 || MT == 2, "groups of <= 32 or <= 64 query rows");
  static_assert(NR % (4 * RPI) == 0 && (32 * MT) % (4 * RPI) == 0, "whole instructions of query rows / of index rows");
};
// bytes of the LDS image [NR][LDR] (host and device)
constexpr size_t sv_group_tile_bytes(int mt) { return (size_t)(32 * mt + 128) * (SV_GT_KS + 4) * 4; }

// The row pieces are requested by inline asm and waited for by a hand-placed s_waitcnt: the compiler takes the destination
// registers for defined when the asm statement ends, so nothing but today's register allocation keeps it from copying or spilling
// them between the request and the wait.  That form is therefore tied to the toolchain it was verified on -- ISA
// inspected, and tests/test_gpu_refine_group.py, test_gpu_shortlist.py and test_gpu_match.py hold the kernels to the per-row
// kernels' bits: AMD clang 22 (ROCm 7.2).  Any other compiler gets plain loads, whose waits it places itself (measured slower: it
// waits for every outstanding load in front of every LDS access behind a conditional load -- but correct by construction).
// -DSEGVLAD_RG_PLAIN_LOADS forces that form.
#if defined(__clang_major__) && __clang_major__ == 22 && !defined(SEGVLAD_RG_PLAIN_LOADS)
#define SV_GT_GLOAD(dst, ptr) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(ptr) : "memory")
#define SV_GT_WAIT_LOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define SV_GT_GLOAD(dst, ptr) (dst) = *reinterpret_cast<const f32x4*>(ptr)
#define SV_GT_WAIT_LOADS() do { } while (0)
#endif

// The loads of a thread: load j stages row rr = 4 RPI j + RPI w + lr of the super-tile (the group's 32 MT query rows, then the 128
// index rows), floats 4 lp .. + 3 of it.  What a thread reads of Q does not depend on the id list: a kernel that walks several
// 128-row tiles per group takes these pointers ONCE, in front of its tile loop.
template <int MT>
struct SvGroupTileQ {
  // load j's query row (rows beyond the group repeat row q_end - 1: ignored by the caller); the entries of the loads that stage
  // index rows are never read and cost nothing
  const float* row[SvGroupTile<MT>::NLD];
};
template <int MT>
__device__ __forceinline__ SvGroupTileQ<MT> sv_group_tile_query_rows(const float* Q, int d, int q0, int q_end) {
  using GT = SvGroupTile<MT>;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  SvGroupTileQ<MT> q;
#pragma unroll
  for (int j = 0; j < GT::NLD; ++j) q.row[j] = Q + (size_t)min(q0 + 4 * GT::RPI * j + GT::RPI * w + l / GT::LPR, q_end - 1) * d;
  return q;
}

// acc[t][r] = the chain of query row q0 + 32 t + sv_frag_row(r, lane >> 5) with index row ids[32 wave + (lane & 31)].
// Called by all 256 threads of the workgroup.  tile: LDS, sv_group_tile_bytes(MT), 16-byte aligned; ids: LDS [128], every entry a
// valid row of R (a caller pads the columns it does not have with a valid row and ignores them); qrows: sv_group_tile_query_rows
// of the group.
// Barriers: ON ENTRY the caller has made ids[] visible with a barrier (and every wave is done with whatever `tile` held); ON RETURN
// every wave has finished reading `tile`, so the caller may overwrite it at once -- ids[] it may only rewrite behind a barrier of
// its own, the lanes' epilogues read it.
template <int MT>
__device__ __forceinline__ void sv_group_tile_dots(float* tile, const uint32_t* ids, const SvGroupTileQ<MT>& qrows, const float* R,
                                                   int d, f32x16 (&acc)[MT]) {
  using GT = SvGroupTile<MT>;
  constexpr int KS = GT::KS, LDR = GT::LDR, LPR = GT::LPR, RPI = GT::RPI, NLD = GT::NLD;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  const int lp = l % LPR, lr = l / LPR;   // loader coordinates: 16-byte piece of a row, row of the instruction
  const float* src[NLD];
#pragma unroll
  for (int j = 0; j < NLD; ++j) {
    const int rr = 4 * RPI * j + RPI * w + lr;
    src[j] = (rr < 32 * MT ? qrows.row[j] : R + (size_t)ids[rr - 32 * MT] * d) + 4 * lp;
  }
  f32x4 v[NLD];
  auto gload = [&](int st) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) SV_GT_GLOAD(v[j], src[j] + (size_t)st * KS);
  };
  // floats 4 lp .. 4 lp + 3 = k-group lp >> 1, half lp & 1: the even k to slots 2 (lp & 1) .. + 1, the odd k four slots further
  float* st_base = tile + (RPI * w + lr) * LDR + 8 * (lp >> 1) + 2 * (lp & 1);
  auto sstore = [&]() {
#pragma unroll
    for (int j = 0; j < NLD; ++j) asm volatile("" : "+v"(v[j]));   // (the values exist from HERE on: behind the caller's wait; the
                                                                   //  re-packing moves below are not memory operations)
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      float* p = st_base + 4 * RPI * j * LDR;
      f32x2 ev, od;
      ev[0] = v[j][0];
      ev[1] = v[j][2];
      od[0] = v[j][1];
      od[1] = v[j][3];
      *reinterpret_cast<f32x2*>(p) = ev;
      *reinterpret_cast<f32x2*>(p + 4) = od;
    }
  };
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* a_frag = tile + i * LDR + 4 * kk;                       // + 32 t rows, + 8 g floats
  const float* b_frag = tile + (32 * MT + 32 * w + i) * LDR + 4 * kk;
  const int nst = d / KS;
  gload(0);
  SV_GT_WAIT_LOADS();
  sstore();
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    if (st + 1 < nst) gload(st + 1);   // in flight while this super-tile is multiplied
    // KS / 8 groups of 8 k; the fragments of group g + 1 are requested before the MFMAs of group g are issued
    f32x4 fa[2][MT], fb[2];
    fb[0] = *reinterpret_cast<const f32x4*>(b_frag);
#pragma unroll
    for (int t = 0; t < MT; ++t) fa[0][t] = *reinterpret_cast<const f32x4*>(a_frag + 32 * t * LDR);
#pragma unroll
    for (int g = 0; g < KS / 8; ++g) {
      if (g + 1 < KS / 8) {
        fb[(g + 1) & 1] = *reinterpret_cast<const f32x4*>(b_frag + 8 * (g + 1));
#pragma unroll
        for (int t = 0; t < MT; ++t) fa[(g + 1) & 1][t] = *reinterpret_cast<const f32x4*>(a_frag + 32 * t * LDR + 8 * (g + 1));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][t][u], fb[g & 1][u], acc[t], 0, 0, 0);
    }
    __syncthreads();   // every wave is done with the LDS image
    if (st + 1 < nst) {
      SV_GT_WAIT_LOADS();
      sstore();
      __syncthreads();
    }
  }
}
