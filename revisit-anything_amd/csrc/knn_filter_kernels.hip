// Exact kNN, large-database path: the fp16 candidate FILTER, the default filter of segvlad_search (gfx950).
//
//   knn_f16_filter_kernel<C>  one fp16 MFMA product per fp32 fma; one configuration type C per kernel the library holds (F16BatchDefault,
//                             F16DeepFlush, ...: 14, and three probes in the development build)
//   launch_f16_filter<C>      its launch: the walk's geometry from f16_walk.h, the LDS bytes from F16Lds<C>, the flush scratch
//   sv_choose_f16_kernel      which kernel a launch takes: the ONE place that knows the rule; f16_with_config maps the choice to its type
//   sv_launch_f16_filter      the entry; sv_f16_filter_skip_ok and sv_f16_eps_kblock ask the same rule
// (operand planes and scales: knn_operand_kernels.hip; the bf16x3 filter for d % 64 != 0: knn_bf16_filter_kernels.hip; what happens to the
//  candidate lists: knn_select_kernels.hip, knn_refine_kernels.hip)
#include <stdio.h>

#include "ctx.h"
#include "f16_walk.h"
#include "knn_dev.h"
#include "mfma_f32_dev.h"

// One fp16 MFMA product per fp32 fma: x~ = fl16(s * x) with a power-of-two scale s (exact), products of two
// fp16 are exact in fp32, so   |dot~ - dot| <= (2^-10 + 2^-22 + 2 d 2^-24) ||q|| ||r||   against the fp32 chain.
// The margin is ~24x wider than bf16x3's, which lets ~1.3-1.4x more candidates through (they are cheap: the
// exact refinement only sees the ~k survivors) for one third of the MFMA work.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#define MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

// Operand tiles go global -> LDS directly (global_load_lds_dwordx4, no VGPR staging, no ds_write): one
// wave-instruction fills 1 KiB of the LDS image, lane l landing at base + 16 l, i.e. RP = 1024 / row_bytes rows
// of HBK fp16.  The LDS image must be lane-linear, so the bank-conflict swizzle is applied on the SOURCE side:
// the lane that owns physical chunk p of row r fetches logical chunk p ^ f(r), and the MFMA fragment reads apply
// the same involution (f(r) = (r >> 1) & 7 for the 128-byte rows of a k-tile: a 16-lane ds_read_b128 group then covers
// all 16 bank slots).
//   BM x BN tile, WM x WN waves, HBK = 64 k per tile, two A stages (queries: L2 resident) and NB = 3 B stages (database
//   rows stream from HBM/MALL; their DMA runs two k-tiles ahead via a counted vmcnt).
// PROBE == 1 (development build): phase timing (s_memtime of wave 0 at the phase boundaries, summed over workgroups; f16_cfg = 93 prints it)
__device__ unsigned long long sv_f16_phase_cycles[8];
#define SV_PHASE(k)                                                                          \
  if (PROBE == 1) {                                                                          \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                            \
    if (threadIdx.x == 0) atomicAdd(&sv_f16_phase_cycles[k], now_ - phase_t0);               \
    phase_t0 = now_;                                                                         \
  }

// fire-and-forget fp32 add at L2 (`global_atomic_add_f32` without return: no register, no wait)
__device__ __forceinline__ void sv_atomic_add_noret(float* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)__builtin_amdgcn_global_atomic_fadd_f32((__attribute__((address_space(1))) float*)p, v);
#else
  (void)p;
  (void)v;
#endif
}

// The members of a configuration type (below: one type per kernel the library holds):
// POL: cache policy of the operand DMA (never changes a result): 1 = database rows (B) non-temporal
// PP : 0 = every wave runs the k-tile as one segment (one barrier per k-tile); 2 = "ping-pong": the k-tile is cut
//      into two phases of [load segment: LDS fragment reads + DMA issue][barrier][MFMA segment][barrier], and the second
//      half of the waves (the SIMD partners of the first half: waves w and w + NW/2 share a SIMD) runs one barrier
//      behind, so that on every SIMD one wave feeds the matrix pipe while its partner reads LDS and issues DMA.
// KBT: > 0 = BLOCKED accumulation (deep rows, e.g. raw K*D = 98 304-d descriptors): every KBT k-tiles the MFMA accumulators
//      are added into a second register set and cleared, so that the fp32 accumulation error of a dot product is bounded
//      by (2 KBT HBK + d / (KBT HBK)) 2^-24 sum|q_i r_i| instead of 2 d 2^-24 sum|q_i r_i| -- whatever the matrix pipe's
//      internal summation order is (see sv_f16_c_eps).  Needs the plain loop (PP == 0) and a second set of accumulators.
// BIAS: the accumulators START at -||r||^2 / 2 (in the scaled domain) instead of 0, so that at the end of the k-loop they
//      hold dot - ||r||^2 / 2 -- the quantity the epilogue screens -- and the per-element subtraction of pass 1 (four of its
//      seven VALU instructions per four elements) disappears; d2~ = ||q||^2 - 2 acc / scale.  The column norms are fetched
//      ahead of the tile (before the head DMA; PERSIST: before the previous tile's epilogue).  The running sums are up to
//      1.5 x larger in magnitude, which sv_f16_c_eps accounts for.
// EPI : epilogue.  0 = workgroup-level (one global atomic per row and tile); 1 = wave-private (see the epilogue)
// MF  : MFMA shape.  0 = v_mfma_f32_32x32x16_f16 (wave tile = TM x TN tiles of 32 x 32); 1 = v_mfma_f32_16x16x32_f16 (the same
//      64 x 128 wave tile as 4 x 8 tiles of 16 x 16, a k-step of 32): the same flops, LDS fragment bytes and accumulator
//      registers, but a QUARTER of the accumulator read-modify-write traffic per flop inside the matrix pipe.  The chip is
//      power-limited on this kernel (tools/ubench/mfma_peak: random operands sustain 1.71-1.76 PF in the 32 x 32 x 16 shape
//      and 1.92-2.01 PF in the 16 x 16 x 32 shape, MFMA only), so the shape that needs less energy per flop is the faster one.
// The buffer-resource type and its two builtins exist in the DEVICE pass only; the host pass, which parses the kernel bodies
// too (and silently drops a kernel's launch stub when its body does not type-check there), sees inert stand-ins.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t sv_rsrc_t;
#define SV_BUF_RSRC(base) __builtin_amdgcn_make_buffer_rsrc((void*)(base), 0, (int)0xffffffffu, 0x00020000)
#define SV_BUF_LOAD_LDS(rs, ldsptr, voff, soff, aux) __builtin_amdgcn_raw_ptr_buffer_load_lds((rs), (ldsptr), 16, (voff), (soff), 0, (aux))
#else
typedef int sv_rsrc_t;
#define SV_BUF_RSRC(base) 0
#define SV_BUF_LOAD_LDS(rs, ldsptr, voff, soff, aux) ((void)(rs), (void)(ldsptr), (void)(voff), (void)(soff))
#endif

// KFL : > 0 = blocked accumulation WITHOUT a second register set (deep rows on the 256 x 256 ping-pong kernel, whose 128 accumulators
//      per lane leave no room for one): every KFL k-tiles a wave ADDS its accumulators into its own slice of a global scratch
//      (kscr: [workgroup][wave][128][64 lanes] fp32, all zero between tiles) with non-returning `global_atomic_add_f32` -- fire and
//      forget: no temporary registers, no wait, the fp32 additions happen in L2, one address is only ever touched by one lane, in
//      program order -- and clears them; behind the last k-tile the rest is added too, the totals are read back INTO the accumulator
//      registers (system-coherent loads: the lines of the previous tile may sit in this CU's vector cache) and the slice is zeroed
//      for the next tile.  Error: sv_f16_c_eps with kb = KFL x HBK (the L2's additions are the "block sums" of that bound).
// BUF : the operand DMA as `buffer_load_dwordx4 ... lds` -- an SGPR resource per operand and tile, ONE never-rewritten 32-bit
//      VGPR offset per piece, the k-offset in an SGPR -- instead of `global_load_lds_dwordx4` on a 64-bit per-lane pointer that
//      every piece re-forms in the same VGPR pair (a write-after-read stall behind the previous piece's address read).  Needs
//      every piece offset of a tile below 4 GiB (the launcher checks).  tools/ubench/mfma_peak: 1317 -> 1345 TF for the loop
//      of this kernel's byte : flop ratio; the deep-row kernel 126.4 -> 125.2 ms; the ping-pong batch kernel 18.19 -> 18.70 ms
//      (slower: its default stays global_load_lds).
// ---- the kernels the library holds: one configuration type per kernel, variants derived from their base ----------------
// (every kernel: k-tiles of SV_F16_HBK = 64, SV_F16_NB = 3 database stages, wave tiles of 64 rows.  The variants that were
//  measured on the way and not kept -- other tile shapes, 32-deep k-tiles, a software-pipelined loop, other DMA placements --
//  are described in DESIGN.md 4 / 7 with their numbers.)
constexpr int SV_F16_NB = 3;   // (SV_F16_HBK: f16_walk.h)
struct F16BatchUnbiasedSmall {   // 8 waves of 64 x 128 on a 256 x 256 tile, ping-pong loop, 32 x 32 x 16 MFMA, workgroup-level epilogue
  static constexpr int BM = 256, BN = 256, WM = 4, WN = 2;
  static constexpr bool PERSIST = false;
  static constexpr int POL = 0, PP = 2, KBT = 0;
  static constexpr bool BIAS = false;
  static constexpr int EPI = 0, MF = 0;
  static constexpr bool BUF = false;
  static constexpr int SKIP = 0, KFL = 0;
  static constexpr int PROBE = 0;   // development build: 1 = phase timing, 2 = no epilogue, 3 = no epilogue and no DMA in the k-loop
};
struct F16BatchUnbiased : F16BatchUnbiasedSmall { static constexpr bool PERSIST = true; };   // launches of >= 1024 tiles
struct F16BatchSmall : F16BatchUnbiasedSmall { static constexpr bool BIAS = true; };          // the small levels of a batch search
struct F16BatchDefault : F16BatchSmall {   // the batch kernel: persistent, 16 x 16 x 32 MFMA, wave-private epilogue
  static constexpr bool PERSIST = true;
  static constexpr int EPI = 1, MF = 1;
};
struct F16BatchComplement : F16BatchDefault { static constexpr int SKIP = 16; };   // the last level over the rows the stride-16 level has not seen
struct F16DeepFlush : F16BatchDefault { static constexpr int KFL = SV_F16_KFLUSH; };   // deep rows: the batch kernel, blocks flushed to a scratch
struct F16DeepFlushComplement : F16DeepFlush { static constexpr int SKIP = 16; };
struct F16DeepBlocked : F16BatchSmall {    // deep rows, launches that do not fill the batch kernel: 8 waves of 64 x 64 on 256 x 128 tiles,
  static constexpr int BN = 128;           // plain loop, a second accumulator set for the block sums
  static constexpr int PP = 0, KBT = SV_F16_KBLOCK / SV_F16_HBK;
  static constexpr int EPI = 1, MF = 1;
};
struct F16DeepBlockedBuf : F16DeepBlocked { static constexpr bool BUF = true; };   // its default form: operand DMA through buffer resources
struct F16DeepBlockedComplement : F16DeepBlocked { static constexpr int SKIP = 16; };
struct F16DeepBlockedBufComplement : F16DeepBlockedBuf { static constexpr int SKIP = 16; };
struct F16DeepUnbiased : F16BatchUnbiasedSmall {   // deep rows, norms too unbalanced for the bias: 4 waves of 64 x 64 on 128 x 128 tiles
  static constexpr int BM = 128, BN = 128, WM = 2, WN = 2;
  static constexpr int PP = 0, KBT = SV_F16_KBLOCK / SV_F16_HBK;
};
struct F16OneImage128 : F16BatchUnbiasedSmall {    // one query image per pass, <= 128 rows (f16_cfg 63): streams the database once,
  static constexpr int BM = 128, BN = 128, WM = 2, WN = 2;   // its rows non-temporal
  static constexpr int POL = 1, PP = 0;
};
struct F16OneImage64 : F16OneImage128 { static constexpr int BM = 64, WM = 1; };   // <= 64 rows (f16_cfg 62)
#ifdef SEGVLAD_ABLATIONS   // development build: three probes of the batch kernel (tools/probe_phases.py, tools/probe_ablate.py)
struct F16ProbePhases : F16BatchDefault { static constexpr int PROBE = 1; };          // f16_cfg 93: right results, prints the phase shares
struct F16ProbeNoEpilogue : F16BatchDefault { static constexpr int PROBE = 2; };      // f16_cfg 94: WRONG results
struct F16ProbeNoEpilogueNoDma : F16BatchDefault { static constexpr int PROBE = 3; }; // f16_cfg 95: WRONG results
#endif
// accumulation-block length of a kernel in elements (0 = one running accumulator): what sv_f16_c_eps has to cover
template <class C>
constexpr int f16_kblock_of() { return (C::KBT > C::KFL ? C::KBT : C::KFL) * SV_F16_HBK; }


// The launch contract of knn_f16_filter_kernel<C>: the LDS bytes of a workgroup, for the kernel's layout, its static_asserts and
// launch_f16_filter.  Stages: two A stages (PA bytes each) + SV_F16_NB B stages (PB each); PERSIST: five equal slots (see a_off / b_off).
// Epilogue scratch, over the stages of the finished tile (PERSIST: over slots 0 and 1 only, the next tile's head lands in the others):
//   EPI = 0   [BM] row records (16 B) + [BM] counters + [BN] column norms + [BM] screening bounds + per wave a hit list of LCAP + 1
//             records of 8 B (a quarter of the wave's elements at most)
//   EPI = 1   per wave WSZ bytes: 1024 of row records, bounds and counters + a hit list of LCAPE + 1 records (see the epilogue)
template <class C>
struct F16Lds {
  static constexpr int NW = C::WM * C::WN, TM = C::BM / (32 * C::WM), TN = C::BN / (32 * C::WN);
  static constexpr int PA = C::BM * SV_F16_HBK * 2, PB = C::BN * SV_F16_HBK * 2;
  static constexpr size_t STAGES = C::PERSIST ? 5 * (size_t)PA : 2 * (size_t)PA + (size_t)SV_F16_NB * PB;
  static constexpr int LCAP = C::PERSIST ? 896 : ((TM * TN * 256 < 2048) ? TM * TN * 256 : 2048);
  static constexpr int LCAPE = 864;
  static constexpr int WSZ = (1024 + (LCAPE + 1) * 8 + 15) & ~15;
  static constexpr size_t EPILOGUE = C::EPI == 1 ? (size_t)NW * WSZ : (size_t)C::BM * 24 + (size_t)C::BN * 4 + (size_t)NW * (LCAP + 1) * 8;
  static constexpr size_t BYTES = STAGES > EPILOGUE ? STAGES : EPILOGUE;   // the launch's dynamic LDS
  static_assert(!C::PERSIST || (PA == PB && STAGES <= 160 * 1024), "persistent layout: five equal slots");
  static_assert(!C::PERSIST || EPILOGUE <= 2 * (size_t)PA, "epilogue scratch");   // (not PERSIST: the scratch overlays the stages; BYTES covers both)
};
// KFL: fp32 words of a wave's slice of the flush scratch (kscr: [workgroup][wave][128][64 lanes], one word per accumulator and lane)
constexpr int SV_F16_KSCR_FLOATS = 128 * 64;

template <class C>
__global__ __launch_bounds__(64 * C::WM * C::WN) void knn_f16_filter_kernel(
    const uint16_t* __restrict__ Qh, const uint16_t* __restrict__ Rh, int M, int N, int d, int b_stride, int tiles_m, int gm,
    int seq_total, int walk,
    float inv_scale, const float* __restrict__ qn, const float* __restrict__ rn, const float* __restrict__ thr,
    int64_t thr_ld, float eps_mult, float c_eps, float rn_max, uint32_t* __restrict__ cand_cnt,
    float* __restrict__ cand_d2, uint32_t* __restrict__ cand_id, int cap, const float* __restrict__ inv_scale_dev,
    float* __restrict__ kscr) {
  // single-image searches leave the query scale on the device (no host round trip in front of the pass): [0] = scale,
  // [1] = 1 / (query scale x database scale)
  if (inv_scale_dev) inv_scale = inv_scale_dev[1];
  constexpr int BM = C::BM, BN = C::BN, WM = C::WM, WN = C::WN, PP = C::PP, KBT = C::KBT, EPI = C::EPI, MF = C::MF, SKIP = C::SKIP, KFL = C::KFL,
                PROBE = C::PROBE;
  constexpr bool PERSIST = C::PERSIST, BIAS = C::BIAS, BUF = C::BUF;
  constexpr int HBK = SV_F16_HBK, NB = SV_F16_NB;
  constexpr int NW = WM * WN;
  constexpr int AUXB = C::POL ? 2 : 0;   // aux = 2: "nt" (streaming) hint
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  static_assert(PP == 0 || PP == 2, "the plain loop or two ping-pong phases");
  static_assert(TM == 2 && (TN == 4 || TN == 2), "wave tiles of 64 rows x 128 or 64 columns: 128 or 64 accumulators per lane, in VGPRs");
  static_assert(KBT == 0 || PP == 0, "blocked accumulation (two accumulator sets): the plain loop");
  constexpr int RB = HBK * 2;            // row bytes per k-tile (128)
  constexpr int CH = RB / 16;            // 16-B chunks per row (8)
  constexpr int RP = 1024 / RB;          // rows per 1-KiB DMA piece
  constexpr int KS = HBK / 16;           // MFMA k-steps per tile
  using L = F16Lds<C>;                   // the LDS bytes of the launch
  constexpr int PA = L::PA, PB = L::PB;  // stage bytes
  constexpr int JA = BM / RP / NW, JB = BN / RP / NW;  // DMA pieces per wave and operand
  static_assert(JA * RP * NW == BM && JB * RP * NW == BN && (PP > 0 || (JA + JB) % (MF ? 2 : KS) == 0), "tile/wave geometry");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned long long phase_t0 = PROBE == 1 ? __builtin_amdgcn_s_memtime() : 0ull;
  // XCD-aware tile order: f16_walk.h.
  // PERSIST: 8 x 32 workgroups stay resident and walk their XCD's sequence 32 positions at a time; the head of the next
  // tile (A(0), B(0), B(1)) is requested before the epilogue of the current one, which hides the ~2 us a fresh
  // workgroup spends waiting for its first operands (6 % of the kernel: one workgroup per CU, nothing else covers it).
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: LDS DMA bases live in M0
  const int wm = w / WN, wn = w % WN;
  // KFL: this wave's slice of the flush scratch, as a scalar (wave-uniform) base address -- formed where it is used (a few SALU
  // instructions every 64 k-tiles) rather than kept live through the main loop
  auto kscr_base = [&]() -> float* {
    const unsigned long long ka = (unsigned long long)(size_t)(kscr + ((size_t)blockIdx.x * NW + (size_t)w) * SV_F16_KSCR_FLOATS);
    return reinterpret_cast<float*>((size_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ka >> 32)) << 32) |
                                             (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ka)));
  };
  const int64_t ldb = (int64_t)d * b_stride;
  // SKIP > 0 ("the complement of a sample"): operand row j is database row j + j / (SKIP - 1) + 1 -- the rows that are NOT multiples
  // of SKIP, in order.  The level before the last one has already filtered the multiples of SKIP (its stride-SKIP sample) with the same
  // arithmetic; its survivors stay in the candidate lists (SvSelect::Carry) and the last level does not compute them again.
  auto grow = [&](int64_t j) -> int64_t {
    if constexpr (SKIP > 0) return j + (int64_t)((uint32_t)j / (uint32_t)(SKIP - 1)) + 1;
    else return j * b_stride;
  };
  const int64_t ldr = (int64_t)d;   // fp16 elements per database row: operand row j starts at Rh + grow(j) * ldr
  const int ntiles = d / HBK;
  const int tiles_n = (N + BN - 1) / BN;
  auto swz = [](int r, int c) { return c ^ ((r >> 1) & 7); };
  // the walk (f16_walk.h) bound to this launch: the tile of position sq in this XCD's sequence, and the k-order of its step
  auto tile_of = [&](int sq, int& tm_, int& tn_) -> bool { SV_F16_WALK_TILE_OF(sq, blockIdx.x & 7, tiles_m, tiles_n, gm, walk, tm_, tn_) };
  auto rev_of = [&](int sq) -> int { return f16_walk_rev_of(sq, gm, ntiles, walk); };
  auto kofs = [&](int rev_, int x) -> int { return f16_walk_kofs(rev_, x, ntiles); };
  int tm, tn;
  int seq = (int)(blockIdx.x >> 3);
  // PERSIST: resident workgroups per XCD = the stride of a workgroup through its XCD's sequence (bits 8.. of `walk`; 32 = one per
  // CU.  Fewer leave CUs to kernels of other streams -- the describe stage of the next batch -- for the whole launch: option f16_persist_wgs)
  const int pstep = (walk >> 8) > 0 ? (walk >> 8) : 32;
  if (PERSIST) {
    while (seq < seq_total && !tile_of(seq, tm, tn)) seq += pstep;
    if (seq >= seq_total) return;
  } else if (gm > 0) {
    if (!tile_of(seq, tm, tn)) return;
  } else {
    tm = blockIdx.x % tiles_m;
    tn = blockIdx.x / tiles_m;
  }
  // LDS stages.  Plain: A stages at 0, PA; B stages behind them.  PERSIST (five 32-KiB slots): the first stages of both
  // operands and B's second sit in slots 3, 4, 2 -- outside the epilogue's scratch (slots 0, 1) -- so that the next
  // tile's head can land while the epilogue runs.
  auto a_off = [](int st_) { return PERSIST ? (st_ == 0 ? 3 * PA : 0) : st_ * PA; };
  auto b_off = [](int st_) { return PERSIST ? (st_ == 0 ? 4 * PA : (st_ == 1 ? 2 * PA : PA)) : 2 * PA + st_ * PB; };
  const int lrow_p = l / CH, lch = l % CH;
  // Source of this lane's 16 bytes of DMA piece j of the tile at m0_ / n0_ (k-tile 0; rows beyond the operand clamp to its last row:
  // they are never emitted; the chunk is the swizzled one, see above): as a pointer, and -- BUF -- as a byte offset inside the tile
  auto src_a = [&](int64_t m0_, int j) -> const uint16_t* {
    const int row = (w * JA + j) * RP + lrow_p;
    const int64_t qa = (m0_ + row < M) ? (m0_ + row) : (int64_t)(M - 1);
    return Qh + qa * d + 8 * swz(row, lch);
  };
  auto src_b = [&](int64_t n0_, int j) -> const uint16_t* {
    const int row = (w * JB + j) * RP + lrow_p;
    const int64_t rb = (n0_ + row < N) ? (n0_ + row) : (int64_t)(N - 1);
    return Rh + grow(rb) * ldr + 8 * swz(row, lch);
  };
  auto voff_a = [&](int64_t m0_, int j) -> unsigned {
    const int row = (w * JA + j) * RP + lrow_p;
    const int rr = (m0_ + row < M) ? row : (int)((int64_t)M - 1 - m0_);
    return (unsigned)rr * (unsigned)(d * 2) + 16u * (unsigned)swz(row, lch);
  };
  auto voff_b = [&](int64_t n0_, int j) -> unsigned {
    const int row = (w * JB + j) * RP + lrow_p;
    const int rr = (n0_ + row < N) ? row : (int)((int64_t)N - 1 - n0_);
    if constexpr (SKIP > 0) return (unsigned)(grow(n0_ + rr) - grow(n0_)) * (unsigned)(d * 2) + 16u * (unsigned)swz(row, lch);
    return (unsigned)rr * (unsigned)(ldb * 2) + 16u * (unsigned)swz(row, lch);
  };
  auto rsrc_of = [](const uint16_t* base) -> sv_rsrc_t { return SV_BUF_RSRC(base); };   // BUF: the tile's buffer resource
  // head of a tile: A(0), B(0) and B(1), by global->LDS DMA.  (The three groups stay three loops per DMA form: issued through one inner
  // helper, the scalar head code of all 14 kernels moved and the deep-row record of the bench came out 0.6-1.0 % slower:
  // profiles/knn_filter_split_ab.txt.)
  auto issue_head = [&](int tm_, int tn_, int rev_) {
    const int64_t m0_ = (int64_t)tm_ * BM, n0_ = (int64_t)tn_ * BN;
    const int k0_ = kofs(rev_, 0), k1_ = kofs(rev_, 1);
    if constexpr (BUF) {
      const sv_rsrc_t ra = rsrc_of(Qh + m0_ * d), rb_ = rsrc_of(Rh + grow(n0_) * ldr);
#pragma unroll
      for (int j = 0; j < JA; ++j) SV_BUF_LOAD_LDS(ra, (sv_lptr_t)(lds + a_off(0) + (w * JA + j) * 1024), voff_a(m0_, j), 2 * k0_, 0);
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const unsigned vo = voff_b(n0_, j);
        SV_BUF_LOAD_LDS(rb_, (sv_lptr_t)(lds + b_off(0) + (w * JB + j) * 1024), vo, 2 * k0_, AUXB);
      }
      if (ntiles > 1) {
#pragma unroll
        for (int j = 0; j < JB; ++j) SV_BUF_LOAD_LDS(rb_, (sv_lptr_t)(lds + b_off(1) + (w * JB + j) * 1024), voff_b(n0_, j), 2 * k1_, AUXB);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < JA; ++j)
      __builtin_amdgcn_global_load_lds((sv_gptr_t)(src_a(m0_, j) + k0_), (sv_lptr_t)(lds + a_off(0) + (w * JA + j) * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < JB; ++j)
      __builtin_amdgcn_global_load_lds((sv_gptr_t)(src_b(n0_, j) + k0_), (sv_lptr_t)(lds + b_off(0) + (w * JB + j) * 1024), 16, 0, AUXB);
    if (ntiles > 1) {
#pragma unroll
      for (int j = 0; j < JB; ++j)
        __builtin_amdgcn_global_load_lds((sv_gptr_t)(src_b(n0_, j) + k1_), (sv_lptr_t)(lds + b_off(1) + (w * JB + j) * 1024), 16, 0, AUXB);
    }
  };
  // BIAS: this lane's column norms of the (next) tile, requested BEFORE the tile's head so that the head's wait covers them
  static_assert((MF == 1) == (EPI == 1) && (MF == 0 || BIAS), "16 x 16 x 32 MFMA <=> the wave-private epilogue, both on biased accumulators");
  constexpr int TN16 = (BN / WN) / 16;                // MF = 1: column tiles of 16 per wave (8, or 4 with blocked accumulation)
  constexpr int CW = MF ? 16 : 32;                    // columns (and rows) per MFMA tile
  constexpr int NCN = (BN / WN) / CW;                 // column tiles per wave = column norms per lane
  static_assert(KFL == 0 || 4 * TN16 * 4 * 64 == SV_F16_KSCR_FLOATS, "flush scratch: one word per accumulator and lane of a wave");
  float cnn[NCN];
  auto load_cn = [&](int tn_) {
#pragma unroll
    for (int nt = 0; nt < NCN; ++nt) {
      const int64_t colj = (int64_t)tn_ * BN + wn * (32 * TN) + nt * CW + (threadIdx.x & (CW - 1));
      cnn[nt] = (colj < N) ? rn[grow(colj)] : INFINITY;  // +inf: columns beyond N never pass
    }
  };
  // PERSIST: this workgroup's next tile behind the current one -- found (sq < seq_total), its column norms and its head requested.
  // A statement macro: as a lambda around issue_head the five persistent kernels gain 27 to 50 instructions (profiles/knn_filter_split_ab.txt).
#define SV_F16_NEXT_TILE(sq, tm_, tn_)                                 \
  sq = seq + pstep;                                                    \
  while (sq < seq_total && !tile_of(sq, tm_, tn_)) sq += pstep;        \
  if (sq < seq_total) {                                                \
    if (BIAS) load_cn(tn_);                                            \
    if (PROBE != 3) issue_head(tm_, tn_, rev_of(sq));                  \
  }
  if (BIAS) load_cn(tn);
  int rev = PERSIST ? rev_of(seq) : 0;   // (only the persistent walk has steps to alternate / rotate)
  issue_head(tm, tn, rev);
  if (ntiles > 1)
    sv_wait_vm_lgkm0<JB>();
  else
    sv_wait_vm_lgkm0<0>();
  // (the barrier that publishes the head to the other waves is the one at the top of the tile loop)

  for (;;) {   // PERSIST: one iteration per tile; otherwise a single pass
    __builtin_amdgcn_s_barrier();   // head of this tile landed for every wave; (PERSIST) every wave left the previous epilogue
    // the lane id is re-derived from an opaque copy in every iteration: otherwise the hundreds of constant addresses of
    // the unrolled epilogue are hoisted out of the tile loop and spill (713 VGPRs)
    int lane_opaque = (int)threadIdx.x;
    asm volatile("" : "+v"(lane_opaque));
    const int tid = lane_opaque, l = tid & 63, i = l & 31, kk = l >> 5;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    float cn[NCN];
    if (BIAS) {
#pragma unroll
      for (int nt = 0; nt < NCN; ++nt) cn[nt] = cnn[nt];
    }
    f32x16 acc[MF ? 1 : TM][MF ? 1 : TN];
    f32x4 acc16[MF ? 4 : 1][MF ? TN16 : 1];   // MF = 1: element j of tile (mt, nt) = row mt*16 + 4*(lane>>4) + j, column nt*16 + (lane&15)
    f32x4 accb16[(MF && KBT > 0) ? 4 : 1][(MF && KBT > 0) ? TN16 : 1];   // blocked accumulation: the sum of the finished k-blocks (+ the bias)
    if constexpr (MF == 0) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          const float a0_ = BIAS ? -(cn[b] * (0.5f / inv_scale)) : 0.f;   // (the same product the epilogue forms: cnh)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = a0_;
        }
    } else {
#pragma unroll
      for (int b = 0; b < TN16; ++b) {
        const float a0_ = -(cn[b] * (0.5f / inv_scale));
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (KBT > 0) {   // the bias lives in the sum of the blocks; every block starts at zero
              accb16[a][b][r] = a0_;
              acc16[a][b][r] = 0.f;
            } else {
              acc16[a][b][r] = a0_;
            }
          }
      }
    }
    f32x16 accb[KBT > 0 ? TM : 1][KBT > 0 ? TN : 1];   // blocked accumulation: the sum of the finished k-blocks
    if (KBT > 0) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) accb[KBT > 0 ? a : 0][KBT > 0 ? b : 0][r] = 0.f;
    }

    // epilogue inputs, requested now so that their latency hides under the main loop (one workgroup per CU: nothing
    // else would cover it): row tid's ||q||^2 and threshold, this lane's column norms
    static_assert(BM <= 64 * NW, "one thread per query row stages the epilogue's row record");
    float pre_q2 = 0.f, pre_thr = 0.f;
    if (EPI == 1) {   // wave-private epilogue: lane l stages row l of THIS wave's 64 query rows
      const int64_t qrow = m0 + wm * (32 * TM) + l;
      if (qrow < M) {
        pre_q2 = qn[qrow];
        pre_thr = thr[qrow * thr_ld];
      }
    } else if (tid < BM && m0 + tid < M) {
      pre_q2 = qn[m0 + tid];
      pre_thr = thr[(m0 + tid) * thr_ld];
    }
    if constexpr (!BIAS) {
#pragma unroll
      for (int nt = 0; nt < TN; ++nt) {
        const int64_t colj = n0 + wn * (32 * TN) + nt * 32 + i;
        cn[nt] = (colj < N) ? rn[grow(colj)] : INFINITY;  // +inf: columns beyond N never pass
      }
    }

    // per-lane source rows of this wave's DMA pieces (clamped: edge rows are never emitted)
    const uint16_t* srcA[BUF ? 1 : JA];
    const uint16_t* srcB[BUF ? 1 : JB];
    unsigned voA[BUF ? JA : 1], voB[BUF ? JB : 1];
    const sv_rsrc_t rsA = rsrc_of(Qh + m0 * d), rsB = rsrc_of(Rh + grow(n0) * ldr);
    if constexpr (BUF) {
#pragma unroll
      for (int j = 0; j < JA; ++j) voA[j] = voff_a(m0, j);
#pragma unroll
      for (int j = 0; j < JB; ++j) voB[j] = voff_b(n0, j);
    } else {
#pragma unroll
      for (int j = 0; j < JA; ++j) srcA[j] = src_a(m0, j);
#pragma unroll
      for (int j = 0; j < JB; ++j) srcB[j] = src_b(n0, j);
    }
    constexpr int BAHEAD = NB - 1;  // how many k-tiles ahead the B DMA runs (A always runs one ahead)
    // DMA piece p of iteration kt: pieces 0..JA-1 belong to A(kt+1), JA..JA+JB-1 to B(kt+BAHEAD)
    auto dma_piece = [&](int piece, int kt, int ia_next, int ib_next) {
      if (PROBE == 3) return;  // (development build) no DMA in the loop
      if constexpr (BUF) {
        if (piece < JA) {
          if (kt + 1 < ntiles)
            SV_BUF_LOAD_LDS(rsA, (sv_lptr_t)(lds + a_off(ia_next) + (w * JA + piece) * 1024), voA[piece], 2 * kofs(rev, kt + 1), 0);
        } else {
          const int j = piece - JA;
          if (kt + BAHEAD < ntiles)
            SV_BUF_LOAD_LDS(rsB, (sv_lptr_t)(lds + b_off(ib_next) + (w * JB + j) * 1024), voB[j], 2 * kofs(rev, kt + BAHEAD), AUXB);
        }
      } else if (piece < JA) {
        if (kt + 1 < ntiles)
          __builtin_amdgcn_global_load_lds((sv_gptr_t)(srcA[piece] + kofs(rev, kt + 1)),
                                           (sv_lptr_t)(lds + a_off(ia_next) + (w * JA + piece) * 1024), 16, 0, 0);
      } else {
        const int j = piece - JA;
        if (kt + BAHEAD < ntiles)
          __builtin_amdgcn_global_load_lds((sv_gptr_t)(srcB[j] + kofs(rev, kt + BAHEAD)),
                                           (sv_lptr_t)(lds + b_off(ib_next) + (w * JB + j) * 1024), 16, 0, AUXB);
      }
    };
    SV_PHASE(0)  // prologue: first tiles landed

    int ia = 0, ib = 0;
    const int fa0 = wm * (32 * TM) + i, fb0 = wn * (32 * TN) + i;
    if constexpr (PP > 0) {
      constexpr int PH = KS / 2;            // MFMA k-steps per phase
      constexpr int DPP = (JA + JB) / 2;    // DMA pieces per phase and wave
      static_assert(KS % 2 == 0 && (JA + JB) % 2 == 0, "phase geometry");
      const bool lag = w >= NW / 2;           // wave-uniform (w comes from readfirstlane)
      if (lag) __builtin_amdgcn_s_barrier(); // the second half of the waves runs one barrier (= one segment) behind
      // (KFL: the k-tiles run in blocks of KFL; the flush sits BETWEEN two runs of the inner loop, not behind a branch inside it -- with
      //  the branch inside, the 128 accumulators met a zeroed copy of themselves at the loop's back edge and 40 registers spilled)
      int kt = 0;
      for (int kstop = (KFL > 0 && KFL < ntiles) ? KFL : ntiles;;) {
        for (; kt < kstop; ++kt) {
          const int ibn = (ib + BAHEAD >= NB) ? ib + BAHEAD - NB : ib + BAHEAD;
          const unsigned char* SA = lds + a_off(ia);
          const unsigned char* SB = lds + b_off(ib);
#pragma unroll
          for (int ph = 0; ph < 2; ++ph) {
            // ---- load segment: fragments of this phase's k-steps, this phase's share of the DMA pieces ----
            f16x8 a[MF ? 1 : PH][MF ? 4 : TM], b[MF ? 1 : PH][MF ? TN16 : TN];
            if constexpr (MF == 0) {
#pragma unroll
              for (int k2 = 0; k2 < PH; ++k2) {
                const int cl = 2 * (ph * PH + k2) + kk;
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                  const int ra = fa0 + 32 * t;
                  a[k2][t] = *reinterpret_cast<const f16x8*>(SA + ra * RB + swz(ra, cl) * 16);
                }
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                  const int rb = fb0 + 32 * t;
                  b[k2][t] = *reinterpret_cast<const f16x8*>(SB + rb * RB + swz(rb, cl) * 16);
                }
              }
            } else {
              // one k-step of 32 per phase: lane l holds row / column (l & 15) of a 16-wide tile, k-chunk (l >> 4) of the step's four
              // (the source-side swizzle of the 128-byte rows is conflict-free for this pattern too: a 16-lane ds_read_b128 group
              //  covers rows {0-3, 12-15} of one chunk and rows {4-11} of the next, 16 distinct bank groups)
              static_assert(PH == 2 && CH == 8, "a phase = 32 k of 128-byte rows");
              const int cl = 4 * ph + (l >> 4);
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const int ra = wm * 64 + 16 * t + (l & 15);
                a[0][t] = *reinterpret_cast<const f16x8*>(SA + ra * RB + swz(ra, cl) * 16);
              }
#pragma unroll
              for (int t = 0; t < TN16; ++t) {
                const int rb = wn * (16 * TN16) + 16 * t + (l & 15);
                b[0][t] = *reinterpret_cast<const f16x8*>(SB + rb * RB + swz(rb, cl) * 16);
              }
            }
#pragma unroll
            for (int pz = 0; pz < DPP; ++pz) dma_piece(ph * DPP + pz, kt, ia ^ 1, ibn);
            if (ph == 1) {
              // last load segment of the k-tile: this wave's pieces of A(kt+1) and B(kt+1) have landed (B(kt+2), the
              // youngest JB DMA instructions, may still fly).  The barriers between here and the first read of tile kt+1
              // (one for the leading half, two for the lagging half) make that true for every wave's pieces.
              if (kt + 2 < ntiles)
                sv_wait_vm_lgkm0<JB>();
              else
                sv_wait_vm_lgkm0<0>();
            } else {
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            // ---- MFMA segment ----
            __builtin_amdgcn_s_setprio(1);
            if constexpr (MF == 0) {
#pragma unroll
              for (int k2 = 0; k2 < PH; ++k2)
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                  for (int nt = 0; nt < TN; ++nt) acc[mt][nt] = MFMA_F16(a[k2][mt], b[k2][nt], acc[mt][nt]);
            } else {
#pragma unroll
              for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < TN16; ++nt)
                  acc16[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][mt], b[0][nt], acc16[mt][nt], 0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
          }
          ia ^= 1;
          ib = (ib + 1 >= NB) ? 0 : ib + 1;
        }
        if (KFL == 0 || kt >= ntiles) break;
        if constexpr (KFL > 0) {   // close a k-block into the wave's global scratch slice (see KFL)
          static_assert(MF == 1 && KBT == 0 && PERSIST && TN16 == 8, "flushed blocks: the persistent 16 x 16 x 32 ping-pong kernel");
          float* const kscr_w = kscr_base() + l;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN16; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                sv_atomic_add_noret(kscr_w + 64 * ((mt * TN16 + nt) * 4 + r), acc16[mt][nt][r]);
                acc16[mt][nt][r] = 0.f;
              }
        }
        kstop = (kt + (KFL > 0 ? KFL : 1) < ntiles) ? kt + (KFL > 0 ? KFL : 1) : ntiles;
      }
      if (!lag) __builtin_amdgcn_s_barrier();  // the leading half waits for the lagging half's last MFMA segment
      if constexpr (KFL > 0) {
        if (ntiles > KFL) {   // the last block joins the flushed ones; totals back into the accumulators; the slice is left zero
          float* const kscr_w = kscr_base() + l;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN16; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r) sv_atomic_add_noret(kscr_w + 64 * ((mt * TN16 + nt) * 4 + r), acc16[mt][nt][r]);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN16; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r)   // (agent-scope load: from L2, not from a line the previous tile left in this CU's vector cache)
                acc16[mt][nt][r] = __hip_atomic_load(kscr_w + 64 * ((mt * TN16 + nt) * 4 + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (int j = 0; j < 16 * TN16; ++j) __hip_atomic_store(kscr_w + 64 * j, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    } else if constexpr (MF == 1) {
      // the plain loop (one barrier per k-tile) on the 16 x 16 x 32 shape: two k-steps of 32 per k-tile
      static_assert(KS == 4 && (JA + JB) % 2 == 0, "two k-steps of 32 per 64-deep k-tile");
      for (int kt = 0; kt < ntiles; ++kt) {
        const int ibn = (ib + BAHEAD >= NB) ? ib + BAHEAD - NB : ib + BAHEAD;
        const unsigned char* SA = lds + a_off(ia);
        const unsigned char* SB = lds + b_off(ib);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int cl = 4 * k2 + (l >> 4);
          f16x8 a[4], b[TN16];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int ra = wm * 64 + 16 * t + (l & 15);
            a[t] = *reinterpret_cast<const f16x8*>(SA + ra * RB + swz(ra, cl) * 16);
          }
#pragma unroll
          for (int t = 0; t < TN16; ++t) {
            const int rb = wn * (16 * TN16) + 16 * t + (l & 15);
            b[t] = *reinterpret_cast<const f16x8*>(SB + rb * RB + swz(rb, cl) * 16);
          }
#pragma unroll
          for (int pz = 0; pz < (JA + JB) / 2; ++pz) dma_piece(k2 * ((JA + JB) / 2) + pz, kt, ia ^ 1, ibn);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN16; ++nt) acc16[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[mt], b[nt], acc16[mt][nt], 0, 0, 0);
        }
        if (kt + 2 < ntiles)
          sv_wait_vm_lgkm0<JB>();
        else
          sv_wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        ia ^= 1;
        ib = (ib + 1 >= NB) ? 0 : ib + 1;
        if constexpr (KBT > 0) {
          if ((kt + 1) % (KBT > 0 ? KBT : 1) == 0 || kt + 1 == ntiles) {   // close a k-block (wave-uniform)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
              for (int nt = 0; nt < TN16; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  accb16[mt][nt][r] += acc16[mt][nt][r];
                  acc16[mt][nt][r] = (kt + 1 == ntiles) ? accb16[mt][nt][r] : 0.f;   // last block: acc = the total
                }
          }
        }
      }
    } else {
      for (int kt = 0; kt < ntiles; ++kt) {
        const int ibn = (ib + BAHEAD >= NB) ? ib + BAHEAD - NB : ib + BAHEAD;
        const unsigned char* SA = lds + a_off(ia);
        const unsigned char* SB = lds + b_off(ib);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int cl = 2 * ks + kk;  // logical 16-B chunk (8 consecutive k) of this lane
          f16x8 a[TM], b[TN];
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const int ra = fa0 + 32 * t;
            a[t] = *reinterpret_cast<const f16x8*>(SA + ra * RB + swz(ra, cl) * 16);
          }
#pragma unroll
          for (int t = 0; t < TN; ++t) {
            const int rb = fb0 + 32 * t;
            b[t] = *reinterpret_cast<const f16x8*>(SB + rb * RB + swz(rb, cl) * 16);
          }
#pragma unroll
          for (int pz = 0; pz < (JA + JB) / KS; ++pz) dma_piece(ks * ((JA + JB) / KS) + pz, kt, ia ^ 1, ibn);
#pragma unroll
          for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) acc[mt][nt] = MFMA_F16(a[mt], b[nt], acc[mt][nt]);
        }
        // this wave's pieces of A(kt+1) and B(kt+1) have landed (B(kt+2) -- the youngest JB DMA
        // instructions -- may still fly: vmcnt retires in order) and its LDS reads are done; after the barrier that
        // holds for every wave, so the stages of tile kt may be overwritten
        if (kt + 2 < ntiles)
          sv_wait_vm_lgkm0<JB>();
        else
          sv_wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        ia ^= 1;
        ib = (ib + 1 >= NB) ? 0 : ib + 1;
        if (KBT > 0 && ((kt + 1) % (KBT > 0 ? KBT : 1) == 0 || kt + 1 == ntiles)) {   // close a k-block (wave-uniform)
#pragma unroll
          for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN; ++nt)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                accb[KBT > 0 ? mt : 0][KBT > 0 ? nt : 0][r] += acc[mt][nt][r];
                acc[mt][nt][r] = (kt + 1 == ntiles) ? accb[KBT > 0 ? mt : 0][KBT > 0 ? nt : 0][r] : 0.f;   // last block: acc = the total
              }
        }
      }
    }

    SV_PHASE(1)  // main loop
    if constexpr (PROBE >= 2) {  // (development build) no epilogue: WRONG results (the accumulators stay live)
      static_assert(PROBE < 2 || (MF == 1 && PERSIST), "the probes are forms of the default batch kernel");
      float t = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN16; ++nt) t += acc16[mt][nt][0] + acc16[mt][nt][3];
      if (t == 12345.678f) cand_cnt[0] = 1;
      // on to the workgroup's next tile (its head requested here, waited for at once)
      int tm_n = 0, tn_n = 0, sq_n;
      SV_F16_NEXT_TILE(sq_n, tm_n, tn_n)
      if (sq_n >= seq_total) return;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      seq = sq_n;
      tm = tm_n;
      tn = tn_n;
      rev = rev_of(seq);
      continue;
    }
    // The epilogue's row record {||q||^2, exact limit, screening bound} of this thread's row, in registers and BEFORE the next
    // tile's head is requested: the compiler waits for the two global loads behind it (issued before the main loop, long
    // since landed) with s_waitcnt vmcnt(0) at their first use -- placed behind the head's DMA instructions that wait sat out
    // the head's whole flight (~2 us per tile, with nothing else to do: the very latency the early request is meant to hide).
    //   v <= lim  <=>  acc - cn * half_scale >= (q2 - lim) * half_scale; the slack (relative 2^-17 of the largest possible
    //   magnitude) makes rounding of this shortcut only ever ADD candidates
    const float half_scale = 0.5f / inv_scale;
    const float rmax_hs = rn_max * half_scale;
    float st_q2 = 0.f, st_lim = -INFINITY, st_tau = INFINITY;
    if (EPI == 1 ? (m0 + wm * (32 * TM) + l < M) : (tid < BM && m0 + tid < M)) {
      st_q2 = pre_q2;
      st_lim = pre_thr + eps_mult * c_eps * sqrtf(st_q2 * rn_max);
      const float base = (st_q2 - st_lim) * half_scale;
      st_tau = base - 7.7e-6f * (fabsf(base) + rmax_hs);
    }
    asm volatile("" : "+v"(st_q2), "+v"(st_lim), "+v"(st_tau));   // (keeps the computation -- and its wait -- on this side of the DMA issue)
    // PERSIST: the next tile of this workgroup; its head is requested now and lands under the epilogue
    int tm_next = 0, tn_next = 0, seq_next = seq_total;
    if (PERSIST) {
      SV_F16_NEXT_TILE(seq_next, tm_next, tn_next)
    }
    // ---- epilogue: keep d2~ <= thr + eps_mult * eps(q) -----------------------------------------------------------
    // The epilogue is VALU-issue bound (s_memtime phase timing, see PROBE: every instruction of the sparse
    // per-survivor paths is paid by the whole wave), so it is organised around instruction count and everything
    // per-survivor happens on DENSE lanes:
    //  * per-row quantities {||q||^2, exact limit, screening bound} and the tile's column norms are staged once per
    //    workgroup in LDS (their global loads were issued before the main loop);
    //  * pass 1 screens every accumulator element with one fma + compare against the row's bound; the (rare) waves
    //    that see a hit compact the raw {accumulator, row | column} pairs by ballot/mbcnt into a wave-private LDS
    //    list -- three instructions per element on the common path, no atomics, no exact arithmetic;
    //  * pass 2a walks that list 64 records at a time (all lanes busy): exact d2~, exact limit test, LDS count per row;
    //  * ONE global atomic per row and workgroup reserves a slot range in that query's candidate list;
    //  * pass 2b walks the list again and stores the survivors at range + LDS ticket.
    // (History: one returning global atomic per survivor parked the wave ~1.5 us each; re-walking the 128 accumulator
    // elements under a per-lane bitmap cost 20 % of the kernel; ~100-instruction exact-test bodies per hit row 25 %.)
    // A wave whose 64 x 128 block holds more than LCAP hits (databases are spatially coherent: the 50 segments of a
    // query image against the rows of the same place) abandons its list and walks its accumulators directly
    // (per-hit LDS atomics: slow, but only for the handful of dense blocks).  The list order is arbitrary: every
    // consumer ranks or sorts it.
    // records per wave: a quarter of its elements at most; PERSIST keeps the whole scratch inside LDS slots 0 and 1 (F16Lds)
    constexpr int LCAP = L::LCAP, LCAPE = L::LCAPE, WSZ = L::WSZ;   // EPI = 0: records per wave list | EPI = 1: the same, bytes per wave
    if constexpr (EPI == 1) {
      // ---- wave-private epilogue (EPI = 1; persistent + biased kernels) ------------------------------------------------
      // Nothing in it is shared between waves, so nothing in it waits for another wave: every wave stages the records of ITS
      // 64 query rows, screens its 64 x 128 block into its own LDS list, tests the list densely and takes ONE returning global
      // atomic per ROW WITH SURVIVORS (ranks inside a row from a wave-private LDS counter): the reservation's round trip
      // overlaps the wait for the next tile's head, which the wave has to sit out anyway, and the stores are left in flight.
      // A block that fills its list (spatially coherent databases: the 50 segments of a query image against the 200 rows of the
      // same place are thousands of hits in ONE 64 x 128 block) flushes it in place and goes on screening -- still one round
      // trip per flush.  (First version: one returning global atomic per survivor, 64 at a time -- fine at ~6 survivors per
      // block, 150 round trips for such a block.  A re-entrant screening pass -- flush, then jump back in -- turns the pass
      // into a loop whose invariants the compiler hoists and spills: 80 dwords.)
      static_assert(BIAS && MF == 1, "wave-private epilogue: the biased kernels on the 16 x 16 x 32 shape");
      // Every LDS access between the head's DMA instructions and the wait inside the first flush is RAW (inline asm): the
      // compiler cannot tell DMA'd LDS bytes from any other LDS address and puts s_waitcnt vmcnt(0) in front of every LDS
      // instruction it can see while a DMA is pending -- the wave would sit out the head's flight before its first epilogue
      // instruction (which is what EPI = 0 does).  One wave's LDS instructions execute in order, so a write followed by a read
      // of the same bytes needs no wait in between; reads are waited for with explicit lgkmcnt.
      // per wave: [64] {||q||^2, exact limit} | +512: [64] screening bounds | +768: [64] survivors per row, then the row's first
      // global slot | +1024: [LCAPE + 1] hits {accumulator bits -> d2~, row << 16 | rank in the row << 8 | column}
      const unsigned wb_a = (unsigned)(size_t)(sv_lptr_t)(lds + (size_t)w * WSZ);
      {
        const float2 qr = make_float2(st_q2, st_lim);
        asm volatile("ds_write_b64 %0, %1\n\tds_write_b32 %2, %3 offset:512\n\tds_write_b32 %2, %4 offset:768" ::"v"(wb_a + 8u * (unsigned)l), "v"(qr),
                     "v"(wb_a + 4u * (unsigned)l), "v"(st_tau), "v"(0u)
                     : "memory");
      }
      SV_PHASE(2)
      // this lane's screening bounds: element j of tile mt is row mt*16 + 4*(lane>>4) + j -- 4 groups of 4 consecutive rows
      float4 tqw[4];
      {
        const unsigned ta = wb_a + 512u + 16u * (unsigned)(l >> 4);
        asm volatile(
            "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\tds_read_b128 %3, %4 offset:192\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(tqw[0]), "=&v"(tqw[1]), "=&v"(tqw[2]), "=&v"(tqw[3])
            : "v"(ta)
            : "memory");
      }
      uint32_t wave_cnt = 0;   // wave-uniform
      const uint32_t colbase = (uint32_t)(wn * (32 * TN) + (l & 15)), rowsel = (uint32_t)(4 * (l >> 4));
      const int64_t rowbase = m0 + wm * 64;
      // dense exact test of the list, one returning global atomic per row with survivors, the stores left in flight
      auto flush = [&]() {
        const uint32_t n_w = wave_cnt;
        for (uint32_t tb = 0; tb < n_w; tb += 64u) {   // exact test; a survivor draws its rank inside its row
          const uint32_t t = tb + (uint32_t)l;
          if (t < n_w) {
            uint2 rec;
            float2 rr;
            asm volatile("ds_read_b64 %0, %1 offset:1024\n\ts_waitcnt lgkmcnt(0)" : "=v"(rec) : "v"(wb_a + 8u * t) : "memory");
            const unsigned lrow = rec.y >> 16;
            asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(rr) : "v"(wb_a + 8u * lrow) : "memory");
            const float v = __fmaf_rn(-2.f, __uint_as_float(rec.x) * inv_scale, rr.x);
            if (v <= rr.y && v < INFINITY) {   // +inf: padding columns beyond N (admitted by the screen when thr = +inf)
              uint32_t rank;
              asm volatile("ds_add_rtn_u32 %0, %1, %2 offset:768\n\ts_waitcnt lgkmcnt(0)" : "=v"(rank) : "v"(wb_a + 4u * lrow), "v"(1u) : "memory");
              rec.x = __float_as_uint(v);
              rec.y |= rank << 8;              // (< 128 survivors per row and block; the column keeps bits 0-7)
            } else {
              rec.y = 0xffffffffu;             // screened in by the slack only
            }
            asm volatile("ds_write_b64 %0, %1 offset:1024" ::"v"(wb_a + 8u * t), "v"(rec) : "memory");
          }
        }
        uint32_t c;
        asm volatile("ds_read_b32 %0, %1 offset:768\n\ts_waitcnt lgkmcnt(0)" : "=v"(c) : "v"(wb_a + 4u * (unsigned)l) : "memory");
        uint32_t base = 0u;
        if (c) base = atomicAdd(&cand_cnt[rowbase + l], c);   // (rows >= M screen with +inf: no survivors)
        // the reservations -- and, the first time round, this wave's DMA pieces of the next tile's head (requested before the
        // screening pass; loads retire in order): the barrier at the top of the tile loop makes that true for every wave
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("ds_write_b32 %0, %1 offset:768" ::"v"(wb_a + 4u * (unsigned)l), "v"(base) : "memory");
        for (uint32_t tb = 0; tb < n_w; tb += 64u) {
          const uint32_t t = tb + (uint32_t)l;
          if (t < n_w) {
            uint2 rec;
            asm volatile("ds_read_b64 %0, %1 offset:1024\n\ts_waitcnt lgkmcnt(0)" : "=v"(rec) : "v"(wb_a + 8u * t) : "memory");
            if (rec.y != 0xffffffffu) {
              const unsigned lrow = rec.y >> 16;
              uint32_t b0;
              asm volatile("ds_read_b32 %0, %1 offset:768\n\ts_waitcnt lgkmcnt(0)" : "=v"(b0) : "v"(wb_a + 4u * lrow) : "memory");
              const uint32_t slot = b0 + ((rec.y >> 8) & 0xffu);
              if (slot < (uint32_t)cap) {
                const int64_t row = rowbase + (int64_t)lrow;
                cand_d2[row * cap + slot] = __uint_as_float(rec.x);
                cand_id[row * cap + slot] = (uint32_t)grow(n0 + (int64_t)(rec.y & 0xffu));
              }
            }
          }
        }
        asm volatile("ds_write_b32 %0, %1 offset:768" ::"v"(wb_a + 4u * (unsigned)l), "v"(0u) : "memory");
        wave_cnt = 0u;
      };
      {
        // 16 screening steps of 8 elements (one row of the wave tile across its 8 column tiles)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 tq4 = tqw[mt];
            const float tau = j == 0 ? tq4.x : j == 1 ? tq4.y : j == 2 ? tq4.z : tq4.w;
            float best;
            asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(best) : "v"(acc16[mt][0][j]), "v"(acc16[mt][1][j]), "v"(acc16[mt][2][j]));
            if constexpr (TN16 == 8) {
              asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(best) : "v"(best), "v"(acc16[mt][3][j]), "v"(acc16[mt][TN16 == 8 ? 4 : 0][j]));
              asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(best) : "v"(best), "v"(acc16[mt][TN16 == 8 ? 5 : 0][j]), "v"(acc16[mt][TN16 == 8 ? 6 : 0][j]));
              asm volatile("v_max_f32 %0, %1, %2" : "=v"(best) : "v"(best), "v"(acc16[mt][TN16 == 8 ? 7 : 0][j]));
            } else {
              asm volatile("v_max_f32 %0, %1, %2" : "=v"(best) : "v"(best), "v"(acc16[mt][3][j]));
            }
            if (__builtin_amdgcn_ballot_w64(best >= tau) != 0ull) {
              const uint32_t rc = (((uint32_t)(mt * 16 + j) + rowsel) << 16) | colbase;
#pragma unroll
              for (int nt = 0; nt < TN16; ++nt) {
                const bool hit = acc16[mt][nt][j] >= tau;
                const uint64_t mk = __builtin_amdgcn_ballot_w64(hit);
                if (mk != 0ull) {
                  const uint32_t pos = wave_cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
                  if (hit) {
                    const uint2 rec = make_uint2(__float_as_uint(acc16[mt][nt][j]), rc + (uint32_t)(nt * 16));
                    asm volatile("ds_write_b64 %0, %1 offset:1024" ::"v"(wb_a + 8u * pos), "v"(rec) : "memory");
                  }
                  wave_cnt += (uint32_t)__popcll(mk);
                }
              }
              if (wave_cnt > (uint32_t)(LCAPE - 64 * TN16)) flush();   // (a step adds up to TN16 x 64 records)
            }
          }
      }
      SV_PHASE(3)
      flush();
      SV_PHASE(4)
    }
    if constexpr (EPI == 0) {
      float4* rrec = reinterpret_cast<float4*>(lds);                         // [BM] {||q||^2, exact limit, screening bound, -}
      uint32_t* rowcnt = reinterpret_cast<uint32_t*>(rrec + BM);             // [BM] survivors per row -> next free global slot
      float* cnl = reinterpret_cast<float*>(rowcnt + BM);                    // [BN] column norms
      float* taul = cnl + BN;                                                // [BM] screening bounds, contiguous (16-B reads)
      uint2* wlist = reinterpret_cast<uint2*>(taul + BM) + (size_t)w * (LCAP + 1);  // this wave's hit list (+1 dump slot)
      if (tid < BM) {
        const int j = tid;
        rrec[j] = make_float4(st_q2, st_lim, st_tau, 0.f);
        rowcnt[j] = 0u;
        taul[j] = st_tau;
      }
      float cnh[TN];
#pragma unroll
      for (int nt = 0; nt < TN; ++nt) {
        cnh[nt] = BIAS ? 0.f : cn[nt] * half_scale;                  // BIAS: already inside the accumulators
        if (!BIAS && wm == 0) cnl[wn * (32 * TN) + nt * 32 + i] = cn[nt];   // both half-waves hold the same value
      }
      __syncthreads();
      uint32_t wave_cnt = 0;  // wave-uniform: only updated under wave-uniform control flow
      // this lane's 16 * TM screening bounds, fetched up front with 16-B reads (accumulator element r of tile mt belongs to
      // row mt*32 + 8*(r>>2) + 4*kk + (r&3): four consecutive rows per (mt, r>>2)) -- a per-iteration LDS read put ~100
      // cycles of latency into each of the 32 screening steps (two waves per SIMD cannot hide it)
      float4 tq[TM][4];
#pragma unroll
      for (int mt = 0; mt < TM; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          tq[mt][g] = *reinterpret_cast<const float4*>(taul + wm * (32 * TM) + mt * 32 + 8 * g + 4 * kk);
#pragma unroll
      for (int mt = 0; mt < TM; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t lrow16 = (uint32_t)(wm * (32 * TM) + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk) << 16;
          const float4 tq4 = tq[mt][r >> 2];
          const float tau = (r & 3) == 0 ? tq4.x : (r & 3) == 1 ? tq4.y : (r & 3) == 2 ? tq4.z : tq4.w;
          float av[TN], dd[TN];
#pragma unroll
          for (int nt = 0; nt < TN; ++nt) {
            av[nt] = acc[mt][nt][r];
            dd[nt] = BIAS ? av[nt] : av[nt] - cnh[nt];
          }
          float best = dd[0];
#pragma unroll
          for (int nt = 1; nt < TN; ++nt) best = fmaxf(best, dd[nt]);
          if (__builtin_amdgcn_ballot_w64(best >= tau) != 0ull) {
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) {
              const bool hit = dd[nt] >= tau;
              const uint64_t mk = __builtin_amdgcn_ballot_w64(hit);
              if (mk != 0ull) {
                uint32_t pos = wave_cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
                pos = pos < (uint32_t)LCAP ? pos : (uint32_t)LCAP;   // beyond the list: the dump slot (the block turns dense below)
                if (hit)
                  wlist[pos] = make_uint2(__float_as_uint(av[nt]), lrow16 | (uint32_t)(wn * (32 * TN) + nt * 32 + i));
                wave_cnt += (uint32_t)__popcll(mk);
              }
            }
          }
        }
      }
      // pass 2a: exact test of this wave's hits, dense (the list is wave-private: no barrier needed before reading it)
      const uint32_t n_w = wave_cnt <= (uint32_t)LCAP ? wave_cnt : 0u;   // a dense block abandons its (truncated) list
      for (uint32_t t = (uint32_t)l; t < n_w; t += 64u) {
        uint2 rec = wlist[t];
        const int lrow = (int)(rec.y >> 16);
        const float4 rr = rrec[lrow];
        const float v = BIAS ? __fmaf_rn(-2.f, __uint_as_float(rec.x) * inv_scale, rr.x)
                             : sv_d2_screen(rr.x, cnl[rec.y & 0xffffu], __uint_as_float(rec.x) * inv_scale);
        if (v <= rr.y && v < INFINITY) {   // +inf: padding columns beyond N (admitted by the screen when thr = +inf)
          atomicAdd(&rowcnt[lrow], 1u);
          rec.x = __float_as_uint(v);
        } else {
          rec.y = 0xffffffffu;   // screened in by the slack only
        }
        wlist[t] = rec;
      }
      const bool dense = wave_cnt > (uint32_t)LCAP;   // wave-uniform
      if (dense) {
        // (the scale is laundered through an empty asm so that the compiler does not keep 128 values of pass 1 or of this
        //  walk alive for the next one: that spilled the common path)
        float isc = inv_scale;
        asm volatile("" : "+v"(isc));
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lrow = wm * (32 * TM) + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) {
              const float4 rr = rrec[lrow];
              const float v = BIAS ? __fmaf_rn(-2.f, acc[mt][nt][r] * isc, rr.x)
                                   : sv_d2_screen(rr.x, cn[nt], acc[mt][nt][r] * isc);
              if (v <= rr.y && v < INFINITY) atomicAdd(&rowcnt[lrow], 1u);
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the 32 row-record loads from being hoisted (register pressure)
          }
      }
      // PERSIST: this wave's DMA pieces of the next tile's head have landed by now (requested before pass 1; loads retire
      // in order); the barrier below makes that true for every wave, so the next tile starts without a memory wait
      if (PERSIST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid < BM) {
        const uint32_t c = rowcnt[tid];
        rowcnt[tid] = (c > 0u) ? atomicAdd(&cand_cnt[m0 + tid], c) : 0u;  // rows >= M never count
      }
      __syncthreads();
      for (uint32_t t = (uint32_t)l; t < n_w; t += 64u) {
        const uint2 rec = wlist[t];
        if (rec.y != 0xffffffffu) {
          const int lrow = (int)(rec.y >> 16);
          const uint32_t slot = atomicAdd(&rowcnt[lrow], 1u);
          if (slot < (uint32_t)cap) {
            const int64_t row = m0 + lrow;
            cand_d2[row * cap + slot] = __uint_as_float(rec.x);
            cand_id[row * cap + slot] = (uint32_t)grow(n0 + (int64_t)(rec.y & 0xffffu));
          }
        }
      }
      if (dense) {
        float isc = inv_scale;
        asm volatile("" : "+v"(isc));
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lrow = wm * (32 * TM) + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) {
              const float4 rr = rrec[lrow];
              {
                const float v = BIAS ? __fmaf_rn(-2.f, acc[mt][nt][r] * isc, rr.x)
                                     : sv_d2_screen(rr.x, cn[nt], acc[mt][nt][r] * isc);
                if (v <= rr.y && v < INFINITY) {
                  const uint32_t slot = atomicAdd(&rowcnt[lrow], 1u);
                  if (slot < (uint32_t)cap) {
                    const int64_t row = m0 + lrow;
                    cand_d2[row * cap + slot] = v;
                    cand_id[row * cap + slot] = (uint32_t)grow(n0 + wn * (32 * TN) + nt * 32 + i);
                  }
                }
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
      }
    }   // EPI == 0
    SV_PHASE(5)  // reservation + pass 2b
    if (!PERSIST || seq_next >= seq_total) break;
    seq = seq_next;
    tm = tm_next;
    tn = tn_next;
    rev = rev_of(seq);
  }   // tile loop
#undef SV_F16_NEXT_TILE
}

template <class C>
static int launch_f16_filter(segvlad_ctx* ctx, const uint16_t* Qh, const uint16_t* Rh, int M, int n_sample, int d, int b_stride,
                             float inv_scale, const float* qn, const float* rn, const float* thr, int64_t thr_ld,
                             float eps_mult, float c_eps, float rn_max, uint32_t* cand_cnt, float* cand_d2, uint32_t* cand_id,
                             int cap) {
  constexpr int BM = C::BM, BN = C::BN, WM = C::WM, WN = C::WN, KFL = C::KFL;
  constexpr bool PERSIST = C::PERSIST;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (n_sample + BN - 1) / BN;
  // tile walk of the persistent kernel (f16_walk.h): bit 0 = query-block-resident order, bit 1 = serpentine k
  // default 3: measured on 10 000 x 1 M x 1024 (rocprofv3 FETCH_SIZE, calibrated; tools/pmc_walk.sh): L2 fills of the full-level
  // launch 42.7 GB (walk 0) / 45.1 GB (2: serpentine alone) / 26.3 GB (3), at the same speed (18.39 / 18.34 ms per search's filter
  // launches, interleaved A/B)
  // deep rows (KFL): serpentine k alone.  Measured 10 000 x 46 875 x 98 304 (config2's filter launches per step, tools/walk_sweep_cfg2.sh):
  // walk 2 -> 93.6 ms, 0 -> 94.4-94.9, 3 -> 100.9-101.7, 1 -> 103.6, 4 -> 102.9, 5 / 6 / 7 -> 110.9 / 111.6 / 116.6; L2 fills 260-290 GB per
  // launch either way (a query block is 8 x 50 MB there: "resident" means nothing at that depth, and the resident order makes the 32
  // workgroups of an XCD meet a NEW database block at every step)
  int walk = PERSIST ? (ctx->opt.f16_walk >= 0 ? (ctx->opt.f16_walk & 7) : (KFL > 0 ? 2 : 3)) : 0;
  // 8 XCDs x 32 (option f16_persist_wgs) resident workgroups, each walks its XCD's sequence
  const int pwgs = (ctx->opt.f16_persist_wgs >= 1 && ctx->opt.f16_persist_wgs <= 32) ? ctx->opt.f16_persist_wgs : 32;
  if (PERSIST) walk |= pwgs << 8;
  // (option f16_gm: the walk's block height; 0 = plain tm-fastest order, which the persistent kernels do not have)
  const F16Walk g = f16_walk_geometry(tiles_m, tiles_n, (PERSIST && ctx->opt.f16_gm == 0) ? 4 : ctx->opt.f16_gm, walk);
  const int64_t tiles = f16_walk_grid(g, PERSIST ? pwgs : 0);
  if (g.seq_total > 0x7fffffffLL || tiles > 0x7fffffffLL) return ctx->fail(SEGVLAD_ERR_LIMIT, "f16 filter: too many tiles");
  const int gm = g.gm, seq_total = (int)g.seq_total;
  const size_t lds = F16Lds<C>::BYTES;
  auto kern = knn_f16_filter_kernel<C>;
  float* kscr = nullptr;
  if (KFL > 0) {   // one slice per resident wave, all zero between tiles (the kernel leaves it so); zeroed here as well
    const size_t bytes = (size_t)tiles * (WM * WN) * SV_F16_KSCR_FLOATS * 4;
    SV_HIP(ctx->s_kflush.reserve(bytes));
    SV_HIP(hipMemsetAsync(ctx->s_kflush.p, 0, bytes, ctx->stream));
    kscr = ctx->s_kflush.as<float>();
  }
  if (lds > 64 * 1024)
    SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), (size_t)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(64 * WM * WN), lds, ctx->stream, Qh, Rh, M, n_sample, d, b_stride, tiles_m,
                     gm, seq_total, walk, inv_scale, qn, rn, thr, thr_ld, eps_mult, c_eps, rn_max, cand_cnt, cand_d2, cand_id, cap,
                     ctx->f16_scale_dev, kscr);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ---- which kernel a launch takes: the ONE place that knows the rule ---------------------------------------------------
// Measurements behind it: batches (M > 128) whose launch has >= 1024 tiles of 256 x 256 fill the persistent
// kernel (10 000 x 1 M x 1024: 21.5 ms of filter launches against 22.5 for the plain 256 x 256 kernel in round 2, 18 ms since
// round 4), smaller levels take its non-persistent form; one query image per pass (M <= 128) streams the database once: 0.41 ms
// on 128 x 128 tiles against 0.51 on 256 x 256.  Deep rows (sv_f16_kblock: d >= 4096, raw K*D descriptors) accumulate in
// blocks, which keeps the filter's error margin -- and with it the refine band -- as tight as at d = 1024 (sv_f16_c_eps):
// 10 000 x 50 000 x 98 304, filter launches: 147 ms for 4 waves of 64 x 64 on 128 x 128 tiles (rounds 2-3; still the kernel
// when the norms are too unbalanced for the bias), 126 ms for 8 waves on 256 x 128 tiles with a second accumulator set
// (round 4; 125 ms with the DMA through buffer resources), and launches that fill the persistent batch kernel take THAT with
// the blocks flushed into a global scratch (round 6b, KFL: 780 vs 667 TF algorithmic).
// The biased kernels need the search's norms balanced (bias_ok: prepare_queries, search.hip).  skip = 16: the launch runs over
// the complement of the stride-16 sample (option level_carry); only the biased batch and deep-row kernels have that form.
F16Choice sv_choose_f16_kernel(const SvOptions& o, bool bias_ok, int M, int64_t n_rows, int d, int b_stride, int skip) {
  const bool deep = sv_f16_kblock(o, d) != 0;
  const bool fills = (int64_t)((M + 255) / 256) * ((n_rows + 255) / 256) >= 1024;   // the persistent 256 x 256 kernels
  const bool flush = deep && (o.f16_deep_cfg < 0 || o.f16_deep_cfg == 5) && bias_ok && M > 128 && fills;
  // BUF kernels: every piece offset of a 256-row tile in 32 bits (row pitch d * b_stride fp16 on the database side; the complement
  // form steps over one row in 16: twice the pitch bounds it)
  const bool buf_ok = o.f16_buf != 0 && (int64_t)256 * d * (skip ? 2 : b_stride) * 2 + 4096 < (int64_t)0xffffffffLL;
  if (skip) {
    if (skip != 16 || b_stride != 1) return {F16Kernel::None, "the complement form exists for the stride-16 sample of contiguous rows only"};
    if (!o.level_carry || M <= 128 || n_rows <= 0 || !bias_ok) return {F16Kernel::None, "the complement form needs level_carry and a biased batch kernel"};
    if (deep) return {flush ? F16Kernel::DeepFlushComplement : buf_ok ? F16Kernel::DeepBlockedBufComplement : F16Kernel::DeepBlockedComplement, nullptr};
    if ((o.f16_cfg >= 0 && o.f16_cfg != 250) || !fills) return {F16Kernel::None, "the complement form needs the persistent batch kernel"};
    return {F16Kernel::BatchComplement, nullptr};
  }
  if (deep) {
    if (flush) return {F16Kernel::DeepFlush, nullptr};
    if (bias_ok && M > 128) return {buf_ok ? F16Kernel::DeepBlockedBuf : F16Kernel::DeepBlocked, nullptr};
    return {F16Kernel::DeepUnbiased, nullptr};
  }
  switch (o.f16_cfg >= 0 ? o.f16_cfg : (M > 128 ? 250 : M > 64 ? 63 : 62)) {
    case 250:
      if (!bias_ok) return {fills ? F16Kernel::BatchUnbiased : F16Kernel::BatchUnbiasedSmall, nullptr};
      return {fills ? F16Kernel::BatchDefault : F16Kernel::BatchSmall, nullptr};
    case 62: return {F16Kernel::OneImage64, nullptr};
    case 63: return {F16Kernel::OneImage128, nullptr};
#ifdef SEGVLAD_ABLATIONS
    case 93: return {F16Kernel::ProbePhases, nullptr};
    case 94: return {F16Kernel::ProbeNoEpilogue, nullptr};
    case 95: return {F16Kernel::ProbeNoEpilogueNoDma, nullptr};
#endif
    default: return {F16Kernel::None, "no such fp16 filter configuration (option f16_cfg)"};
  }
}

// f(C{}) for the configuration type C of kernel k
template <class F>
static auto f16_with_config(F16Kernel k, F&& f) -> decltype(f(F16BatchDefault{})) {
  switch (k) {
    case F16Kernel::BatchDefault: return f(F16BatchDefault{});
    case F16Kernel::BatchComplement: return f(F16BatchComplement{});
    case F16Kernel::BatchSmall: return f(F16BatchSmall{});
    case F16Kernel::BatchUnbiased: return f(F16BatchUnbiased{});
    case F16Kernel::BatchUnbiasedSmall: return f(F16BatchUnbiasedSmall{});
    case F16Kernel::DeepFlush: return f(F16DeepFlush{});
    case F16Kernel::DeepFlushComplement: return f(F16DeepFlushComplement{});
    case F16Kernel::DeepBlockedBuf: return f(F16DeepBlockedBuf{});
    case F16Kernel::DeepBlocked: return f(F16DeepBlocked{});
    case F16Kernel::DeepBlockedBufComplement: return f(F16DeepBlockedBufComplement{});
    case F16Kernel::DeepBlockedComplement: return f(F16DeepBlockedComplement{});
    case F16Kernel::DeepUnbiased: return f(F16DeepUnbiased{});
    case F16Kernel::OneImage64: return f(F16OneImage64{});
    case F16Kernel::OneImage128: return f(F16OneImage128{});
#ifdef SEGVLAD_ABLATIONS
    case F16Kernel::ProbePhases: return f(F16ProbePhases{});
    case F16Kernel::ProbeNoEpilogue: return f(F16ProbeNoEpilogue{});
    case F16Kernel::ProbeNoEpilogueNoDma: return f(F16ProbeNoEpilogueNoDma{});
#endif
    case F16Kernel::None: break;
  }
  return decltype(f(F16BatchDefault{}))();
}

// Can the LAST level of a batch search run over the complement of the stride-16 sample (skip = 16)?
bool sv_f16_filter_skip_ok(const segvlad_ctx* ctx, int M, int64_t n_rows, int d) {
  return sv_choose_f16_kernel(ctx->opt, ctx->f16_bias_ok, M, n_rows, d, 1, 16).kernel != F16Kernel::None;
}

// The accumulation-block length the error constant of a search over rows of d has to cover: that of the kernel a launch takes
// which fills the machine, with the bias allowed -- the longest of any launch of the search (the flushed blocks of the
// persistent deep-row kernel are longer than the register-blocked kernels' that the smaller levels run).
int sv_f16_eps_kblock(const SvOptions& o, int d) {
  static_assert(f16_kblock_of<F16DeepFlush>() >= f16_kblock_of<F16DeepBlocked>() && f16_kblock_of<F16DeepBlocked>() == f16_kblock_of<F16DeepUnbiased>() &&
                    f16_kblock_of<F16DeepBlocked>() == SV_F16_KBLOCK,
                "the largest launch has the longest blocks");
  const F16Choice c = sv_choose_f16_kernel(o, true, 1 << 20, (int64_t)1 << 40, d, 1, 0);
  return f16_with_config(c.kernel, [](auto cfg) { return f16_kblock_of<decltype(cfg)>(); });
}

int sv_launch_f16_filter(segvlad_ctx* ctx, const uint16_t* Qh, const uint16_t* Rh, int M, int n_sample, int d, int b_stride,
                         float inv_scale, const float* qn, const float* rn, const float* thr, int64_t thr_ld, float eps_mult,
                         float c_eps, float rn_max, uint32_t* cand_cnt, float* cand_d2, uint32_t* cand_id, int cap, int skip) {
  if (M <= 0 || n_sample <= 0) return SEGVLAD_OK;
  // (skip: operand row j = database row j + j / 15 + 1, n_sample = the number of rows that are not multiples of 16: see the kernel's SKIP)
  const F16Choice c = sv_choose_f16_kernel(ctx->opt, ctx->f16_bias_ok, M, n_sample, d, b_stride, skip);
  if (c.kernel == F16Kernel::None)
    return ctx->fail(skip ? SEGVLAD_ERR_STATE : SEGVLAD_ERR_ARG, "f16 filter (f16_cfg %d, %d x %d x %d, skip %d): %s", ctx->opt.f16_cfg, M, n_sample, d, skip, c.why);
  auto launch = [&](auto cfg) {
    return launch_f16_filter<decltype(cfg)>(ctx, Qh, Rh, M, n_sample, d, b_stride, inv_scale, qn, rn, thr, thr_ld, eps_mult, c_eps, rn_max, cand_cnt,
                                            cand_d2, cand_id, cap);
  };
#ifdef SEGVLAD_ABLATIONS
  if (c.kernel == F16Kernel::ProbePhases) {   // synchronises and prints the shares of the kernel's phases
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c8[8];
    SV_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sv_f16_phase_cycles), z, sizeof(z)));
    const int rc = launch(F16ProbePhases{});
    SV_HIP(hipStreamSynchronize(ctx->stream));
    SV_HIP(hipMemcpyFromSymbol(c8, HIP_SYMBOL(sv_f16_phase_cycles), sizeof(c8)));
    double tot = 0;
    for (int k = 0; k < 6; ++k) tot += (double)c8[k];
    fprintf(stderr, "[f16 filter phases] M=%d n=%d: head-wait %.1f%% main %.1f%% stage %.1f%% pass1 %.1f%% pass2a %.1f%% rest %.1f%% (%.3g cycles/WG-sum)\n",
            M, n_sample, 100 * c8[0] / tot, 100 * c8[1] / tot, 100 * c8[2] / tot, 100 * c8[3] / tot, 100 * c8[4] / tot, 100 * c8[5] / tot, tot);
    return rc;
  }
#endif
  return f16_with_config(c.kernel, launch);
}
