// Exact kNN, large-database path: the refine lists of the selects (knn_select_kernels.hip) evaluated exactly -- the sequential fp32
// fma chain of the matrix path (knn_dev.h: sv_dot_seq_, SV_LDS_ROW_WALK; small_pass_dev.h: chain_step), sv_d2 with the stored norms,
// (distance, id) order, top k (knn_dev.h: sv_write_topk).
//   refine_exact_kernel<QLDS>         one workgroup per list, one thread per candidate row; the query row in LDS (d up to ~38k) or not
//   refine_exact_wide_kernel<KC, D>   deep rows (raw K*D descriptors): the rows fetched coalesced into an LDS tile, a lane per row
//   refine_exact_small_kernel         ONE query image per pass (<= 128 lists): a list dealt to `parts` workgroups, the last one
//                                     orders it; finishes the rows the select flagged itself (small_pass_dev.h)
//   sv_refine_small_repair, sv_launch_refine_exact
#include <stdlib.h>

#include "ctx.h"
#include "knn_dev.h"
#include "small_pass_dev.h"

// One thread per candidate row, the chain of knn_dev.h: sv_dot_seq_<32> (32 x 16 bytes of the row in flight per lane) where the
// row is whole bursts, one float4 at a time otherwise.  The query row is cached in LDS (QLDS; d up to ~38k).
// only_rows != null: rows whose flag is clear are left untouched (second refinement tier).
template <bool QLDS>
__global__ __launch_bounds__(256) void refine_exact_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                           const float* __restrict__ qn, const float* __restrict__ rn,
                                                           const uint32_t* __restrict__ ref_cnt,
                                                           const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                           float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                           const uint32_t* __restrict__ only_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);                                     // [d] when QLDS
  uint64_t* a = reinterpret_cast<uint64_t*>(smem + (QLDS ? (size_t)d * 4 : 0));   // [rpad]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (only_rows && !only_rows[row]) return;
  const int n = (int)ref_cnt[row];
  const int np2 = sv_np2(n);   // (<= rpad)
  if (QLDS)
    for (int j = tid; j < d; j += 256) qs[j] = Q[row * d + j];
  for (int j = tid; j < np2; j += 256) a[j] = SV_WORD_NONE;
  __syncthreads();
  const float q2 = qn[row];
  const float4* qp = QLDS ? reinterpret_cast<const float4*>(qs) : reinterpret_cast<const float4*>(Q + row * d);
  const int n4 = d >> 2;
  for (int j = tid; j < n; j += 256) {
    const uint32_t id = ref_id[row * rcap + j];
    const float4* rp = reinterpret_cast<const float4*>(R + (size_t)id * d);
    const float acc = (n4 & 31) == 0 ? sv_dot_seq_<32>(qp, rp, n4) : sv_dot_seq_<1>(qp, rp, n4);
    a[j] = sv_word(sv_d2(q2, rn[id], acc), id);
  }
  sv_bitonic(a, np2, tid);
  sv_write_topk<false>(a, n, k, d2_out, idx_out, row, tid);
}

// Deep rows (raw K*D descriptors: d = 98 304 is 384 KiB per row, far beyond the LDS and -- one row per lane -- beyond what
// L1 can keep of 256 private streams): the same sequential chain, with the candidate rows fetched COALESCED (KC * 4 bytes
// of a row per step: C4 lanes x 16 B) into an LDS tile [64 rows][KC (+4 pad)], double buffered, which the 64 lanes of wave 0
// then walk ONE ROW EACH (conflict-free ds_read_b128: the row stride is 4 banks mod 64); all four waves load.
// What bounds it is bytes in flight: one workgroup per CU (the tile) with one step of 32 KiB outstanding ran at 1.4-1.8 TB/s
// -- piece size, a time skew between the rows and the 3 * 2^17-byte row pitch made no difference, and
// tools/ubench/gather_bw.hip reaches 7 TB/s on the same addresses with 256 KiB per CU in flight.  So the loads run DEPTH
// steps ahead in a register ring (DEPTH x NP float4 per thread: 128 KiB per CU at DEPTH = 4), and only the step that is due
// is written to the LDS tile.  d % KC == 0.
// Its LDS, for the kernel's pointers and the launcher's byte count: [2][ROWS][LDR] tile floats, [2][KC] query floats, [ROWS] ids,
// then the list's rpad sort words.
template <int KC>
struct RefineWideLds {
  static constexpr int ROWS = 64, LDR = KC + 4;
  static constexpr int TILE = 2 * ROWS * LDR, QS = 2 * KC;           // floats
  static constexpr size_t FIXED = (size_t)(TILE + QS + ROWS) * 4;    // bytes in front of the sort words
};
constexpr int SV_WIDE_KC = 128;   // the instantiation sv_launch_refine_exact launches (DEPTH = 4)
template <int KC, int DEPTH>
__global__ __launch_bounds__(256) void refine_exact_wide_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                                const float* __restrict__ qn, const float* __restrict__ rn,
                                                                const uint32_t* __restrict__ ref_cnt,
                                                                const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                                float* __restrict__ d2_out, int64_t* __restrict__ idx_out,
                                                                const uint32_t* __restrict__ only_rows) {
  using L = RefineWideLds<KC>;
  constexpr int ROWS = L::ROWS, LDR = L::LDR, C4 = KC / 4;   // C4 16-byte pieces per row and step
  constexpr int NP = ROWS * C4 / 256;                    // pieces per thread and step
  constexpr int RSTEP = 256 / C4;                        // tile rows between two pieces of a thread
  static_assert(C4 <= 64 && 64 % C4 == 0 && NP * 256 == ROWS * C4, "a wave covers whole rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);                                 // [2][ROWS][LDR]
  float* qs = tile + L::TILE;                                                   // [2][KC]
  uint32_t* ids = reinterpret_cast<uint32_t*>(qs + L::QS);                      // [ROWS]
  uint64_t* a = reinterpret_cast<uint64_t*>(ids + ROWS);                        // [rpad]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (only_rows && !only_rows[row]) return;
  const int n = (int)ref_cnt[row];
  const int np2 = sv_np2(n);
  for (int j = tid; j < np2; j += 256) a[j] = SV_WORD_NONE;
  const float q2 = qn[row];
  const float* qrow = Q + row * d + (tid < C4 ? tid * 4 : 0);
  const int nch = d / KC;
  const int seg = tid % C4, lrow0 = tid / C4;   // piece u of this thread: tile row lrow0 + RSTEP u, 16-byte segment seg
  for (int base = 0; base < n; base += ROWS) {
    const int cnt = (n - base < ROWS) ? (n - base) : ROWS;
    __syncthreads();   // the previous pass is done with ids[] and the tile
    if (tid < cnt) ids[tid] = ref_id[row * rcap + base + tid];
    __syncthreads();
    // (no per-piece predication: a branch around every load makes the compiler wait for each one.  Tile rows beyond the
    //  list re-read candidate 0 -- L2 hits -- and are never looked at; every thread carries a query piece, lanes >= C4 a
    //  duplicate of piece 0 that is never stored)
    const float* src[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int lr = lrow0 + RSTEP * u;
      src[u] = R + (size_t)ids[lr < cnt ? lr : 0] * d + seg * 4;
    }
    // The ring is four NAMED register sets and the step is a macro instantiated once per set: hipcc 7.2 sends a
    // [DEPTH][NP] array that is indexed through a lambda parameter to scratch memory (seen in the ISA: scratch_load/_store
    // around every piece, vmcnt(0) after every load).
    static_assert(DEPTH == 4 && NP == 8, "four named ring sets of eight named pieces");
#define SV_WG_DECL(X) float4 g##X##0, g##X##1, g##X##2, g##X##3, g##X##4, g##X##5, g##X##6, g##X##7, q##X
    SV_WG_DECL(A);
    SV_WG_DECL(B);
    SV_WG_DECL(C);
    SV_WG_DECL(D);
#define SV_WG_LOAD(X, c_)                                                          \
    do {                                                                           \
      const size_t o_ = (size_t)(c_) * KC;                                         \
      g##X##0 = *reinterpret_cast<const float4*>(src[0] + o_);                     \
      g##X##1 = *reinterpret_cast<const float4*>(src[1] + o_);                     \
      g##X##2 = *reinterpret_cast<const float4*>(src[2] + o_);                     \
      g##X##3 = *reinterpret_cast<const float4*>(src[3] + o_);                     \
      g##X##4 = *reinterpret_cast<const float4*>(src[4] + o_);                     \
      g##X##5 = *reinterpret_cast<const float4*>(src[5] + o_);                     \
      g##X##6 = *reinterpret_cast<const float4*>(src[6] + o_);                     \
      g##X##7 = *reinterpret_cast<const float4*>(src[7] + o_);                     \
      q##X = *reinterpret_cast<const float4*>(qrow + o_);                          \
    } while (0)
#define SV_WG_STORE(X, buf_)                                                       \
    do {                                                                           \
      float* t_ = tile + ((size_t)(buf_) * ROWS + lrow0) * LDR + seg * 4;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 0 * LDR) = g##X##0;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 1 * LDR) = g##X##1;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 2 * LDR) = g##X##2;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 3 * LDR) = g##X##3;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 4 * LDR) = g##X##4;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 5 * LDR) = g##X##5;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 6 * LDR) = g##X##6;          \
      *reinterpret_cast<float4*>(t_ + (size_t)RSTEP * 7 * LDR) = g##X##7;          \
      if (tid < C4) *reinterpret_cast<float4*>(qs + (buf_) * KC + tid * 4) = q##X; \
    } while (0)
    // one step: multiply step c out of tile buffer c & 1, move step c + 1 (ring set XN) into the other buffer, request
    // step c + 1 + DEPTH into the set that just became free
#define SV_WG_MUL(c) \
    if (tid < cnt) SV_LDS_ROW_WALK(tile + ((size_t)((c) & 1) * ROWS + tid) * LDR, qs + ((c) & 1) * KC, C4, 8, acc)
    // steady state (no conditions on the loads: the compiler's wait counts then leave the three younger steps in flight)
#define SV_WG_STEP_FULL(c_, XN)                                                                            \
    do {                                                                                                   \
      const int c = (c_);                                                                                  \
      SV_WG_MUL(c)                                                                                         \
      SV_WG_STORE(XN, (c + 1) & 1);                                                                        \
      SV_WG_LOAD(XN, c + 1 + DEPTH);                                                                       \
      __syncthreads();                                                                                     \
    } while (0)
#define SV_WG_STEP(c_, XN)                                                                                 \
    do {                                                                                                   \
      const int c = (c_);                                                                                  \
      if (c < nch) {                                                                                       \
        SV_WG_MUL(c)                                                                                       \
        if (c + 1 < nch) {                                                                                 \
          SV_WG_STORE(XN, (c + 1) & 1);   /* waits for the loads of step c + 1 only */                     \
          if (c + 1 + DEPTH < nch) SV_WG_LOAD(XN, c + 1 + DEPTH);                                          \
        }                                                                                                  \
        __syncthreads();                                                                                   \
      }                                                                                                    \
    } while (0)
    float acc = 0.f;
    // set A holds steps 0, 4, 8, ...; B 1, 5, ...; C 2, 6, ...; D 3, 7, ...
    SV_WG_LOAD(A, 0);
    if (1 < nch) SV_WG_LOAD(B, 1);
    if (2 < nch) SV_WG_LOAD(C, 2);
    if (3 < nch) SV_WG_LOAD(D, 3);
    SV_WG_STORE(A, 0);
    if (4 < nch) SV_WG_LOAD(A, 4);
    __syncthreads();
    int c0 = 0;
    for (; c0 + 3 + 1 + DEPTH < nch; c0 += 4) {   // every load of these four steps exists
      SV_WG_STEP_FULL(c0, B);
      SV_WG_STEP_FULL(c0 + 1, C);
      SV_WG_STEP_FULL(c0 + 2, D);
      SV_WG_STEP_FULL(c0 + 3, A);
    }
    for (; c0 < nch; c0 += 4) {                    // the last steps: nothing (or not everything) left to request
      SV_WG_STEP(c0, B);
      SV_WG_STEP(c0 + 1, C);
      SV_WG_STEP(c0 + 2, D);
      SV_WG_STEP(c0 + 3, A);
    }
#undef SV_WG_STEP
#undef SV_WG_STEP_FULL
#undef SV_WG_MUL
#undef SV_WG_STORE
#undef SV_WG_LOAD
#undef SV_WG_DECL
    if (tid < cnt) {
      const uint32_t id = ids[tid];
      a[base + tid] = sv_word(sv_d2(q2, rn[id], acc), id);
    }
  }
  sv_bitonic(a, np2, tid);
  sv_write_topk<false>(a, n, k, d2_out, idx_out, row, tid);
}

// A handful of queries (one query image per pass): fewer lists than CUs, and a list walked by ONE workgroup is one memory
// round trip after the other (59 us for 240 rows of 1024 floats).  Here a list is dealt to `parts` workgroups, 32 rows each:
// a workgroup requests 1024 floats of each of its 32 rows in ONE burst (thread t: 16 bytes of row 2 j + (t >> 7), in both
// 512-float halves: 32 coalesced loads in flight per thread, one round trip per 1024 floats), parks one half at a time in an
// LDS tile [32][516], and 32 lanes walk one row each (the same sequential fp32 chain; the query's floats are LDS
// broadcasts).  The keys go to global memory as device-scope stores; the workgroup that takes the last ticket of its query
// reads them back, sorts them and writes the top k.  d % 1024 == 0.  tick[] is all zero before and after.
// Measured (50 queries x ~240 rows, 1 M x 1024 index): 59 us -> 34-38 us; what is left is a chain of ~7 dependent memory
// round trips (list length + ids, rows, key stores, ticket, key loads, results) around 5 us of arithmetic.
// tick: ctx->s_ref_tick (small_pass_dev.h).  Its LDS, for the kernel's pointers and the launcher's byte count: [ROWS][LDR] tile floats,
// the list's rpad sort words, [2 KC] query floats.
struct RefineSmallLds {
  static constexpr int ROWS = 32, KC = 512, LDR = KC + 4;
  static constexpr int TILE = ROWS * LDR, QS = 2 * KC;               // floats
  static constexpr size_t FIXED = (size_t)(TILE + QS) * 4;          // bytes besides the sort words
};
__global__ __launch_bounds__(256) void refine_exact_small_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                                 const float* __restrict__ qn, const float* __restrict__ rn,
                                                                 const uint32_t* __restrict__ ref_cnt,
                                                                 const uint32_t* __restrict__ ref_id, int rcap, int rpad, int k,
                                                                 float* __restrict__ d2_out, int64_t* __restrict__ idx_out, int parts,
                                                                 uint64_t* __restrict__ gkeys, uint32_t* __restrict__ tick,
                                                                 uint32_t* __restrict__ fail_rows, uint32_t* __restrict__ fail_count,
                                                                 SvSmallFinish fz) {
  using L = RefineSmallLds;
  constexpr int ROWS = L::ROWS, KC = L::KC, LDR = L::LDR;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);                  // [ROWS][LDR]
  uint64_t* a = reinterpret_cast<uint64_t*>(tile + L::TILE);     // [rpad]
  __shared__ uint32_t ids[ROWS];
  __shared__ int last;
  const int tid = threadIdx.x;
  // part-major: the first workgroups of the grid are part 0 of EVERY list, then part 1, ... -- the parts that hold rows (a band of ~270
  // rows: parts 0-8 of 16) are all resident in the first round of workgroups, the empty ones come last and leave at once.  Row-major
  // (rounds 3-5) put all 16 parts of lists 0-31 into the 512 resident slots and made lists 32-49 wait for them (round 6: 40 -> 33 us).
  const int nlists = (int)(gridDim.x / parts);
  const int64_t row = blockIdx.x % nlists;
  const int base = (int)(blockIdx.x / nlists) * ROWS;
  // the list's length and this workgroup's slice of it are requested together (the slice lies inside the list's rcap slots
  // whatever the length; entries beyond it are not looked at)
  const uint32_t idv = tid < ROWS ? ref_id[row * rcap + base + tid] : 0u;
  // fz.on (round 6, second step: the pass WITHOUT small_tail_kernel -- every kernel boundary of this chain costs 4-5 us, whatever the
  // kernel does): the rows the select flagged are finished HERE, by the row's own `parts` workgroups -- a band that outgrew the
  // first tier: every part evaluates its slice of the candidate list, the last one sorts; a row flagged for the redo: exact brute
  // force, every part a slice of the index, the last one merges (small_pass_dev.h; the same chain, sv_d2, (distance, id) order).
  // The two flags are requested with the list's length: no extra round trip on the common path.
  const uint32_t f_fail = fz.on ? fail_rows[row] : 0u, f_rovf = fz.on ? fz.rovf_rows[row] : 0u;
  const int n = (int)ref_cnt[row];
  if (f_fail | f_rovf) {   // (workgroup-uniform)
    const int p = (int)(blockIdx.x / nlists);
    static_assert(L::FIXED >= 65536 + ST_KC * 4, "the flagged-row carving below lies inside the kernel's fixed LDS");
    uint64_t* a2 = reinterpret_cast<uint64_t*>(smem);                 // <= 8192 words of sort scratch
    float* qs2 = reinterpret_cast<float*>(smem + 65536);              // 1024 floats
    uint64_t* best2 = a2 + 2048;                                      // (brute force: the sort scratch is 2048 words)
    uint64_t* slot = fz.part2 + (size_t)row * fz.row_words;           // this row's words of the exchange buffer
    if (f_fail) sp_brute_slice(Q, R, qn, rn, fz.n_db, d, k, fz.kp, row, p, parts, slot, a2, best2, qs2, tid);
    else sp_tier2_slice(Q, R, qn, rn, d, row, p, parts, min(fz.cand_cnt[row], (uint32_t)fz.cap), fz.ref_lim[row], fz.cand_d2, fz.cand_id, fz.cap, slot,
                        qs2, tid);
    __threadfence();
    __syncthreads();
    if (tid == 0) last = (__hip_atomic_fetch_add(&tick[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(parts - 1));
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (f_fail) {
      sp_brute_merge(slot, k, fz.kp, parts, a2, best2, tid);
      sv_write_topk<true>(best2, fz.kp, k, d2_out, idx_out, row, tid);
    } else {
      const int c = (int)min(fz.cand_cnt[row], (uint32_t)fz.cap);
      const int np2 = sv_np2(c);
      for (int j = tid; j < np2; j += 256)
        a2[j] = j < c ? __hip_atomic_load(&slot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : SV_WORD_NONE;
      sv_bitonic(a2, np2, tid);
      sv_write_topk<true>(a2, np2, k, d2_out, idx_out, row, tid);
    }
    if (tid == 0) {
      __hip_atomic_store(&tick[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(&fz.stats[f_fail ? 0 : 1], 1u);
      const uint32_t tot = atomicAdd(&fz.totals[f_fail ? 0 : 1], 1u) + 1u;
      if (fz.host_totals) fz.host_totals[f_fail ? 0 : 1] = tot;   // (the pinned mirror: the latest writer's total)
    }
    return;
  }
  const int cnt = min(ROWS, n - base);
  if (cnt > 0) {
    if (tid < ROWS) ids[tid] = idv;
    __syncthreads();
    if (tid >= cnt && tid < ROWS) ids[tid] = ids[0];   // rows beyond the list re-read its first one
    __syncthreads();
    const int h = tid >> 7, off = (tid & 127) * 4;
    // (named registers: hipcc 7.2 sends a float4 g[..] filled in an unrolled loop to scratch memory here, with a vmcnt(0)
    //  behind every load)
#define SV_RS_J(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15)
#define SV_RS_SRC(j) const float* src##j = R + (size_t)ids[2 * j + h] * d + off;
#define SV_RS_LOAD(j)                                                       \
  const float4 gA##j = *reinterpret_cast<const float4*>(src##j + c0);        \
  const float4 gB##j = *reinterpret_cast<const float4*>(src##j + c0 + KC);
#define SV_RS_STORE_A(j) *reinterpret_cast<float4*>(tile + (2 * j + h) * LDR + off) = gA##j;
#define SV_RS_STORE_B(j) *reinterpret_cast<float4*>(tile + (2 * j + h) * LDR + off) = gB##j;
#define SV_RS_WALK(c_) \
  if (tid < cnt) SV_LDS_ROW_WALK(tile + tid * LDR, qs + (c_), KC / 4, 16, acc)
    SV_RS_J(SV_RS_SRC)
    // (the query's 1024 floats of the step sit in LDS beside the tile, read as broadcasts: through the scalar cache every
    //  batch of 64 floats was a cold ~0.7 us miss in front of its fmas)
    float* qs = reinterpret_cast<float*>(a + rpad);   // [2 KC]
    const float* qsrc = Q + row * d + tid * 4;
    float acc = 0.f;
    for (int c0 = 0; c0 < d; c0 += 2 * KC) {
      SV_RS_J(SV_RS_LOAD)
      const float4 qv4 = *reinterpret_cast<const float4*>(qsrc + c0);
      if (c0) __syncthreads();   // the walkers are done with the previous half
      SV_RS_J(SV_RS_STORE_A)
      *reinterpret_cast<float4*>(qs + tid * 4) = qv4;
      __syncthreads();
      SV_RS_WALK(0)
      __syncthreads();
      SV_RS_J(SV_RS_STORE_B)
      __syncthreads();
      SV_RS_WALK(KC)
    }
#undef SV_RS_WALK
#undef SV_RS_STORE_B
#undef SV_RS_STORE_A
#undef SV_RS_LOAD
#undef SV_RS_SRC
#undef SV_RS_J
    if (tid < cnt) {
      const uint32_t id = ids[tid];
      __hip_atomic_store(&gkeys[row * rcap + base + tid], sv_word(sv_d2(qn[row], rn[id], acc), id), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // The keys are device-scope (write-through) stores and device-scope loads; each wave waits for its stores to be
  // acknowledged before the barrier that precedes the ticket.  (A __threadfence() on either side is an L2 write-back +
  // invalidate on this eight-L2 part.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) last = (__hip_atomic_fetch_add(&tick[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(parts - 1));
  __syncthreads();
  if (!last) return;
  const int np2 = sv_np2(n);
  // Ordering.  Every access to gkeys / tick is an agent-scope atomic (sc1: performed at the memory side, never served from
  // an XCD's own L2), the writers wait for their key stores to be ACKNOWLEDGED (vmcnt(0)) before the barrier in front of the
  // ticket, and the reader issues its loads after its ticket returned: on this hardware that is a release / acquire chain
  // through the ticket.  The C++ model does not promise it for relaxed atomics, and a formal acq_rel ticket costs an L2
  // write-back + invalidate per workgroup (see above) -- so the protocol is CHECKED instead of trusted: gkeys holds all ones
  // wherever no key of this launch has landed (the launcher fills a new buffer so, the reader puts the fill back behind
  // every key it takes; a key is never all ones: finite distance, 32-bit id); a slot still all ones is re-read a bounded
  // number of times, and a slot that never fills FLAGS its query (fail_rows: the caller redoes flagged rows on another
  // path, exactly) and raises the sticky word tick[SV_TICK_POISON], on which the host re-initialises both buffers before
  // their next use (a key landing after the reader gave up would otherwise pass for a key of the next launch).
  int holes = 0;
  for (int j = tid; j < np2; j += 256) {
    uint64_t v = SV_WORD_NONE;
    if (j < n) {
      for (int spin = 0; spin < 4096; ++spin) {
        v = __hip_atomic_load(&gkeys[row * rcap + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v != SV_WORD_NONE) break;
      }
      if (v == SV_WORD_NONE) ++holes;
      __hip_atomic_store(&gkeys[row * rcap + j], SV_WORD_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a[j] = v;
  }
  if (tid == 0) __hip_atomic_store(&tick[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (fz.on && (fz.debug & 8) && row == 1) holes = 1;   // (tests: the path below has never been taken by the hardware)
  if (__syncthreads_or(holes)) {   // (never observed)
    if (tid == 0) __hip_atomic_store(&tick[SV_TICK_POISON], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!fz.on) {   // the row's output is left to the redo (the caller's read-back, or small_tail_kernel)
      if (tid == 0 && fail_rows) sv_flag_once_(fail_rows, fail_count, row);
      return;
    }
    // fused finish: nobody comes after this kernel -- this workgroup re-evaluates the row's whole band itself (<= rcap rows, a thread
    // per row: the same chain); the sticky word makes the NEXT pass's head refill the hand-over buffers (a key that lands late must
    // not pass for a key of that pass)
    float* qs2 = reinterpret_cast<float*>(smem);   // (the row tile is free: every part has drawn its ticket)
    for (int j0 = 0; j0 < n; j0 += 256) {
      const int j = j0 + tid;
      const uint32_t id = ref_id[row * rcap + min(j, n - 1)];
      const float acc2 = sp_chain_row(Q, d, row, R + (size_t)id * d, j < n, qs2, tid);
      if (j < n) a[j] = sv_word(sv_d2(qn[row], rn[id], acc2), id);
    }
    __syncthreads();
    if (tid == 0) atomicAdd(&fz.stats[2], 1u);
  }
  // (distance, id) order WITHOUT a sort: the keys are distinct (the id is part of them), so a key's place in the sorted list is the
  // number of smaller keys -- every thread counts that for its own one or two keys against the n keys in LDS (broadcast reads, no
  // barrier) and writes its result straight to that place.  The bitonic sort of 512 words was 45 barrier-separated stages: 9.6 us of
  // the last workgroup's 25 (round 6); the count is ~2.
  for (int j = tid; j < n; j += 256) {
    const uint64_t v = a[j];
    int place = 0;
#pragma unroll 8
    for (int t = 0; t < n; ++t) place += (a[t] < v) ? 1 : 0;
    if (place < k) {
      d2_out[row * k + place] = sv_word_d2(v);
      idx_out[row * k + place] = sv_word_id(v);
    }
  }
  for (int j = n + tid; j < k; j += 256) {   // a list shorter than k pads with (inf, -1)
    d2_out[row * k + j] = INFINITY;
    idx_out[row * k + j] = -1;
  }
}

int sv_refine_small_repair(segvlad_ctx* ctx) {
  // the hand-over buffers of refine_exact_small_kernel back to their initial state (all ones / all zero)
  if (ctx->s_ref_tick.p) SV_HIP(hipMemsetAsync(ctx->s_ref_tick.p, 0, ctx->s_ref_tick.cap, ctx->stream));
  if (ctx->s_ref_keys.p) SV_HIP(hipMemsetAsync(ctx->s_ref_keys.p, 0xff, ctx->s_ref_keys.cap, ctx->stream));
  return SEGVLAD_OK;
}

int sv_launch_refine_exact(segvlad_ctx* ctx, const float* Q, const float* R, int nq, int d, const float* qn, const float* rn,
                           const uint32_t* ref_cnt, const uint32_t* ref_id, int rcap, int k, float* d2_out, int64_t* idx_out,
                           const uint32_t* only_rows, uint32_t* fail_rows, uint32_t* fail_count, const uint32_t** poison_dev,
                           const SvSmallFinish* fz, bool* fused_done) {
  if (poison_dev) *poison_dev = nullptr;
  if (fused_done) *fused_done = false;
  if (nq <= 0) return SEGVLAD_OK;
  const int rpad = sv_np2(rcap);
  size_t lds = (size_t)d * 4 + (size_t)rpad * 8;
  using LS = RefineSmallLds;
  if (nq <= SV_TICK_ROWS && d % LS::QS == 0 && rcap <= 1024 && rcap % LS::ROWS == 0 && !only_rows) {   // one query image: lists shared by workgroups
    const int parts = rcap / LS::ROWS;
    const size_t tick_cap = ctx->s_ref_tick.cap;
    SV_HIP(ctx->s_ref_tick.reserve((size_t)SV_TICK_WORDS * 4));
    if (ctx->s_ref_tick.cap != tick_cap) SV_HIP(hipMemsetAsync(ctx->s_ref_tick.p, 0, ctx->s_ref_tick.cap, ctx->stream));
    const size_t keys_cap = ctx->s_ref_keys.cap;
    SV_HIP(ctx->s_ref_keys.reserve((size_t)nq * rcap * 8));
    if (ctx->s_ref_keys.cap != keys_cap) SV_HIP(hipMemsetAsync(ctx->s_ref_keys.p, 0xff, ctx->s_ref_keys.cap, ctx->stream));
    lds = LS::FIXED + (size_t)rpad * 8;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_small_kernel), lds));
    SvSmallFinish f;   // (off)
    if (fz && fz->on && fail_rows && fused_done && k <= 1024) {
      // the flagged rows' exchange words: a row's `parts` lists of kp keys (brute force) or its `cap` candidate keys (second tier)
      f = *fz;
      f.kp = 256;
      while (f.kp < k) f.kp <<= 1;
      f.row_words = std::max<int64_t>((int64_t)parts * f.kp, f.cap);
      SV_HIP(ctx->s_tail_part.reserve((size_t)nq * f.row_words * 8));
      SV_TRY(sv_small_words(ctx));
      SV_TRY(sv_ensure_pinned_words(ctx));
      f.part2 = ctx->s_tail_part.as<uint64_t>();
      f.totals = ctx->s_tail_tick.as<uint32_t>() + SV_TAIL_TOTALS;
      f.host_totals = ctx->h_pin + SV_PIN_TOTALS;
      f.debug = ctx->opt.debug_small_tail;
      *fused_done = true;
    }
    hipLaunchKernelGGL(refine_exact_small_kernel, dim3(nq * parts), dim3(256), lds, ctx->stream, Q, R, d, qn, rn, ref_cnt, ref_id, rcap,
                       rpad, k, d2_out, idx_out, parts, ctx->s_ref_keys.as<uint64_t>(), ctx->s_ref_tick.as<uint32_t>(), fail_rows, fail_count, f);
    SV_HIP(hipGetLastError());
    if (poison_dev) *poison_dev = ctx->s_ref_tick.as<uint32_t>() + SV_TICK_POISON;
    return SEGVLAD_OK;
  }
#define SV_REFINE_ARGS dim3(nq), dim3(256), lds, ctx->stream, Q, R, d, qn, rn, ref_cnt, ref_id, rcap, rpad, k, d2_out, idx_out, only_rows
  if (lds <= 160 * 1024) {
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_kernel<true>), lds));
    hipLaunchKernelGGL(refine_exact_kernel<true>, SV_REFINE_ARGS);
  } else if (d % SV_WIDE_KC == 0) {
    lds = RefineWideLds<SV_WIDE_KC>::FIXED + (size_t)rpad * 8;   // (the sort keys: <= 64 KiB for a second-tier list)
    if (lds > 160 * 1024) return ctx->fail(SEGVLAD_ERR_LIMIT, "refine: a %d-entry list of %d-d rows exceeds the LDS", rcap, d);
    auto kern = refine_exact_wide_kernel<SV_WIDE_KC, 4>;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, SV_REFINE_ARGS);
  } else {
    lds = (size_t)rpad * 8;
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(refine_exact_kernel<false>), lds));
    hipLaunchKernelGGL(refine_exact_kernel<false>, SV_REFINE_ARGS);
  }
#undef SV_REFINE_ARGS
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}
