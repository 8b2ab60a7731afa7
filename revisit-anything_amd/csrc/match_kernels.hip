// Mutual nearest segments between query images and candidate reference images (segvlad_match_pairs).  No reference counterpart:
// the reference studies one query / reference pair on the host (get_matches_for_single_image_pair, func_vpr.py:247-270); this is the
// verification step of deployed place recognition -- after the vote, does query image b really show candidate image c? -- for a
// batch of query images and up to 64 candidates each, on the rows and the image -> row map the index already holds.
//
//   slot (b, j): A = the query rows of image b, B = the index rows of image cand[b][j].
//   per call
//     (memset)            the row minima [nq][C] and the column minima [sum of |B| over the live slots]: all ones = "none"
//     mp_gemm_kernel      1-D grid over a HOST-built task table that holds only live slots: a task is (a group of <= 64 consecutive
//                         query rows of one image -- the groups of sl_gemm_kernel --, one slot).  It walks B in 128-row tiles through
//                         the gathered-row exact fp32 tile (group_tile_dev.h, the one sl_gemm_kernel and refine_group_gemm_kernel
//                         use): v_mfma_f32_32x32x2_f32 in k order, then sv_d2 with the stored norms -- per pair the chain
//                         segvlad_search evaluates, bit for bit.  From the key block in LDS: every query row's running minimum (distance bits, position in B),
//                         kept in LDS across the tiles and written once; every column's minimum (distance bits, query row) goes to the
//                         slot's column array by a 64-bit unsigned atomic minimum -- an image of more than 64 segments spans several
//                         tasks, and a minimum does not depend on the order of arrival.
//     mp_finish_kernel    one workgroup per query image, a wave per slot: the mutual pairs (the column minimum of a row's nearest
//                         column names that row, and d2 < max_d2), their number, their similarities added in fp64 in query-row order
//                         (a wave-uniform walk over the ballot), the per-row outputs; then the image's slots ranked by
//                         (n_mutual desc, score desc, slot asc), slots without rows last.
// The positions of B ascend with the row ids (the map keeps an image's rows ascending), so (distance, position) orders like
// (distance, row id).  A NaN distance gets the key of "none" and is never a minimum.  Nothing is read back: the grid and the scratch
// sizes come from cand and the host mirror of the map's offsets (sv_sl_map_host).  The entry point is at the end of this file.
#include <algorithm>

#include "ctx.h"
#include "group_tile_dev.h"
#include "knn_dev.h"

namespace {

constexpr int MP_GMAX = 64;   // query rows per group, at most (SL_GMAX)
constexpr uint32_t MP_NONE = 0xffffffffu;

__device__ __forceinline__ uint32_t mp_f2key(float f) {   // (f2key_; a NaN is nobody's nearest)
  return f != f ? MP_NONE : f2key_(f);
}
__device__ __forceinline__ uint64_t mp_min64(uint64_t a, uint64_t b) { return b < a ? b : a; }

struct MpTask {    // one workgroup of mp_gemm_kernel
  int32_t q0, nrows;        // the group's query rows
  int32_t slot;             // b * C + j
  uint32_t roff, U;         // B = sl_img_rows[roff .. roff + U)
  uint32_t colbase;         // the slot's first word in the column minima
  uint32_t pad[2];
};
struct MpSlot {    // one entry per (b, j) for mp_finish_kernel; U == 0: padding, or an image without rows
  uint32_t roff, U, colbase, pad;
};

template <int MT>
__global__ __launch_bounds__(256) void mp_gemm_kernel(const float* __restrict__ Q, const float* __restrict__ R, int d,
                                                      const float* __restrict__ qn, const float* __restrict__ rn,
                                                      const MpTask* __restrict__ tasks, int C, const uint32_t* __restrict__ rows,
                                                      uint64_t* __restrict__ rowmin, uint64_t* __restrict__ colmin) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [staging image] [dk: 32 MT x 128 distance keys]
  float* tile = reinterpret_cast<float*>(smem);
  uint32_t* dk = reinterpret_cast<uint32_t*>(smem + sv_group_tile_bytes(MT));
  __shared__ uint32_t ids[128];
  __shared__ uint64_t s_rmin[32 * MT];
  const MpTask tk = tasks[blockIdx.x];
  const int q0 = tk.q0, nrows = tk.nrows;
  const int q_end = q0 + nrows;
  const int U = (int)tk.U;
  const uint32_t* brows = rows + tk.roff;
  uint64_t* cmin = colmin + tk.colbase;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 31, kk = l >> 5;
  // initialised by wave 0, made visible to the row's owner by the barrier at the top of the first tile (every task has one: U > 0);
  // from there on row r is only touched by wave r & 3, so the tiles' updates need no barrier of their own
  if (tid < 32 * MT) s_rmin[tid] = ~0ull;
  const SvGroupTileQ<MT> qrows = sv_group_tile_query_rows<MT>(Q, d, q0, q_end);   // (the same for every tile)
  const int ntile = (U + 127) >> 7;
  for (int t = 0; t < ntile; ++t) {
    const int c0 = t * 128;
    if (tid < 128) ids[tid] = c0 + tid < U ? brows[c0 + tid] : 0u;   // (columns beyond U: row 0, computed and never used)
    __syncthreads();
    f32x16 acc[MT];
    sv_group_tile_dots<MT>(tile, ids, qrows, R, d, acc);
    {
      const int col = 32 * w + i;
      const float r2 = rn[ids[col]];
#pragma unroll
      for (int u = 0; u < MT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lr2 = 32 * u + sv_frag_row(r, kk);
          if (q0 + lr2 < q_end) dk[lr2 * 128 + col] = mp_f2key(sv_d2_screen(qn[q0 + lr2], r2, acc[u][r]));
        }
    }
    __syncthreads();
    // row minima: a wave per row, two columns per lane, (distance bits, position in B)
    for (int r = w; r < nrows; r += 4) {
      uint64_t best = ~0ull;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = l + 64 * h;
        const uint32_t key = dk[r * 128 + col];
        if (c0 + col < U && key != MP_NONE) best = mp_min64(best, ((uint64_t)key << 32) | (uint32_t)(c0 + col));
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = mp_min64(best, (uint64_t)__shfl_xor((unsigned long long)best, o));
      if (l == 0 && best < s_rmin[r]) s_rmin[r] = best;
    }
    // column minima: a thread per column, (distance bits, query row); the groups of an image meet in the atomic minimum
    if (tid < 128 && c0 + tid < U) {
      uint64_t best = ~0ull;
      for (int r = 0; r < nrows; ++r) {
        const uint32_t key = dk[r * 128 + tid];
        if (key != MP_NONE) best = mp_min64(best, ((uint64_t)key << 32) | (uint32_t)(q0 + r));
      }
      if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(cmin + c0 + tid), (unsigned long long)best);
    }
    __syncthreads();
  }
  if (tid < nrows) rowmin[(size_t)(q0 + tid) * C + (tk.slot % C)] = s_rmin[tid];
}

// ---- per query image: the mutual pairs of every slot, their number and score, and the order of the slots --------------------
__global__ __launch_bounds__(256) void mp_finish_kernel(const int32_t* __restrict__ qoff, const MpSlot* __restrict__ slots, int C,
                                                        const uint32_t* __restrict__ rows, const uint64_t* __restrict__ rowmin,
                                                        const uint64_t* __restrict__ colmin, float max_d2,
                                                        int32_t* __restrict__ n_mutual_out, double* __restrict__ score_out,
                                                        int32_t* __restrict__ order_out, int64_t* __restrict__ fwd_idx_out,
                                                        float* __restrict__ fwd_d2_out, uint8_t* __restrict__ mutual_out) {
  __shared__ int s_n[64];
  __shared__ double s_sc[64];
  __shared__ int s_live[64];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int a0 = qoff[b], a1 = qoff[b + 1];
  for (int j = w; j < C; j += 4) {
    const MpSlot sl = slots[(size_t)b * C + j];
    int cnt = 0;
    double sc = 0.0;
    for (int qb = a0; qb < a1; qb += 64) {
      const int q = qb + l;
      bool m = false;
      float dd = INFINITY;
      int64_t id = -1;
      if (q < a1) {
        const uint64_t key = sl.U ? rowmin[(size_t)q * C + j] : ~0ull;
        if (key != ~0ull) {
          const uint32_t p = (uint32_t)key;
          dd = key2f_((uint32_t)(key >> 32));
          id = (int64_t)rows[sl.roff + p];
          m = (uint32_t)colmin[sl.colbase + p] == (uint32_t)q && dd < max_d2;
        }
        if (fwd_idx_out) fwd_idx_out[(size_t)q * C + j] = id;
        if (fwd_d2_out) fwd_d2_out[(size_t)q * C + j] = dd;
        if (mutual_out) mutual_out[(size_t)q * C + j] = m ? 1 : 0;
      }
      uint64_t mk = __builtin_amdgcn_ballot_w64(m);
      cnt += (int)__popcll(mk);
      const double term = (double)(2.0f - dd);   // fp32 subtraction (sims_kernel), fp64 additions in query-row order
      while (mk) {
        const int src = __builtin_ctzll(mk);
        mk &= mk - 1;
        sc += __shfl(term, src);
      }
    }
    if (l == 0) {
      s_n[j] = cnt;
      s_sc[j] = sc;
      s_live[j] = sl.U != 0u;
      n_mutual_out[(size_t)b * C + j] = cnt;
      score_out[(size_t)b * C + j] = sc;
    }
  }
  __syncthreads();
  if (order_out && tid < C) {
    const int n = s_n[tid], live = s_live[tid];
    const double sc = s_sc[tid];
    int rank = 0;
    for (int o = 0; o < C; ++o) {
      if (o == tid) continue;
      bool before;
      if (s_live[o] != live) before = s_live[o] != 0;
      else if (!live) before = o < tid;
      else if (s_n[o] != n) before = s_n[o] > n;
      else if (s_sc[o] != sc) before = s_sc[o] > sc;
      else before = o < tid;
      rank += before;
    }
    order_out[(size_t)b * C + rank] = tid;
  }
}

}   // namespace

// segvlad_match_pairs after the argument checks: Q on the device, 16-byte aligned, qn its squared norms; qoff / cand host; outputs on
// the device (n_mutual_out and score_out always, the others may be null); the index may be empty
static int match_pairs(segvlad_ctx* ctx, const float* Q, int nq, const float* qn, const int32_t* qoff, int n_img, const int32_t* cand,
                       int C, float max_d2, int32_t* n_mutual_out, double* score_out, int32_t* order_out, int64_t* fwd_idx_out,
                       float* fwd_d2_out, uint8_t* mutual_out) {
  static_assert(sizeof(MpTask) == 32 && sizeof(MpSlot) == 16, "tables are handed over as plain words");
  const int d = ctx->db_d;
  SV_TRY(sv_sl_map_host(ctx));
  StageScope sc(ctx, "match_pairs");
  const int nimg_ref = ctx->db_img_max + 1;
  const uint32_t* off = ctx->sl_off_host.data();
  // the slots (one column array per live slot, duplicates included: every slot is evaluated on its own) and the tasks
  std::vector<MpSlot> slots((size_t)n_img * C);
  std::vector<MpTask> tasks;
  uint64_t ncol = 0;
  int gmax = 0;
  for (int b = 0; b < n_img; ++b) {
    const int rws = qoff[b + 1] - qoff[b];
    const int ng = (rws + MP_GMAX - 1) / MP_GMAX;
    for (int j = 0; j < C; ++j) {
      const int id = cand[(size_t)b * C + j];
      MpSlot s = {0u, 0u, 0u, 0u};
      if (id >= 0 && id < nimg_ref && off[id + 1] > off[id]) {
        s.roff = off[id];
        s.U = off[id + 1] - off[id];
        if (ncol + s.U > 0x7fffffffull) return ctx->fail(SEGVLAD_ERR_LIMIT, "match_pairs: the candidates' rows exceed 2^31 - 1 in all");
        s.colbase = (uint32_t)ncol;
        ncol += s.U;
        for (int g = 0; g < ng; ++g) {   // an image's rows in ceil(rows / 64) near-equal runs (segvlad_search_shortlist's groups)
          const int a0 = qoff[b] + (int)((int64_t)rws * g / ng), a1 = qoff[b] + (int)((int64_t)rws * (g + 1) / ng);
          tasks.push_back({a0, a1 - a0, b * C + j, s.roff, s.U, s.colbase, {0u, 0u}});
          gmax = std::max(gmax, a1 - a0);
        }
      }
      slots[(size_t)b * C + j] = s;
    }
  }
  const size_t n_row_words = (size_t)nq * C;
  SV_HIP(ctx->s_mp_min.reserve((n_row_words + (size_t)ncol) * 8));
  uint64_t* rowmin = ctx->s_mp_min.as<uint64_t>();
  uint64_t* colmin = rowmin + n_row_words;
  if (n_row_words + ncol > 0) SV_HIP(hipMemsetAsync(rowmin, 0xff, (n_row_words + (size_t)ncol) * 8, ctx->stream));
  // launch metadata in one copy: qoff [n_img + 1] (padded to 16 bytes), the slots, the tasks
  const size_t w_slots = ((size_t)n_img + 1 + 3) & ~(size_t)3;
  const size_t w_tasks = w_slots + slots.size() * (sizeof(MpSlot) / 4);
  std::vector<uint32_t> meta(w_tasks + tasks.size() * (sizeof(MpTask) / 4));
  memcpy(meta.data(), qoff, ((size_t)n_img + 1) * 4);
  memcpy(meta.data() + w_slots, slots.data(), slots.size() * sizeof(MpSlot));
  if (!tasks.empty()) memcpy(meta.data() + w_tasks, tasks.data(), tasks.size() * sizeof(MpTask));
  const void* dmeta;
  SV_TRY(sv_in(ctx, meta.data(), meta.size() * 4, &dmeta));
  const int32_t* dqoff = (const int32_t*)dmeta;
  const MpSlot* dslots = reinterpret_cast<const MpSlot*>((const uint32_t*)dmeta + w_slots);
  const MpTask* dtasks = reinterpret_cast<const MpTask*>((const uint32_t*)dmeta + w_tasks);
  int launches = 1;
  if (!tasks.empty()) {
    const int mt = gmax > 32 ? 2 : 1;
    const size_t glds = sv_group_tile_bytes(mt) + (size_t)32 * mt * 128 * 4;
    auto gk = mt == 2 ? mp_gemm_kernel<2> : mp_gemm_kernel<1>;
    SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(gk), glds));
    hipLaunchKernelGGL(gk, dim3((unsigned)tasks.size()), dim3(256), glds, ctx->stream, Q, ctx->db_rows.as<float>(), d, qn,
                       ctx->db_norms.as<float>(), dtasks, C, ctx->sl_img_rows.as<uint32_t>(), rowmin, colmin);
    SV_HIP(hipGetLastError());
    ++launches;
  }
  hipLaunchKernelGGL(mp_finish_kernel, dim3((unsigned)n_img), dim3(256), 0, ctx->stream, dqoff, dslots, C,
                     ctx->sl_img_rows.as<uint32_t>(), rowmin, colmin, max_d2, n_mutual_out, score_out, order_out, fwd_idx_out,
                     fwd_d2_out, mutual_out);
  SV_HIP(hipGetLastError());
  sc.count(launches);
  return SEGVLAD_OK;
}

extern "C" int segvlad_match_pairs(segvlad_ctx* ctx, const float* Q, int nq, const int32_t* qseg_offsets, int n_img, const int32_t* cand,
                                   int C, float max_d2, int32_t* n_mutual_out, double* score_out, int32_t* order_out,
                                   int64_t* fwd_idx_out, float* fwd_d2_out, uint8_t* mutual_out) {
  CHECK_CTX();
  if (nq < 0 || n_img < 0 || C < 1 || C > 64)
    return ctx->fail(SEGVLAD_ERR_ARG, "match_pairs: need nq, n_img >= 0, 1<=C<=64 (C=%d)", C);
  SV_TRY(sv_check_qseg_offsets(ctx, "match_pairs", qseg_offsets, n_img, nq));
  if (n_img > 0 && !cand) return ctx->fail(SEGVLAD_ERR_ARG, "match_pairs: null cand");
  if (cand && sv_is_device_ptr(cand)) return ctx->fail(SEGVLAD_ERR_ARG, "match_pairs: cand must be host memory");
  SV_TRY(sv_check_img_index(ctx, "match_pairs"));
  if (n_img == 0) return SEGVLAD_OK;   // (then nq == 0 too: nothing to write)
  if ((nq > 0 && !Q) || !n_mutual_out || !score_out) return ctx->fail(SEGVLAD_ERR_ARG, "match_pairs: null pointer");
  const int d = ctx->db_d;
  if (nq > 0 && d % 32 != 0) return ctx->fail(SEGVLAD_ERR_LIMIT, "match_pairs: d=%d (the exact GEMM takes d %% 32 == 0)", d);
  if (ctx->db_n > 0x7fffffffll) return ctx->fail(SEGVLAD_ERR_LIMIT, "match_pairs: more than 2^31 - 1 rows");
  const void* dq = nullptr;
  const float* q = nullptr;
  void *dn, *ds, *dord = nullptr, *dfi = nullptr, *dfd = nullptr, *dmu = nullptr;
  SV_TRY(sv_out(ctx, n_mutual_out, (size_t)n_img * C * 4, &dn));
  SV_TRY(sv_out(ctx, score_out, (size_t)n_img * C * 8, &ds));
  if (order_out) SV_TRY(sv_out(ctx, order_out, (size_t)n_img * C * 4, &dord));
  if (nq > 0) {   // (no query rows at all: every image is empty, the finish pass alone writes the zeros and the order)
    SV_TRY(sv_in(ctx, Q, (size_t)nq * d * 4, &dq));
    SV_TRY(sv_aligned_queries(ctx, (const float*)dq, nq, &q));
    if (fwd_idx_out) SV_TRY(sv_out(ctx, fwd_idx_out, (size_t)nq * C * 8, &dfi));
    if (fwd_d2_out) SV_TRY(sv_out(ctx, fwd_d2_out, (size_t)nq * C * 4, &dfd));
    if (mutual_out) SV_TRY(sv_out(ctx, mutual_out, (size_t)nq * C, &dmu));
    SV_HIP(ctx->s_qnorm.reserve((size_t)nq * 4));
    SV_TRY(sv_launch_row_sumsq(ctx, q, nq, d, ctx->s_qnorm.as<float>()));
  }
  SV_TRY(match_pairs(ctx, q, nq, ctx->s_qnorm.as<float>(), qseg_offsets, n_img, cand, C, max_d2, (int32_t*)dn, (double*)ds,
                     (int32_t*)dord, (int64_t*)dfi, (float*)dfd, (uint8_t*)dmu));
  return sv_finish(ctx);
}
