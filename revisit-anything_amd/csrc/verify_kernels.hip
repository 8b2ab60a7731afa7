// Spatial verification of matched segments (segvlad_verify_pairs).  No reference counterpart: the reference stops at the vote
// (func_vpr.py:207-224) and studies matched segments of ONE image pair by eye (get_matches_for_single_image_pair,
// func_vpr.py:247-270).  Behind segvlad_match_pairs: do the mutual pairs of slot (b, j) agree on one 2-D similarity transform of
// their centroids?  An exhaustive two-point search, for a batch of query images and up to 64 candidates each, on any
// correspondences (the call never touches the index).
//
//   slot (b, j): the correspondences = the query rows q of image b, ascending, with mutual[q][j] != 0, 0 <= fwd_idx[q][j] < n_r
//                and four finite coordinates; M of them, (p_m, s_m) the m-th; hypothesis h = the pair i < j, lexicographic.
//   per call
//     (memset)            the slots' best keys [n_img][C], 64-bit: 0 = "no eligible hypothesis"
//     vp_score_kernel     1-D grid over a HOST-built task table: a task is (slot, first hypothesis number of a chunk); the table is
//                         sized from qseg_offsets alone -- rows (rows - 1) / 2 bounds the slot's M (M - 1) / 2 --, so a workgroup
//                         whose chunk starts beyond the slot's real number leaves.  The workgroup compacts the slot's
//                         correspondences into LDS in query-row order (ballot + popcount, a wave per 64-row step), every lane takes
//                         one hypothesis at a time and sweeps the M points out of LDS (every lane reads the same address: a
//                         broadcast), keeps (count << 32) | (0xffffffff - h), and the workgroup's maximum goes to the slot's word
//                         by ONE 64-bit atomic maximum: most inliers, then the lowest h, whatever the order of arrival.
//     vp_finish_kernel    one workgroup per query image, a wave per slot: compacts again, decodes the winner, evaluates its inliers
//                         with the SAME device functions (vp_hypothesis, vp_inlier), writes flags, count, pair and model; then
//                         ranks the image's slots by (n_inlier desc, slot asc).
// The arithmetic of the decision (segvlad.h) is plain fp64 multiplications, additions and comparisons in a fixed order, compiled
// with floating-point contraction OFF inside the functions that hold it: a host loop in fp64 reproduces every decision bit for
// bit.  Nothing is read back.  The entry point is at the end of this file.
#include <algorithm>
#include <cmath>

#include "ctx.h"

namespace {

constexpr int VP_MAX_ROWS = 256;   // query rows per image, at most: the search is cubic in M, and a slot's points fill 8 KiB of LDS
constexpr int VP_THREADS = 256;

struct VpTask {    // one workgroup of vp_score_kernel
  int32_t slot;    // b * C + j
  int32_t h0;      // the chunk's first hypothesis number
};

struct VpHyp {     // a hypothesis (i, j): its anchor (p_i, s_i) and the similarity scaled by n = |p_j - p_i|^2
  double pix, piy, six, siy, n, ar, ai, lim;
};

// segvlad.h, "Arithmetic": every operation separately rounded, in this order.  Returns whether the hypothesis is eligible.
__device__ __forceinline__ bool vp_hypothesis(double pix, double piy, double six, double siy, double pjx, double pjy, double sjx,
                                              double sjy, double min2, double max2, double tol2, VpHyp& hy) {
#pragma clang fp contract(off)
  const double dx = pjx - pix, dy = pjy - piy;
  const double ex = sjx - six, ey = sjy - siy;
  const double n = dx * dx + dy * dy, m = ex * ex + ey * ey;
  hy.pix = pix, hy.piy = piy, hy.six = six, hy.siy = siy;
  hy.n = n;
  hy.ar = ex * dx + ey * dy;
  hy.ai = ey * dx - ex * dy;
  hy.lim = (tol2 * n) * n;
  return n > 0.0 && min2 * n <= m && m <= max2 * n;
}

// is correspondence (p_t, s_t) an inlier of the hypothesis?  |a (p_t - p_i) - (s_t - s_i)| < tol, multiplied through by n
__device__ __forceinline__ bool vp_inlier(const VpHyp& hy, double ptx, double pty, double stx, double sty) {
#pragma clang fp contract(off)
  const double px = ptx - hy.pix, py = pty - hy.piy;
  const double sx = stx - hy.six, sy = sty - hy.siy;
  const double ux = (hy.ar * px - hy.ai * py) - hy.n * sx;
  const double uy = (hy.ar * py + hy.ai * px) - hy.n * sy;
  return ux * ux + uy * uy < hy.lim;
}

// informative output: a = (ar / n, ai / n), t = s_i - a p_i
__device__ __forceinline__ void vp_model(const VpHyp& hy, double* out) {
#pragma clang fp contract(off)
  const double are = hy.ar / hy.n, aim = hy.ai / hy.n;
  out[0] = are;
  out[1] = aim;
  out[2] = hy.six - (are * hy.pix - aim * hy.piy);
  out[3] = hy.siy - (are * hy.piy + aim * hy.pix);
}

// hypothesis number -> (i, j), i < j < M: row i starts at S(i) = i (2 M - i - 1) / 2.  A float square root guesses i (every
// operand is an integer below 2^24), integer steps make it exact.  0 <= h < M (M - 1) / 2, 2 <= M <= 256.
__device__ __forceinline__ int vp_row_start(int i, int M) { return i * (2 * M - i - 1) / 2; }
__device__ __forceinline__ void vp_decode(int h, int M, int& i, int& j) {
  const float t = (float)(2 * M - 1);
  int r = (int)((t - sqrtf(t * t - 8.f * (float)h)) * 0.5f);
  r = r < 0 ? 0 : (r > M - 2 ? M - 2 : r);
  while (r > 0 && vp_row_start(r, M) > h) --r;
  while (r < M - 2 && vp_row_start(r + 1, M) <= h) ++r;
  i = r;
  j = h - vp_row_start(r, M) + r + 1;
}

// query row q of slot column j: is it a correspondence, and its two points
__device__ __forceinline__ bool vp_load(const double* __restrict__ q_xy, const double* __restrict__ r_xy, int64_t n_r,
                                        const int64_t* __restrict__ fwd_idx, const uint8_t* __restrict__ mutual, int q, int C, int j,
                                        double& px, double& py, double& sx, double& sy) {
  if (!mutual[(size_t)q * C + j]) return false;
  const int64_t id = fwd_idx[(size_t)q * C + j];
  if (id < 0 || id >= n_r) return false;
  px = q_xy[2 * (size_t)q], py = q_xy[2 * (size_t)q + 1];
  sx = r_xy[2 * (size_t)id], sy = r_xy[2 * (size_t)id + 1];
  return __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(sx) && __builtin_isfinite(sy);
}

__device__ __forceinline__ unsigned long long vp_max64(unsigned long long a, unsigned long long b) { return b > a ? b : a; }

__global__ __launch_bounds__(VP_THREADS) void vp_score_kernel(const double* __restrict__ q_xy, const double* __restrict__ r_xy,
                                                              int64_t n_r, const int32_t* __restrict__ qoff,
                                                              const VpTask* __restrict__ tasks, int C, int chunk,
                                                              const int64_t* __restrict__ fwd_idx, const uint8_t* __restrict__ mutual,
                                                              double min2, double max2, double tol2,
                                                              unsigned long long* __restrict__ best) {
  __shared__ double s_px[VP_MAX_ROWS], s_py[VP_MAX_ROWS], s_sx[VP_MAX_ROWS], s_sy[VP_MAX_ROWS];
  __shared__ int s_cnt[4];
  __shared__ unsigned long long s_key[4];
  const VpTask tk = tasks[blockIdx.x];
  const int b = tk.slot / C, js = tk.slot % C;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int a0 = qoff[b], a1 = qoff[b + 1];   // (a1 - a0 <= 256: a wave per 64-row step)
  const int q = a0 + tid;
  double px = 0.0, py = 0.0, sx = 0.0, sy = 0.0;
  const bool valid = q < a1 && vp_load(q_xy, r_xy, n_r, fwd_idx, mutual, q, C, js, px, py, sx, sy);
  const uint64_t mk = __builtin_amdgcn_ballot_w64(valid);
  if (l == 0) s_cnt[w] = (int)__popcll(mk);
  __syncthreads();
  int base = 0, M = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if (v < w) base += s_cnt[v];
    M += s_cnt[v];
  }
  if (valid) {
    const int pos = base + (int)__popcll(mk & ((1ull << l) - 1ull));
    s_px[pos] = px, s_py[pos] = py, s_sx[pos] = sx, s_sy[pos] = sy;
  }
  __syncthreads();
  const int H = M * (M - 1) / 2;
  if (M < 2 || tk.h0 >= H) return;   // (the same for every thread of the workgroup)
  const int h_end = min(H, tk.h0 + chunk);
  unsigned long long key = 0ull;
  for (int h = tk.h0 + tid; h < h_end; h += VP_THREADS) {
    int i, j;
    vp_decode(h, M, i, j);
    VpHyp hy;
    if (!vp_hypothesis(s_px[i], s_py[i], s_sx[i], s_sy[i], s_px[j], s_py[j], s_sx[j], s_sy[j], min2, max2, tol2, hy)) continue;
    uint32_t cnt = 0;
    for (int t = 0; t < M; ++t) cnt += vp_inlier(hy, s_px[t], s_py[t], s_sx[t], s_sy[t]) ? 1u : 0u;
    key = vp_max64(key, ((unsigned long long)cnt << 32) | (unsigned long long)(0xffffffffu - (uint32_t)h));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = vp_max64(key, __shfl_xor(key, o));
  if (l == 0) s_key[w] = key;
  __syncthreads();
  if (tid == 0) {
    key = vp_max64(vp_max64(s_key[0], s_key[1]), vp_max64(s_key[2], s_key[3]));
    if (key) atomicMax(best + tk.slot, key);
  }
}

// ---- per query image: every slot's winner -- its inlier flags, count, sample and model -- and the order of the slots ----------
__global__ __launch_bounds__(VP_THREADS) void vp_finish_kernel(const double* __restrict__ q_xy, const double* __restrict__ r_xy,
                                                               int64_t n_r, const int32_t* __restrict__ qoff, int C,
                                                               const int64_t* __restrict__ fwd_idx, const uint8_t* __restrict__ mutual,
                                                               double min2, double max2, double tol2,
                                                               const unsigned long long* __restrict__ best,
                                                               int32_t* __restrict__ n_inlier_out, int32_t* __restrict__ pair_out,
                                                               double* __restrict__ model_out, int32_t* __restrict__ order_out,
                                                               uint8_t* __restrict__ inlier_out) {
  __shared__ double s_pt[4][4][VP_MAX_ROWS];   // per wave: px, py, sx, sy of its slot's correspondences
  __shared__ int32_t s_row[4][VP_MAX_ROWS];    // ... and their query rows
  __shared__ int s_n[64];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int a0 = qoff[b], a1 = qoff[b + 1];
  for (int j0 = 0; j0 < C; j0 += 4) {
    const int js = j0 + w;   // (wave-uniform)
    int M = 0;
    if (js < C) {
      for (int qb = a0; qb < a1; qb += 64) {
        const int q = qb + l;
        double px = 0.0, py = 0.0, sx = 0.0, sy = 0.0;
        const bool valid = q < a1 && vp_load(q_xy, r_xy, n_r, fwd_idx, mutual, q, C, js, px, py, sx, sy);
        const uint64_t mk = __builtin_amdgcn_ballot_w64(valid);
        if (valid) {
          const int pos = M + (int)__popcll(mk & ((1ull << l) - 1ull));
          s_pt[w][0][pos] = px, s_pt[w][1][pos] = py, s_pt[w][2][pos] = sx, s_pt[w][3][pos] = sy;
          s_row[w][pos] = q;
        } else if (q < a1 && inlier_out) {
          inlier_out[(size_t)q * C + js] = 0;   // dropped: not a correspondence, not an inlier
        }
        M += (int)__popcll(mk);
      }
    }
    __syncthreads();   // (a wave reads what its other lanes wrote)
    if (js < C) {
      const unsigned long long key = best[(size_t)b * C + js];
      const bool won = M >= 2 && key != 0ull;
      int i = 0, j = 0;
      VpHyp hy = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (won) {
        vp_decode((int)(0xffffffffu - (uint32_t)key), M, i, j);
        (void)vp_hypothesis(s_pt[w][0][i], s_pt[w][1][i], s_pt[w][2][i], s_pt[w][3][i], s_pt[w][0][j], s_pt[w][1][j], s_pt[w][2][j],
                            s_pt[w][3][j], min2, max2, tol2, hy);
      }
      if (inlier_out)
        for (int t = l; t < M; t += 64)
          inlier_out[(size_t)s_row[w][t] * C + js] =
              won && vp_inlier(hy, s_pt[w][0][t], s_pt[w][1][t], s_pt[w][2][t], s_pt[w][3][t]) ? 1 : 0;
      if (l == 0) {
        const size_t o = (size_t)b * C + js;
        const int cnt = won ? (int)(key >> 32) : 0;
        s_n[js] = cnt;
        n_inlier_out[o] = cnt;
        if (pair_out) {
          pair_out[2 * o] = won ? s_row[w][i] : -1;
          pair_out[2 * o + 1] = won ? s_row[w][j] : -1;
        }
        if (model_out) {
          double mo[4] = {NAN, NAN, NAN, NAN};
          if (won) vp_model(hy, mo);
#pragma unroll
          for (int u = 0; u < 4; ++u) model_out[4 * o + u] = mo[u];
        }
      }
    }
    __syncthreads();   // (the next slot of this wave overwrites its points)
  }
  if (order_out && tid < C) {
    const int n = s_n[tid];
    int rank = 0;
    for (int o = 0; o < C; ++o) rank += s_n[o] > n || (s_n[o] == n && o < tid);
    order_out[(size_t)b * C + rank] = tid;
  }
}

}   // namespace

// segvlad_verify_pairs after the argument checks: every bulk pointer on the device, qoff host, n_img > 0
static int verify_pairs(segvlad_ctx* ctx, const double* q_xy, const double* r_xy, int64_t n_r, const int32_t* qoff, int n_img, int C,
                        const int64_t* fwd_idx, const uint8_t* mutual, double tol, double min_scale, double max_scale,
                        int32_t* n_inlier_out, int32_t* pair_out, double* model_out, int32_t* order_out, uint8_t* inlier_out) {
  static_assert(sizeof(VpTask) == 8, "the table is handed over as plain words");
  StageScope sc(ctx, "verify_pairs");
  // hypotheses per task: 256 (one per lane) unless that makes more than 2^16 tasks; the result does not depend on it
  int chunk = VP_THREADS;
  auto n_tasks = [&](int ch) {
    uint64_t t = 0;
    for (int b = 0; b < n_img; ++b) {
      const int64_t rws = qoff[b + 1] - qoff[b];
      t += (uint64_t)C * (uint64_t)((rws * (rws - 1) / 2 + ch - 1) / ch);
    }
    return t;
  };
  while (chunk < VP_MAX_ROWS * (VP_MAX_ROWS - 1) / 2 && n_tasks(chunk) > 65536) chunk *= 2;
  const uint64_t nt = n_tasks(chunk);
  if (nt > 0x7fffffffull) return ctx->fail(SEGVLAD_ERR_LIMIT, "verify_pairs: more than 2^31 - 1 tasks");
  // launch metadata in one copy: qoff [n_img + 1] (padded to 16 bytes), the tasks
  const size_t w_tasks = ((size_t)n_img + 1 + 3) & ~(size_t)3;
  std::vector<uint32_t> meta(w_tasks + (size_t)nt * (sizeof(VpTask) / 4));
  memcpy(meta.data(), qoff, ((size_t)n_img + 1) * 4);
  {
    VpTask* t = reinterpret_cast<VpTask*>(meta.data() + w_tasks);
    for (int b = 0; b < n_img; ++b) {
      const int64_t rws = qoff[b + 1] - qoff[b], H = rws * (rws - 1) / 2;
      for (int j = 0; j < C; ++j)
        for (int64_t h0 = 0; h0 < H; h0 += chunk) *t++ = {b * C + j, (int32_t)h0};
    }
  }
  const void* dmeta;
  SV_TRY(sv_in(ctx, meta.data(), meta.size() * 4, &dmeta));
  const int32_t* dqoff = (const int32_t*)dmeta;
  const VpTask* dtasks = reinterpret_cast<const VpTask*>((const uint32_t*)dmeta + w_tasks);
  const size_t n_slots = (size_t)n_img * C;
  SV_HIP(ctx->s_vp_best.reserve(n_slots * 8));
  unsigned long long* best = ctx->s_vp_best.as<unsigned long long>();
  SV_HIP(hipMemsetAsync(best, 0, n_slots * 8, ctx->stream));
  const double min2 = min_scale * min_scale, max2 = max_scale * max_scale, tol2 = tol * tol;
  int launches = 1;
  if (nt > 0) {
    hipLaunchKernelGGL(vp_score_kernel, dim3((unsigned)nt), dim3(VP_THREADS), 0, ctx->stream, q_xy, r_xy, n_r, dqoff, dtasks, C, chunk,
                       fwd_idx, mutual, min2, max2, tol2, best);
    SV_HIP(hipGetLastError());
    ++launches;
  }
  hipLaunchKernelGGL(vp_finish_kernel, dim3((unsigned)n_img), dim3(VP_THREADS), 0, ctx->stream, q_xy, r_xy, n_r, dqoff, C, fwd_idx,
                     mutual, min2, max2, tol2, best, n_inlier_out, pair_out, model_out, order_out, inlier_out);
  SV_HIP(hipGetLastError());
  sc.count(launches);
  return SEGVLAD_OK;
}

extern "C" int segvlad_verify_pairs(segvlad_ctx* ctx, const double* q_xy, int nq, const double* r_xy, int64_t n_r,
                                    const int32_t* qseg_offsets, int n_img, int C, const int64_t* fwd_idx, const uint8_t* mutual,
                                    double tol, double min_scale, double max_scale, int32_t* n_inlier_out, int32_t* pair_out,
                                    double* model_out, int32_t* order_out, uint8_t* inlier_out) {
  CHECK_CTX();
  if (nq < 0 || n_img < 0 || n_r < 0 || C < 1 || C > 64)
    return ctx->fail(SEGVLAD_ERR_ARG, "verify_pairs: need nq, n_r, n_img >= 0, 1<=C<=64 (C=%d)", C);
  SV_TRY(sv_check_qseg_offsets(ctx, "verify_pairs", qseg_offsets, n_img, nq));
  if (!std::isfinite(tol) || !(tol > 0.0)) return ctx->fail(SEGVLAD_ERR_ARG, "verify_pairs: tol must be finite and > 0");
  if (!(min_scale > 0.0) || !(min_scale <= max_scale) || !std::isfinite(max_scale))
    return ctx->fail(SEGVLAD_ERR_ARG, "verify_pairs: need 0 < min_scale <= max_scale < inf");
  for (int b = 0; b < n_img; ++b)
    if (qseg_offsets[b + 1] - qseg_offsets[b] > VP_MAX_ROWS)
      return ctx->fail(SEGVLAD_ERR_LIMIT, "verify_pairs: query image %d owns %d rows, more than %d (the search is cubic in them)", b,
                       qseg_offsets[b + 1] - qseg_offsets[b], VP_MAX_ROWS);
  if (n_img == 0) return SEGVLAD_OK;   // (then nq == 0 too: nothing to write)
  if (!n_inlier_out || (nq > 0 && (!q_xy || !fwd_idx || !mutual)) || (n_r > 0 && !r_xy))
    return ctx->fail(SEGVLAD_ERR_ARG, "verify_pairs: null pointer");
  const void *dq = nullptr, *dr = nullptr, *dfi = nullptr, *dmu = nullptr;
  void *dn, *dpair = nullptr, *dmodel = nullptr, *dord = nullptr, *dinl = nullptr;
  const size_t n_slots = (size_t)n_img * C;
  SV_TRY(sv_out(ctx, n_inlier_out, n_slots * 4, &dn));
  if (pair_out) SV_TRY(sv_out(ctx, pair_out, n_slots * 2 * 4, &dpair));
  if (model_out) SV_TRY(sv_out(ctx, model_out, n_slots * 4 * 8, &dmodel));
  if (order_out) SV_TRY(sv_out(ctx, order_out, n_slots * 4, &dord));
  if (nq > 0) {   // (no query rows at all: every image is empty, the finish pass alone writes the per-image outputs)
    SV_TRY(sv_in(ctx, q_xy, (size_t)nq * 2 * 8, &dq));
    SV_TRY(sv_in(ctx, r_xy, (size_t)n_r * 2 * 8, &dr));
    SV_TRY(sv_in(ctx, fwd_idx, (size_t)nq * C * 8, &dfi));
    SV_TRY(sv_in(ctx, mutual, (size_t)nq * C, &dmu));
    if (inlier_out) SV_TRY(sv_out(ctx, inlier_out, (size_t)nq * C, &dinl));
  }
  SV_TRY(verify_pairs(ctx, (const double*)dq, (const double*)dr, n_r, qseg_offsets, n_img, C, (const int64_t*)dfi, (const uint8_t*)dmu,
                      tol, min_scale, max_scale, (int32_t*)dn, (int32_t*)dpair, (double*)dmodel, (int32_t*)dord, (uint8_t*)dinl));
  return sv_finish(ctx);
}
