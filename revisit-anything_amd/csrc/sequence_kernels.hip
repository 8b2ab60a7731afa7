// Re-ranking of candidate lists by their consistency along the query sequence (segvlad_sequence_rerank).  No reference counterpart:
// the reference judges every query image alone (func_vpr.py:207-224).  Behind segvlad_vote / segvlad_match_pairs /
// segvlad_verify_pairs: a candidate r of query frame t is believed when the frames around t hold candidates on one line
// r + v (t' - t) through the map -- SeqSLAM's trajectory search, restricted to the candidate lists [T][C] (C <= 64).  The call
// never touches the d-wide rows, the index or the vocabulary.
//
//   per call
//     sq_sort_kernel      one wavefront per frame, one lane per slot: the frame's slots ranked by (empty last, id asc, slot asc) by
//                         counting over shuffles; writes the ids and scores in that order to context scratch (4 + 8 B per slot), an
//                         empty slot as (INT32_MAX, NaN): the lists need no lengths.
//     sq_walk_kernel      a workgroup takes F consecutive frames -- F = 256 / (C n_vel), so that every lane has a pair, 1 when a frame
//                         alone has more pairs than lanes -- and stages the sorted lists of frames t0 - back .. t0 + F - 1 + fwd in LDS
//                         (at most 65 x 64 x 12 B for one frame).  One thread takes one (frame, slot, velocity) pair and walks tau in
//                         ascending order: a binary search for the first id >= p - tol, a scan while id <= p + tol for the largest
//                         score, one fp64 add.  The pairs' (acc, hits) go to LDS OVER the lists (every walk has ended), one thread per
//                         (frame, slot) takes the best velocity (ties: the lowest), writes the three per-slot outputs, and ranks the
//                         frame's slots by counting.
// The arithmetic (segvlad.h) is one fp64 multiplication rounded half to even and fp64 additions in a fixed order, compiled with
// floating-point contraction OFF inside the function that holds it: a host loop reproduces every bit.  No atomics, nothing is read
// back.  The entry point is at the end of this file.
#include <algorithm>
#include <cmath>

#include "ctx.h"

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_MAX_C = 64, SQ_MAX_WIN = 32, SQ_MAX_VEL = 16;
constexpr int SQ_MAX_PASS = SQ_MAX_C * SQ_MAX_VEL / SQ_THREADS;   // pairs per thread when one frame has more pairs than lanes
constexpr size_t SQ_LDS_TARGET = 160 * 1024 / 3;                  // three workgroups per CU

struct SqVel {
  double v[SQ_MAX_VEL];
};

__device__ __forceinline__ bool sq_empty(int32_t id, double sc) { return id < 0 || !__builtin_isfinite(sc); }

// ---- pre-pass: every frame's slots in id order, empty slots last -------------------------------------------------------------
__global__ __launch_bounds__(SQ_THREADS) void sq_sort_kernel(const int32_t* __restrict__ cand, const double* __restrict__ score, int T,
                                                             int C, int32_t* __restrict__ ids, double* __restrict__ scs) {
  const int l = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (SQ_THREADS / 64) + (threadIdx.x >> 6);   // (64-bit: T may end within 3 of INT32_MAX)
  if (t >= T) return;   // (wave-uniform)
  int32_t id = 0x7fffffff;
  double sc = 0.0;
  int e = 1;
  if (l < C) {
    id = cand[(size_t)t * C + l];
    sc = score[(size_t)t * C + l];
    e = sq_empty(id, sc) ? 1 : 0;
  }
  int rank = 0;
  for (int m = 0; m < C; ++m) {
    const int32_t idm = __shfl(id, m);
    const int em = __shfl(e, m);
    const bool first = em != e ? em < e : (e || idm == id ? m < l : idm < id);
    rank += first ? 1 : 0;
  }
  if (l < C) {   // (the keys are distinct: the ranks are a permutation of 0 .. C - 1)
    ids[(size_t)t * C + rank] = e ? 0x7fffffff : id;   // (behind every id in reach of the binary search, whatever the slot held)
    scs[(size_t)t * C + rank] = e ? NAN : sc;
  }
}

// segvlad.h, "Arithmetic": the walk of one (slot, velocity) pair over the staged lists.  s_id / s_sc: the sorted lists of frames
// w0, w0 + 1, ... (C entries each, an empty slot is (INT32_MAX, NaN) and its place behind every other); [lo, hi): the frame's sequence
__device__ __forceinline__ void sq_walk(const int32_t* s_id, const double* s_sc, int C, int w0, int t, int lo, int hi, int back,
                                        int fwd, int32_t r, double own, double vel, int64_t tol, double& acc_out, int& hits_out) {
#pragma clang fp contract(off)
  double acc = 0.0;
  int hits = 0;
  for (int tau = -back; tau <= fwd; ++tau) {
    if (tau == 0) {
      acc = acc + own;
      continue;
    }
    const int64_t tp = (int64_t)t + tau;
    if (tp < lo || tp >= hi) continue;
    const int64_t p = (int64_t)r + (int64_t)__builtin_rint(vel * (double)tau);
    const int64_t pl = p - tol, ph = p + tol;
    const int32_t* fid = s_id + (size_t)(tp - w0) * C;
    const double* fsc = s_sc + (size_t)(tp - w0) * C;
    int a = 0, b = C;   // the first j with id >= pl: the ids alone decide (an empty slot holds INT32_MAX; the scan stops at its NaN)
    while (a < b) {
      const int m = (a + b) >> 1;
      if ((int64_t)fid[m] < pl) a = m + 1;
      else b = m;
    }
    bool hit = false;
    double sup = 0.0;
    for (int j = a; j < C; ++j) {
      const double s = fsc[j];
      if (s != s || (int64_t)fid[j] > ph) break;
      if (!hit || s > sup) sup = s;
      hit = true;
    }
    if (hit) {
      acc = acc + sup;
      ++hits;
    }
  }
  acc_out = acc;
  hits_out = hits;
}

// does slot o come before slot c?  (non-empty first, seq_score descending -- a NaN sum behind every number --, slot ascending)
__device__ __forceinline__ bool sq_before(int ne_o, double s_o, int o, int ne_c, double s_c, int c) {
  if (ne_o != ne_c) return ne_o > ne_c;
  if (ne_c) {
    const bool nan_o = s_o != s_o, nan_c = s_c != s_c;
    if (nan_o != nan_c) return nan_c;
    if (!nan_c && s_o != s_c) return s_o > s_c;
  }
  return o < c;
}

// LDS (dynamic): region A = max(W C, F P) doubles + as many int32 -- the staged lists, then the pairs' results --, then the
// frames' final scores [F C] fp64, their non-empty flags [F C] and the frames' sequence bounds [2 F]
__global__ __launch_bounds__(SQ_THREADS) void sq_walk_kernel(const int32_t* __restrict__ cand, const double* __restrict__ score, int T,
                                                             int C, const int32_t* __restrict__ seq_off, int n_seq, int back, int fwd,
                                                             SqVel vel, int n_vel, int tol, int F, int n_a,
                                                             const int32_t* __restrict__ ids, const double* __restrict__ scs,
                                                             double* __restrict__ seq_score_out, int32_t* __restrict__ n_hit_out,
                                                             int32_t* __restrict__ vel_out, int32_t* __restrict__ order_out) {
  extern __shared__ double sq_lds[];
  double* a_d = sq_lds;
  int32_t* a_i = reinterpret_cast<int32_t*>(a_d + n_a);
  double* s_fin = a_d + n_a + (n_a + 1) / 2;
  int32_t* s_ne = reinterpret_cast<int32_t*>(s_fin + F * C);
  int32_t* s_lo = s_ne + F * C;
  int32_t* s_hi = s_lo + F;
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * F;
  const int nf = min(F, T - t0);   // frames of this workgroup (>= 1)
  const int w0 = max(0, t0 - back), w1 = (int)min((int64_t)T, (int64_t)t0 + nf + fwd);
  for (int i = tid; i < (w1 - w0) * C; i += SQ_THREADS) {
    a_i[i] = ids[(size_t)w0 * C + i];
    a_d[i] = scs[(size_t)w0 * C + i];
  }
  if (tid < nf) {   // the sequence of frame t0 + tid: the last s with seq_off[s] <= t (empty sequences own no frame)
    int lo = 0, hi = T;
    if (seq_off) {
      const int t = t0 + tid;
      int a = 0, b = n_seq;   // the first s with seq_off[s] > t: in 1 .. n_seq
      while (a < b) {
        const int m = (a + b) >> 1;
        if (seq_off[m] <= t) a = m + 1;
        else b = m;
      }
      lo = seq_off[a - 1], hi = seq_off[a];
    }
    s_lo[tid] = lo, s_hi[tid] = hi;
  }
  __syncthreads();
  const int P = C * n_vel, NP = nf * P;
  double racc[SQ_MAX_PASS];
  int rhit[SQ_MAX_PASS];
#pragma unroll
  for (int i = 0; i < SQ_MAX_PASS; ++i) {
    const int pair = i * SQ_THREADS + tid;   // (f, c, u), u fastest
    racc[i] = 0.0, rhit[i] = 0;
    if (pair < NP) {
      const int f = pair / P, rem = pair - f * P, c = rem / n_vel, u = rem - c * n_vel;
      const int t = t0 + f;
      const int32_t r = cand[(size_t)t * C + c];
      const double own = score[(size_t)t * C + c];
      if (!sq_empty(r, own)) sq_walk(a_i, a_d, C, w0, t, s_lo[f], s_hi[f], back, fwd, r, own, vel.v[u], (int64_t)tol, racc[i], rhit[i]);
    }
  }
  __syncthreads();   // (every walk has ended: the results take the lists' place)
#pragma unroll
  for (int i = 0; i < SQ_MAX_PASS; ++i) {
    const int pair = i * SQ_THREADS + tid;
    if (pair < NP) a_d[pair] = racc[i], a_i[pair] = rhit[i];
  }
  __syncthreads();
  const int f = tid / C, c = tid - f * C;   // (F C <= 256: one thread per (frame, slot))
  const bool live = tid < nf * C;
  if (live) {
    const size_t o = (size_t)(t0 + f) * C + c;
    const bool ne = !sq_empty(cand[o], score[o]);
    double best = 0.0;
    int hits = 0, bu = -1;
    if (ne) {
      const int base = tid * n_vel;
      best = a_d[base], hits = a_i[base], bu = 0;
      for (int u = 1; u < n_vel; ++u)
        if (a_d[base + u] > best) best = a_d[base + u], hits = a_i[base + u], bu = u;
    }
    s_fin[tid] = best, s_ne[tid] = ne ? 1 : 0;
    seq_score_out[o] = best;
    if (n_hit_out) n_hit_out[o] = hits;
    if (vel_out) vel_out[o] = bu;
  }
  if (!order_out) return;   // (the same for every thread)
  __syncthreads();
  if (live) {
    const double s = s_fin[tid];
    const int ne = s_ne[tid];
    int rank = 0;
    for (int o = 0; o < C; ++o) rank += sq_before(s_ne[f * C + o], s_fin[f * C + o], o, ne, s, c) ? 1 : 0;
    order_out[(size_t)(t0 + f) * C + rank] = c;
  }
}

// frames per workgroup and the LDS it takes
struct SqShape {
  int F, n_a;
  size_t lds;
};
SqShape sq_shape(int C, int n_vel, int back, int fwd) {
  const int P = C * n_vel;
  auto shape = [&](int F) {
    SqShape s;
    s.F = F;
    s.n_a = std::max((F + back + fwd) * C, F * P);
    s.lds = (size_t)s.n_a * 8 + (size_t)((s.n_a + 1) / 2) * 8 + (size_t)F * C * 12 + (size_t)F * 8;
    return s;
  };
  int F = std::max(1, SQ_THREADS / P);
  while (F > 1 && shape(F).lds > SQ_LDS_TARGET) --F;
  return shape(F);
}

}   // namespace

// segvlad_sequence_rerank after the argument checks: every bulk pointer on the device, seq_off host, T > 0
static int sequence_rerank(segvlad_ctx* ctx, const int32_t* cand, const double* score, int T, int C, const int32_t* seq_off, int n_seq,
                           int back, int fwd, const double* vel, int n_vel, int tol, double* seq_score_out, int32_t* n_hit_out,
                           int32_t* vel_out, int32_t* order_out) {
  static_assert(SQ_MAX_PASS * SQ_THREADS == SQ_MAX_C * SQ_MAX_VEL, "a thread's passes cover the largest frame");
  StageScope sc(ctx, "sequence_rerank");
  const int32_t* dseq = nullptr;   // (one sequence: the kernel needs no table)
  if (n_seq > 1) {
    const void* d;
    SV_TRY(sv_in(ctx, seq_off, ((size_t)n_seq + 1) * 4, &d));
    dseq = (const int32_t*)d;
  }
  const size_t n_slots = (size_t)T * C;
  SV_HIP(ctx->s_sq_id.reserve(n_slots * 4));
  SV_HIP(ctx->s_sq_sc.reserve(n_slots * 8));
  int32_t* ids = ctx->s_sq_id.as<int32_t>();
  double* scs = ctx->s_sq_sc.as<double>();
  hipLaunchKernelGGL(sq_sort_kernel, dim3((unsigned)(((int64_t)T + SQ_THREADS / 64 - 1) / (SQ_THREADS / 64))), dim3(SQ_THREADS), 0, ctx->stream,
                     cand, score, T, C, ids, scs);
  SV_HIP(hipGetLastError());
  SqVel v;
  for (int u = 0; u < SQ_MAX_VEL; ++u) v.v[u] = u < n_vel ? vel[u] : 0.0;
  const SqShape sh = sq_shape(C, n_vel, back, fwd);
  if (sh.lds > 48 * 1024) SV_HIP(sv_max_dyn_lds((const void*)sq_walk_kernel, sh.lds));
  hipLaunchKernelGGL(sq_walk_kernel, dim3((unsigned)(((int64_t)T + sh.F - 1) / sh.F)), dim3(SQ_THREADS), sh.lds, ctx->stream, cand, score, T, C,
                     dseq, n_seq, back, fwd, v, n_vel, tol, sh.F, sh.n_a, (const int32_t*)ids, (const double*)scs, seq_score_out,
                     n_hit_out, vel_out, order_out);
  SV_HIP(hipGetLastError());
  sc.count(2);
  return SEGVLAD_OK;
}

extern "C" int segvlad_sequence_rerank(segvlad_ctx* ctx, const int32_t* cand, const double* score, int T, int C,
                                       const int32_t* seq_offsets, int n_seq, int back, int fwd, const double* vel, int n_vel, int tol,
                                       double* seq_score_out, int32_t* n_hit_out, int32_t* vel_out, int32_t* order_out) {
  CHECK_CTX();
  if (T < 0 || n_seq < 0 || C < 1 || C > SQ_MAX_C)
    return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: need T, n_seq >= 0, 1<=C<=64 (T=%d, n_seq=%d, C=%d)", T, n_seq, C);
  if (back < 0 || back > SQ_MAX_WIN || fwd < 0 || fwd > SQ_MAX_WIN)
    return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: need 0 <= back, fwd <= 32 (back=%d, fwd=%d)", back, fwd);
  if (n_vel < 1 || n_vel > SQ_MAX_VEL || tol < 0 || tol > (1 << 30))
    return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: need 1 <= n_vel <= 16, 0 <= tol <= 2^30 (n_vel=%d, tol=%d)", n_vel, tol);
  if (!seq_offsets || !vel) return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: null seq_offsets or vel");
  if (sv_is_device_ptr(seq_offsets) || sv_is_device_ptr(vel))
    return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: seq_offsets and vel must be host memory");
  if (seq_offsets[0] != 0 || seq_offsets[n_seq] != T)
    return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: seq_offsets must run from 0 to T=%d", T);
  for (int s = 0; s < n_seq; ++s)
    if (seq_offsets[s + 1] < seq_offsets[s]) return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: seq_offsets decrease at %d", s);
  for (int u = 0; u < n_vel; ++u)
    if (!std::isfinite(vel[u]) || std::fabs(vel[u]) > 1048576.0)
      return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: velocity %d is not finite or beyond 2^20 in magnitude", u);
  if (T == 0) return SEGVLAD_OK;   // nothing to write
  if (!cand || !score || !seq_score_out) return ctx->fail(SEGVLAD_ERR_ARG, "sequence_rerank: null pointer");
  const size_t n_slots = (size_t)T * C;
  const void *dc, *ds;
  void *dss, *dnh = nullptr, *dv = nullptr, *dord = nullptr;
  SV_TRY(sv_in(ctx, cand, n_slots * 4, &dc));
  SV_TRY(sv_in(ctx, score, n_slots * 8, &ds));
  SV_TRY(sv_out(ctx, seq_score_out, n_slots * 8, &dss));
  if (n_hit_out) SV_TRY(sv_out(ctx, n_hit_out, n_slots * 4, &dnh));
  if (vel_out) SV_TRY(sv_out(ctx, vel_out, n_slots * 4, &dv));
  if (order_out) SV_TRY(sv_out(ctx, order_out, n_slots * 4, &dord));
  SV_TRY(sequence_rerank(ctx, (const int32_t*)dc, (const double*)ds, T, C, seq_offsets, n_seq, back, fwd, vel, n_vel, tol, (double*)dss,
                         (int32_t*)dnh, (int32_t*)dv, (int32_t*)dord));
  return sv_finish(ctx);
}
