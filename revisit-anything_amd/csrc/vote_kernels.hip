// Similarity-weighted image vote (get_matches "max_seg_topk_wt_borda_Im" + weighted_borda_count,
// func_vpr.py:61-77, 207-224) and the integer variant ("max_seg_topk", func_vpr.py:118-125).
//
// One workgroup per query image.  The reference walks the (rank, segment) entries rank-major and
// adds python floats (fp64) into a dict keyed by reference IMAGE id, then sorts the keys by score,
// descending and stable (ties keep first-appearance order).  To reproduce the fp64 sums bit for bit
// the entries are sorted by (image id, visiting order) in LDS and every distinct image is summed
// sequentially, in visiting order, by one thread.  The weights are formed in fp32 exactly as NumPy
// does: (s - s_min) / (s_max - s_min) with the GLOBAL extrema.
//
// Fast path (images of <= 4096 entries): when every weight of a run is 0 or lies in [2^-17, 1] -- a multiple of 2^-40 --
// every partial sum of <= 4096 of them is exactly representable in fp64, so the run's sum does not depend on the order
// of the additions: the entries are then added with LDS fp64 atomics in parallel (a query image whose matches concentrate
// on one place has runs of hundreds of entries: the sequential walk was 0.3 of the kernel's 0.43 ms on the bench).  A run
// holding any other weight (or a NaN) is poisoned and summed sequentially as before.  Same bits either way.
#include "ctx.h"
#include "knn_dev.h"

struct Run {
  double score;
  uint32_t first;  // visiting order of the first appearance
  int32_t img;
};

// better(a, b): a ranks before b
__device__ __forceinline__ bool better(double sa, uint32_t ta, double sb, uint32_t tb) {
  return sa > sb || (sa == sb && ta < tb);
}

constexpr int VOTE_THREADS = 1024;

// GLOBAL = false: the (image id, visiting order) keys of one query image are sorted in LDS (<= 16384 entries, i.e. 327
// segments at k = 50); images with more entries are skipped.  GLOBAL = true: the workgroup handles query image
// img_list[blockIdx.x] with its keys in a global scratch row (any size: SAM's automatic generator can return many hundreds
// of segments on cluttered images) -- same algorithm, same bits, slower.
template <bool GLOBAL>
__global__ __launch_bounds__(VOTE_THREADS) void vote_kernel(const int64_t* __restrict__ idx, const float* __restrict__ sims,
                                                   const int32_t* __restrict__ img_of_seg, int64_t n_ref_seg,
                                                   const int32_t* __restrict__ qoff, int k,
                                                   const float* __restrict__ minmax, int n_top, int mode,
                                                   Run* __restrict__ runs_scratch, int64_t runs_stride,
                                                   int32_t* __restrict__ pred, double* __restrict__ score, int use_wl,
                                                   int e_lds_cap, const int32_t* __restrict__ img_list,
                                                   uint64_t* __restrict__ gkeys, int64_t gkeys_stride, int fast) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* keys = GLOBAL ? gkeys + (int64_t)blockIdx.x * gkeys_stride : reinterpret_cast<uint64_t*>(smem);
  __shared__ uint32_t s_nruns;
  __shared__ double r_score[VOTE_THREADS];
  __shared__ uint32_t r_tie[VOTE_THREADS];
  __shared__ int r_pos[VOTE_THREADS];
  const int tid = threadIdx.x;
  const int qi = GLOBAL ? img_list[blockIdx.x] : (int)blockIdx.x;
  const int q0 = qoff[qi], Sq = qoff[qi + 1] - q0;
  const int E = Sq * k;
  if (!GLOBAL && E > e_lds_cap) return;   // oversized image: the GLOBAL launch handles it
  int Epad = 2;
  while (Epad < E) Epad <<= 1;
  const float smin = minmax[0], smax = minmax[1];
  const float den = smax - smin;

  // visiting order o = rank * Sq + seg  (rank-major, then segment: func_vpr.py:216 zips the transposed lists)
  for (int o = tid; o < Epad; o += VOTE_THREADS) {
    uint64_t key = ~0ull;
    if (o < E) {
      const int rank = o / Sq, seg = o - rank * Sq;
      const int64_t m = idx[(int64_t)(q0 + seg) * k + rank];
      if (m >= 0 && m < n_ref_seg) key = ((uint64_t)(uint32_t)img_of_seg[m] << 32) | (uint32_t)o;
    }
    keys[o] = key;
  }
  if (tid == 0) s_nruns = 0;
  sv_bitonic<uint64_t, VOTE_THREADS>(keys, Epad, tid);

  // the weights of the sorted entries, in parallel (the fp64 run sums below must stay sequential to reproduce the
  // reference's order of additions; fetching sims[] inside that serial walk was one exposed global load per entry)
  float* wl = reinterpret_cast<float*>(keys + Epad);   // [E]  (LDS mode only; use_wl = 0 in GLOBAL mode)
  if (mode == SEGVLAD_VOTE_WT_BORDA_IM && use_wl) {
    for (int p = tid; p < E; p += VOTE_THREADS) {
      const uint64_t key = keys[p];
      float wgt = 0.f;
      if (key != ~0ull) {
        const uint32_t o = (uint32_t)key;
        const int rank = o / Sq, seg = o - rank * Sq;
        wgt = (sims[(int64_t)(q0 + seg) * k + rank] - smin) / den;
      }
      wl[p] = wgt;
    }
    __syncthreads();
  }
  double* accd = reinterpret_cast<double*>(wl + Epad);   // [Epad] per-run sums, indexed by the run's first position (fast path)
  if (!GLOBAL && fast) {
    for (int p = tid; p < Epad; p += VOTE_THREADS) accd[p] = 0.0;
    __syncthreads();
    for (int p = tid; p < E; p += VOTE_THREADS) {
      const uint64_t key = keys[p];
      if (key == ~0ull) continue;
      const uint32_t img = (uint32_t)(key >> 32);
      int lo = 0, hi = p;   // first position of this image's run
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(keys[mid] >> 32) < img) lo = mid + 1;
        else hi = mid;
      }
      const float wgt = (mode == SEGVLAD_VOTE_WT_BORDA_IM) ? wl[p] : 1.f;
      const bool exact = wgt == 0.f || (wgt >= 7.62939453125e-6f && wgt <= 1.f);   // 2^-17
      unsafeAtomicAdd(&accd[lo], exact ? (double)wgt : (double)NAN);
    }
    __syncthreads();
  }

  Run* runs = runs_scratch + (int64_t)qi * runs_stride;
  for (int p = tid; p < E; p += VOTE_THREADS) {
    const uint64_t key = keys[p];
    if (key == ~0ull) continue;
    const uint32_t img = (uint32_t)(key >> 32);
    if (p > 0 && (uint32_t)(keys[p - 1] >> 32) == img) continue;  // not a run start
    double acc = 0.0;
    uint32_t cnt = 0;
    int e = p;
    const bool summed = !GLOBAL && fast && accd[p] == accd[p];   // not poisoned
    if (summed) {
      acc = accd[p];
      e = E;   // skip the walk
    } else if (!GLOBAL && use_wl && mode == SEGVLAD_VOTE_WT_BORDA_IM) {
      // sequential sum in visiting order, with the run's end found first (binary search): a loop without a data-dependent
      // exit lets the LDS reads run ahead of the dependent fp64 additions (the walk below pays a key read, a compare and
      // a weight read per entry, back to back: ~200 cycles each)
      int lo = p + 1, hi = E;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t km = keys[mid];
        if (km != ~0ull && (uint32_t)(km >> 32) == img) lo = mid + 1;
        else hi = mid;
      }
      const int e_end = lo;
#pragma unroll 8
      for (int q = p; q < e_end; ++q) acc += (double)wl[q];
      cnt = (uint32_t)(e_end - p);
      e = E;
    }
    while (e < E) {
      const uint64_t ke = keys[e];
      if (ke == ~0ull || (uint32_t)(ke >> 32) != img) break;
      if (mode == SEGVLAD_VOTE_WT_BORDA_IM) {
        if (use_wl) {
          acc += (double)wl[e];
        } else {   // > 8192 entries per image: no room for the weight array
          const uint32_t o = (uint32_t)ke;
          const int rank = o / Sq, seg = o - rank * Sq;
          acc += (double)((sims[(int64_t)(q0 + seg) * k + rank] - smin) / den);
        }
      }
      ++cnt;
      ++e;
    }
    Run r;
    r.score = (mode == SEGVLAD_VOTE_WT_BORDA_IM || summed) ? acc : (double)cnt;
    r.first = (mode == SEGVLAD_VOTE_WT_BORDA_IM) ? (uint32_t)key : img;  // COUNT ties: lower image id
    r.img = (int32_t)img;
    runs[atomicAdd(&s_nruns, 1u)] = r;
  }
  __syncthreads();
  const int R = (int)s_nruns;
  __threadfence_block();
  // n_top rounds of arg-best; a taken run gets score = -inf
  for (int round = 0; round < n_top; ++round) {
    double bs = -INFINITY;
    uint32_t bt = ~0u;
    int bp = -1;
    for (int j = tid; j < R; j += VOTE_THREADS) {
      const Run r = runs[j];
      if (r.score == -INFINITY) continue;
      if (bp < 0 || better(r.score, r.first, bs, bt)) {
        bs = r.score;
        bt = r.first;
        bp = j;
      }
    }
    r_score[tid] = bs;
    r_tie[tid] = bt;
    r_pos[tid] = bp;
    __syncthreads();
    for (int o = VOTE_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const int pb = r_pos[tid + o];
        if (pb >= 0 && (r_pos[tid] < 0 || better(r_score[tid + o], r_tie[tid + o], r_score[tid], r_tie[tid]))) {
          r_score[tid] = r_score[tid + o];
          r_tie[tid] = r_tie[tid + o];
          r_pos[tid] = pb;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int bpos = r_pos[0];
      if (bpos >= 0) {
        pred[(int64_t)qi * n_top + round] = runs[bpos].img;
        if (score) score[(int64_t)qi * n_top + round] = runs[bpos].score;
        runs[bpos].score = -INFINITY;
      } else {
        pred[(int64_t)qi * n_top + round] = -1;
        if (score) score[(int64_t)qi * n_top + round] = 0.0;
      }
    }
    __syncthreads();
  }
}

// ---- per-image cap (SEGVLAD_VOTE_PER_IMAGE(m) in segvlad_vote's mode) -------------------------------------------------------
// An entry of row q votes when it is valid (0 <= id < n_ref_seg) and fewer than m valid entries at earlier ranks of the row carry
// its image id.  This pass writes a copy of idx with every other valid entry set to -1; the vote kernels then run on the copy
// unchanged, so a capped vote IS the plain vote over the blanked lists.
//
// One wave per query row, 64 ranks at a time.  Every lane holds the image id of its rank and counts the earlier valid entries
// that carry it: the earlier chunks first (their ids come back from LDS, one per lane, and are compared lane by lane through
// v_readlane -- only the valid lanes are visited), then the lower lanes of its own chunk.  The walk over the earlier chunks ends
// as soon as no lane of the wave can still vote.  LDS keeps the first CAP_LDS_RANKS ids of a row; a deeper row gathers the
// ids behind them again (k > 1024 is beyond every search of the library: correct, not fast).
constexpr int CAP_WAVES = 4;
constexpr int CAP_LDS_RANKS = 1024;

__global__ __launch_bounds__(CAP_WAVES * 64) void vote_cap_kernel(const int64_t* __restrict__ idx, const int32_t* __restrict__ img_of_seg,
                                                                  int64_t n_ref_seg, int nq, int k, int m, int64_t* __restrict__ out) {
  __shared__ int32_t s_img[CAP_WAVES][CAP_LDS_RANKS];
  __shared__ uint8_t s_ok[CAP_WAVES][CAP_LDS_RANKS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * CAP_WAVES + w;
  const bool live = q < nq;   // (a wave without a row keeps the block's barriers company)
  const int64_t* row = idx + q * k;
  for (int c0 = 0; c0 < k; c0 += 64) {
    const int r = c0 + lane;
    int64_t id = -1;
    int32_t g = 0;
    bool ok = false;
    if (live && r < k) {
      id = row[r];
      ok = id >= 0 && id < n_ref_seg;
      if (ok) g = img_of_seg[id];
    }
    if (c0 < CAP_LDS_RANKS) {
      s_img[w][r] = g;
      s_ok[w][r] = ok ? 1 : 0;
    }
    __syncthreads();
    int cnt = 0;
    for (int p0 = 0; p0 < c0; p0 += 64) {
      if (!__any(ok && cnt < m)) break;   // wave-uniform: nobody here can still vote
      int32_t gp = 0;
      bool pok;
      if (p0 < CAP_LDS_RANKS) {
        gp = s_img[w][p0 + lane];
        pok = s_ok[w][p0 + lane] != 0;
      } else {   // (some lane is valid, so the wave has a row; p0 + lane < c0 <= k)
        const int64_t pid = row[p0 + lane];
        pok = pid >= 0 && pid < n_ref_seg;
        if (pok) gp = img_of_seg[pid];
      }
      for (uint64_t pm = __ballot(pok); pm; pm &= pm - 1) cnt += __builtin_amdgcn_readlane(gp, __ffsll((unsigned long long)pm) - 1) == g;
    }
    for (uint64_t om = __ballot(ok); om; om &= om - 1) {
      const int j = __ffsll((unsigned long long)om) - 1;
      cnt += (j < lane) & (__builtin_amdgcn_readlane(g, j) == g);
    }
    if (live && r < k) out[q * k + r] = (ok && cnt >= m) ? -1 : id;
  }
}

int sv_launch_vote_cap(segvlad_ctx* ctx, const int64_t* idx, const int32_t* img_of_seg, int64_t n_ref_seg, int nq, int k, int m,
                       int64_t* out) {
  if (nq <= 0) return SEGVLAD_OK;
  hipLaunchKernelGGL(vote_cap_kernel, dim3((unsigned)(((int64_t)nq + CAP_WAVES - 1) / CAP_WAVES)), dim3(CAP_WAVES * 64), 0, ctx->stream, idx,
                     img_of_seg, n_ref_seg, nq, k, m, out);
  SV_HIP(hipGetLastError());
  return SEGVLAD_OK;
}

// ---- one-to-one vote (SEGVLAD_VOTE_UNIQUE_REF in segvlad_vote's mode) -------------------------------------------------------
// Among the valid entries of one query image that carry the same reference segment id, one wins: the largest sim (a NaN below
// every number, -0 == +0), then the smallest visiting position p = rank * S + segment.  This pass writes a copy of idx with every
// other valid entry set to -1; the cap and the vote kernels then run on the copy unchanged.
//
// Every entry gets one 64-bit key, {sim mapped to an order-preserving uint32, ~p}, so that the 64-bit maximum over the keys of an
// id IS the winner, ties resolved.  A hash table per query image, open addressing with linear probing over T = 2 * entries slots
// (never more than half full, so a probe always ends), holds {id + 1, best key} per slot: the id is claimed with a 64-bit
// compare-and-swap (0 = free), the key raised with a 64-bit max (0 = none: ~p is never 0).  Both commute, so the table's keys do
// not depend on the order of arrival; an entry then keeps its id exactly when its key is its slot's key.  A hot id puts hundreds
// of entries on one slot: contention on one LDS address, not an error.
//
// Images of <= UNIQ_LDS_ENTRIES entries: one workgroup each, the table in LDS (ds_cmpst_rtn_b64 / ds_max_u64), one launch.
// Larger ones: the same scheme on a zeroed global table with agent-scope atomics, insert and resolve as two launches (the kernel
// boundary is the barrier); image b's table starts at slot 2 * (qoff[b] - qoff[first large image]) * k, so no per-image list
// travels to the device and nothing waits for the host.
constexpr int UNIQ_LDS_ENTRIES = 4096;   // 8192 slots x 16 B = 128 KiB of the 160
constexpr int UNIQ_THREADS = 1024;
constexpr int UNIQ_G_THREADS = 256;
constexpr int UNIQ_G_PER_BLOCK = 2048;   // entries a workgroup of the global kernels walks

__device__ __forceinline__ uint32_t uniq_slot(int64_t id, uint32_t T) {
  const uint32_t h = (uint32_t)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 32);
  return (uint32_t)(((uint64_t)h * T) >> 32);
}

// sims == nullptr: every entry the same constant, the smallest p wins
__device__ __forceinline__ uint64_t uniq_key(const float* __restrict__ sims, int64_t at, uint32_t p) {
  uint32_t hi = 1u;
  if (sims) {
    const float s = sims[at];
    uint32_t u = __float_as_uint(s);
    if (s == 0.f) u = 0u;                                  // -0 -> +0
    hi = (s != s) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  }
  return ((uint64_t)hi << 32) | (uint32_t)~p;
}

template <int SCOPE>
__device__ __forceinline__ void uniq_insert(unsigned long long* tid_, unsigned long long* tkey, uint32_t T, int64_t id, uint64_t key) {
  const unsigned long long want = (unsigned long long)id + 1ull;
  uint32_t h = uniq_slot(id, T);
  for (;;) {
    unsigned long long seen = 0ull;
    if (__hip_atomic_compare_exchange_strong(&tid_[h], &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE) || seen == want) break;
    h = h + 1u == T ? 0u : h + 1u;
  }
  __hip_atomic_fetch_max(&tkey[h], (unsigned long long)key, __ATOMIC_RELAXED, SCOPE);
}

// the best key of id (the table holds it: every valid entry was inserted)
__device__ __forceinline__ uint64_t uniq_best(const unsigned long long* tid_, const unsigned long long* tkey, uint32_t T, int64_t id) {
  const unsigned long long want = (unsigned long long)id + 1ull;
  uint32_t h = uniq_slot(id, T);
  while (tid_[h] != want) h = h + 1u == T ? 0u : h + 1u;
  return tkey[h];
}

__global__ __launch_bounds__(UNIQ_THREADS) void vote_unique_lds_kernel(const int64_t* __restrict__ idx, const float* __restrict__ sims,
                                                                       int64_t n_ref_seg, const int32_t* __restrict__ qoff, int k,
                                                                       int64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int q0 = qoff[blockIdx.x], Sq = qoff[blockIdx.x + 1] - q0;
  const int64_t E64 = (int64_t)Sq * k;
  if (E64 <= 0 || E64 > UNIQ_LDS_ENTRIES) return;   // oversized image: the global launches handle it
  const int E = (int)E64;
  const uint32_t T = 2u * (uint32_t)E;
  unsigned long long* t_id = reinterpret_cast<unsigned long long*>(smem);   // [T]
  unsigned long long* t_key = t_id + T;                                      // [T]
  for (uint32_t j = tid; j < 2u * T; j += UNIQ_THREADS) t_id[j] = 0ull;
  __syncthreads();
  for (int o = tid; o < E; o += UNIQ_THREADS) {
    const int rank = o / Sq, seg = o - rank * Sq;
    const int64_t at = (int64_t)(q0 + seg) * k + rank;
    const int64_t id = idx[at];
    if (id >= 0 && id < n_ref_seg) uniq_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(t_id, t_key, T, id, uniq_key(sims, at, (uint32_t)o));
  }
  __syncthreads();
  for (int o = tid; o < E; o += UNIQ_THREADS) {
    const int rank = o / Sq, seg = o - rank * Sq;
    const int64_t at = (int64_t)(q0 + seg) * k + rank;
    const int64_t id = idx[at];
    const bool ok = id >= 0 && id < n_ref_seg;
    out[at] = (ok && uniq_best(t_id, t_key, T, id) != uniq_key(sims, at, (uint32_t)o)) ? -1 : id;
  }
}

// RESOLVE = false: insert.  RESOLVE = true: write the copy.  Grid (images b0 .. b0 + gridDim.x - 1, chunks); an image of that
// range that fits the LDS kernel is skipped.
template <bool RESOLVE>
__global__ __launch_bounds__(UNIQ_G_THREADS) void vote_unique_global_kernel(const int64_t* __restrict__ idx, const float* __restrict__ sims,
                                                                            int64_t n_ref_seg, const int32_t* __restrict__ qoff, int k,
                                                                            int b0, unsigned long long* __restrict__ table,
                                                                            int64_t* __restrict__ out) {
  const int b = b0 + (int)blockIdx.x;
  const int q0 = qoff[b], Sq = qoff[b + 1] - q0;
  const int64_t E = (int64_t)Sq * k;
  if (E <= UNIQ_LDS_ENTRIES) return;
  const uint32_t T = (uint32_t)(2 * E);
  unsigned long long* t_id = table + 4 * (int64_t)(q0 - qoff[b0]) * k;   // 2 slots per entry, 2 words per slot
  unsigned long long* t_key = t_id + T;
  const int64_t o_end = min(E, ((int64_t)blockIdx.y + 1) * UNIQ_G_PER_BLOCK);
  for (int64_t o = (int64_t)blockIdx.y * UNIQ_G_PER_BLOCK + threadIdx.x; o < o_end; o += UNIQ_G_THREADS) {
    const int rank = (int)(o / Sq), seg = (int)(o - (int64_t)rank * Sq);
    const int64_t at = (int64_t)(q0 + seg) * k + rank;
    const int64_t id = idx[at];
    const bool ok = id >= 0 && id < n_ref_seg;
    if (!RESOLVE) {
      if (ok) uniq_insert<__HIP_MEMORY_SCOPE_AGENT>(t_id, t_key, T, id, uniq_key(sims, at, (uint32_t)o));
    } else {
      out[at] = (ok && uniq_best(t_id, t_key, T, id) != uniq_key(sims, at, (uint32_t)o)) ? -1 : id;
    }
  }
}

// out [nq][k] = idx with every valid entry that is not its id's winner within its query image set to -1.  *launches: what was
// enqueued (1 for the images the LDS table holds, 3 -- table fill, insert, resolve -- for the larger ones).
int sv_launch_vote_unique(segvlad_ctx* ctx, const int64_t* idx, const float* sims, int64_t n_ref_seg, const int32_t* qoff_dev,
                          const int32_t* qoff_host, int n_img, int k, int64_t* out, int* launches) {
  *launches = 0;
  int64_t e_small = 0, e_big = 0;
  int b_first = -1, b_last = -1;
  for (int i = 0; i < n_img; ++i) {
    const int s = qoff_host[i + 1] - qoff_host[i];
    if (s < 0) return ctx->fail(SEGVLAD_ERR_ARG, "vote: qseg_offsets must be non-decreasing");
    const int64_t e = (int64_t)s * k;
    if (e > UNIQ_LDS_ENTRIES) {
      if (b_first < 0) b_first = i;
      b_last = i;
      if (e > e_big) e_big = e;
    } else if (e > e_small) {
      e_small = e;
    }
  }
  if (e_big > (1ll << 24)) return ctx->fail(SEGVLAD_ERR_LIMIT, "vote: %lld entries per query image", (long long)e_big);
  if (e_small > 0) {
    const size_t lds = (size_t)e_small * 32;   // 2 slots per entry, 16 B per slot
    if (lds > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(vote_unique_lds_kernel), lds));
    hipLaunchKernelGGL(vote_unique_lds_kernel, dim3(n_img), dim3(UNIQ_THREADS), lds, ctx->stream, idx, sims, n_ref_seg, qoff_dev, k, out);
    SV_HIP(hipGetLastError());
    *launches += 1;
  }
  if (b_first >= 0) {
    const size_t bytes = (size_t)(qoff_host[b_last + 1] - qoff_host[b_first]) * k * 32;
    SV_HIP(ctx->s_vote_tab.reserve(bytes));
    SV_HIP(hipMemsetAsync(ctx->s_vote_tab.p, 0, bytes, ctx->stream));
    const dim3 grid((unsigned)(b_last - b_first + 1), (unsigned)((e_big + UNIQ_G_PER_BLOCK - 1) / UNIQ_G_PER_BLOCK));
    hipLaunchKernelGGL(vote_unique_global_kernel<false>, grid, dim3(UNIQ_G_THREADS), 0, ctx->stream, idx, sims, n_ref_seg, qoff_dev, k,
                       b_first, ctx->s_vote_tab.as<unsigned long long>(), out);
    SV_HIP(hipGetLastError());
    hipLaunchKernelGGL(vote_unique_global_kernel<true>, grid, dim3(UNIQ_G_THREADS), 0, ctx->stream, idx, sims, n_ref_seg, qoff_dev, k,
                       b_first, ctx->s_vote_tab.as<unsigned long long>(), out);
    SV_HIP(hipGetLastError());
    *launches += 3;
  }
  return SEGVLAD_OK;
}

int sv_launch_vote(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg,
                   int64_t n_ref_seg, const int32_t* qoff_dev, const int32_t* qoff_host, int n_img, int k,
                   const float* minmax_dev, int n_top, int mode, int32_t* pred, double* score) {
  if (n_img <= 0) return SEGVLAD_OK;
  constexpr int E_LDS = 16384;   // entries the in-LDS sort holds (8 B keys, 128 KiB)
  int maxS_small = 0, maxS = 0;
  std::vector<int32_t> big;
  for (int i = 0; i < n_img; ++i) {
    const int s = qoff_host[i + 1] - qoff_host[i];
    if (s < 0) return ctx->fail(SEGVLAD_ERR_ARG, "vote: qseg_offsets must be non-decreasing");
    if (s > maxS) maxS = s;
    if ((int64_t)s * k > E_LDS) big.push_back(i);
    else if (s > maxS_small) maxS_small = s;
  }
  const int64_t Emax = (int64_t)maxS * k;
  const int64_t stride = Emax > 0 ? Emax : 1;
  SV_HIP(ctx->s_misc.reserve((size_t)n_img * stride * sizeof(Run)));
  if ((int)big.size() < n_img) {
    const int64_t E = (int64_t)maxS_small * k;
    int Epad = 2;
    while (Epad < E) Epad <<= 1;
    size_t lds = (size_t)Epad * 12;   // sort keys + the entries' weights
    const int use_wl = lds <= 128 * 1024;
    if (!use_wl) lds = (size_t)Epad * 8;
    const int fast = Epad <= 4096 ? 1 : 0;   // + per-run fp64 sums (order-independent when exact, see the header)
    if (fast) lds = (size_t)Epad * 20;
    if (lds > 64 * 1024)
      SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(vote_kernel<false>), (size_t)lds));
    hipLaunchKernelGGL(vote_kernel<false>, dim3(n_img), dim3(VOTE_THREADS), lds, ctx->stream, idx, sims, img_of_seg, n_ref_seg, qoff_dev,
                       k, minmax_dev, n_top, mode, ctx->s_misc.as<Run>(), stride, pred, score, use_wl, E_LDS,
                       (const int32_t*)nullptr, (uint64_t*)nullptr, (int64_t)0, fast);
    SV_HIP(hipGetLastError());
  }
  if (!big.empty()) {   // oversized query images: keys sorted in a global scratch row each
    if (Emax > (1ll << 24)) return ctx->fail(SEGVLAD_ERR_LIMIT, "vote: %d segments x k=%d entries per query image", maxS, k);
    int64_t Epad = 2;
    while (Epad < Emax) Epad <<= 1;
    const size_t nb = big.size();
    SV_HIP(ctx->s_vote_keys.reserve(nb * (size_t)Epad * 8 + nb * 4 + 64));
    uint64_t* gk = ctx->s_vote_keys.as<uint64_t>();
    int32_t* list = reinterpret_cast<int32_t*>(gk + nb * (size_t)Epad);
    SV_HIP(hipMemcpyAsync(list, big.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vote_kernel<true>, dim3((unsigned)nb), dim3(VOTE_THREADS), 0, ctx->stream, idx, sims, img_of_seg, n_ref_seg,
                       qoff_dev, k, minmax_dev, n_top, mode, ctx->s_misc.as<Run>(), stride, pred, score, 0, E_LDS,
                       (const int32_t*)list, gk, Epad, 0);
    SV_HIP(hipGetLastError());
    SV_HIP(hipStreamSynchronize(ctx->stream));   // big[] lives on this frame
  }
  return SEGVLAD_OK;
}
