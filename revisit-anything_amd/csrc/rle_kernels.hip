// Run-length masks: SAM's uncompressed RLE (mask_to_rle_pytorch / rle_to_mask, sam/segment_anything/utils/amg.py:107-149) as a second
// way into the mask branch -- segvlad_incidence_rle writes what segvlad_incidence_centroids writes for the decoded masks, byte for
// byte, and segvlad_rle_decode inflates a batch to dense bytes on the device.
//
// A batch: counts uint32 [n_runs], the runs of all masks one after the other; run_offsets int64 [S + 1]; mask s owns
// counts[run_offsets[s] .. run_offsets[s + 1]).  A mask is column-major (pixel p = col * Hm + row), its runs alternate zeros / ones
// and start with zeros.
//
// Both kernels: one workgroup per mask (decode: per mask and window), 256 threads.
//   phase 1  the runs are walked in chunks of RLE_CHUNK: thread i takes the (zeros, ones) pair 2i, 2i + 1, a workgroup prefix sum of
//            the pair lengths gives every ones-run its first pixel; the running start is carried from chunk to chunk in 64 bits and
//            saturates at Hm Wm + 1, so that no sum of 32-bit counts can wrap back into range;
//   phase 2  every ones-run, clipped to [0, Hm Wm), sets its bits in a column-major LDS bitmap ([column][ceil(Hm / 32)] words) --
//            split at column ends, full words as plain stores (a full word belongs to one run), partial words with atomicOr; a run
//            over more than two columns is queued and set by the whole workgroup, a column per thread.  The incidence kernel adds
//            the exact integer sums (count, sum of rows, sum of columns) of every column piece as arithmetic series;
//   phase 3  incidence: lane = token, the bits its cell samples, ballot (incidence_fused_kernel's phase 2 on the transposed
//            bitmap); decode: row-major stores of 0 / 1 bytes, the column index fastest.
// A count only ever becomes a position of the LDS bitmap, clamped to Hm Wm first; every global store goes to an address that
// (mask, word) or (mask, row, column) fixes.  A mask whose runs do not sum to Hm Wm is clipped there, the pixels its runs do not
// reach are zero, and it adds one to *n_bad.
#include <algorithm>

#include "ctx.h"
#include "incidence_dev.h"

constexpr int RLE_CHUNK = 512;   // runs per step of the walk (engine.RLE_CHUNK_RUNS; tests/test_rle_host.py compares the two)
constexpr int RLE_THREADS = RLE_CHUNK / 2;
constexpr size_t RLE_LDS_BOUND = 150 * 1024;   // the bitmap; the workgroup's static block (RleShared) comes on top: < 160 KiB
static_assert(RLE_THREADS == 256, "the wave bookkeeping below is written for four waves");

typedef unsigned long long u64;

struct RleShared {
  u64 wsum[4];              // the waves' sums of a chunk
  u64 la[RLE_THREADS];      // long runs of the chunk, clipped: pixels [la, lb)
  u64 lb[RLE_THREADS];
  u64 red[3][4];            // the waves' (sum of rows, sum of columns, count)
  uint32_t n_long, pad[3];
};
static_assert(sizeof(RleShared) % 16 == 0, "the dynamic block behind it stays 16-byte aligned");
static_assert(RLE_LDS_BOUND + sizeof(RleShared) <= 160 * 1024, "bitmap + static block must fit the CU's LDS");

// columns [c0, c0 + nc) x row words [w0, w0 + nw) of a mask: what one workgroup holds as bits[(col - c0) * wst + (word - w0)]
struct RleWindow {
  int c0, nc, w0, nw;
};

__device__ __forceinline__ void rle_split(u64 p, uint32_t Hm, bool small, uint32_t& col, uint32_t& row) {
  if (small) {   // Hm Wm < 2^32: 32-bit division
    const uint32_t q = (uint32_t)p / Hm;
    col = q;
    row = (uint32_t)p - q * Hm;
  } else {
    const u64 q = p / Hm;
    col = (uint32_t)q;
    row = (uint32_t)(p - q * Hm);
  }
}

// rows r_lo .. r_hi (inclusive) of column col, which lies inside the window's columns
template <bool SUMS>
__device__ __forceinline__ void rle_set_column(uint32_t* bits, int wst, const RleWindow& win, uint32_t col, uint32_t r_lo, uint32_t r_hi,
                                               u64& cnt, u64& sr, u64& sc) {
  if (SUMS) {
    const u64 n = (u64)(r_hi - r_lo) + 1;
    cnt += n;
    sr += ((u64)r_lo + (u64)r_hi) * n / 2;   // r_lo + ... + r_hi: (first + last) n is even
    sc += (u64)col * n;
  }
  const int wl = (int)(r_lo >> 5), wh = (int)(r_hi >> 5);
  const int wa = max(wl, win.w0), wb = min(wh, win.w0 + win.nw - 1);
  uint32_t* colw = bits + ((int)col - win.c0) * wst;
  for (int w = wa; w <= wb; ++w) {
    const uint32_t lo = (w == wl) ? (r_lo & 31u) : 0u, hi = (w == wh) ? (r_hi & 31u) : 31u;
    const uint32_t m = (hi == 31u ? 0xffffffffu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
    if (m == 0xffffffffu) colw[w - win.w0] = m;
    else atomicOr(&colw[w - win.w0], m);
  }
}

// the columns first .. last (inside the window) of the run of pixels [a, b): thread `lane_id` of `n_lanes` takes every n_lanes-th
template <bool SUMS>
__device__ __forceinline__ void rle_set_run(uint32_t* bits, int wst, const RleWindow& win, uint32_t Hm, uint32_t ca, uint32_t ra, uint32_t ce,
                                            uint32_t re, uint32_t first, uint32_t last, uint32_t lane_id, uint32_t n_lanes, u64& cnt,
                                            u64& sr, u64& sc) {
  for (u64 c = (u64)first + lane_id; c <= (u64)last; c += n_lanes)
    rle_set_column<SUMS>(bits, wst, win, (uint32_t)c, c == ca ? ra : 0u, c == ce ? re : Hm - 1u, cnt, sr, sc);
}

// Phases 1 and 2 for the runs counts[lo, hi) of one mask into the (zeroed) bitmap of `win`.  walk_all: every run is read and the
// return value says whether they sum to exactly P = Hm Wm; otherwise the walk ends behind the window's last column.  Ends with a
// workgroup barrier: the bitmap is complete for every thread.
template <bool SUMS>
__device__ __forceinline__ bool rle_build(const uint32_t* __restrict__ counts, int64_t lo, int64_t hi, uint32_t Hm, u64 P, const RleWindow win,
                                          bool walk_all, uint32_t* bits, int wst, RleShared& sh, u64& cnt, u64& sr, u64& sc) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool small = P <= 0xffffffffull;
  const uint32_t c_end = (uint32_t)(win.c0 + win.nc);              // first column behind the window
  const u64 win_end = min(P, (u64)c_end * Hm);
  u64 carry = 0;                                                    // pixels before this chunk, saturated at P + 1 (uniform)
  for (int64_t base = lo; base < hi; base += RLE_CHUNK) {
    if (tid == 0) sh.n_long = 0;
    const int64_t j = base + 2 * tid;
    const uint32_t z = j < hi ? counts[j] : 0u, o = j + 1 < hi ? counts[j + 1] : 0u;
    const u64 v = (u64)z + (u64)o;
    u64 incl = v;
    for (int d = 1; d < 64; d <<= 1) {   // inclusive scan of the wave
      const u64 u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    if (lane == 63) sh.wsum[wv] = incl;
    __syncthreads();
    u64 pre = carry;
    for (int k = 0; k < wv; ++k) pre += sh.wsum[k];
    const u64 tot = sh.wsum[0] + sh.wsum[1] + sh.wsum[2] + sh.wsum[3];   // < 2^42
    const u64 a = min(pre + (incl - v) + z, P), b = min(pre + incl, P);  // the ones-run, clipped (pre <= P + 1: no wrap)
    if (b > a) {
      uint32_t ca, ra, ce, re;
      rle_split(a, Hm, small, ca, ra);
      rle_split(b - 1, Hm, small, ce, re);
      const uint32_t first = max(ca, (uint32_t)win.c0), last = min(ce, c_end - 1u);
      if (first <= last) {
        if (last - first >= 2u) {
          const uint32_t k = atomicAdd(&sh.n_long, 1u);
          sh.la[k] = a;
          sh.lb[k] = b;
        } else {
          rle_set_run<SUMS>(bits, wst, win, Hm, ca, ra, ce, re, first, last, 0u, 1u, cnt, sr, sc);
        }
      }
    }
    __syncthreads();
    const uint32_t nl = sh.n_long;
    for (uint32_t k = 0; k < nl; ++k) {
      uint32_t ca, ra, ce, re;
      rle_split(sh.la[k], Hm, small, ca, ra);
      rle_split(sh.lb[k] - 1, Hm, small, ce, re);
      rle_set_run<SUMS>(bits, wst, win, Hm, ca, ra, ce, re, max(ca, (uint32_t)win.c0), min(ce, c_end - 1u), (uint32_t)tid, RLE_THREADS, cnt, sr,
                        sc);
    }
    carry = min(carry + tot, P + 1);
    __syncthreads();
    if (carry > P || (!walk_all && carry >= win_end)) break;
  }
  return carry == P;
}

extern "C" {

__global__ __launch_bounds__(RLE_THREADS) void incidence_rle_kernel(const uint32_t* __restrict__ counts, const int64_t* __restrict__ run_offsets,
                                                                   int S, int Hm, int Wm, int H, int W, int patch, int dh, int dw, float sh_,
                                                                   float sw_, int wst, uint64_t* __restrict__ inc, int nw,
                                                                   double* __restrict__ cent, uint32_t* __restrict__ n_bad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* bits = reinterpret_cast<uint32_t*>(smem);   // [Wm][wst], the first ceil(Hm / 32) words of a column used
  __shared__ RleShared sh;
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < Wm * wst; j += RLE_THREADS) bits[j] = 0;
  __syncthreads();
  const int64_t nr = max(run_offsets[S], (int64_t)0);
  const int64_t lo = min(max(run_offsets[s], (int64_t)0), nr), hi = min(max(run_offsets[s + 1], lo), nr);
  const RleWindow win = {0, Wm, 0, (Hm + 31) >> 5};
  u64 sr = 0, sc = 0, cnt = 0;
  const bool ok = rle_build<true>(counts, lo, hi, (uint32_t)Hm, (u64)Hm * (u64)Wm, win, true, bits, wst, sh, cnt, sr, sc);
  for (int o = 32; o > 0; o >>= 1) {   // exact integer sums, reduced and divided as incidence_fused_kernel does
    sr += __shfl_xor(sr, o);
    sc += __shfl_xor(sc, o);
    cnt += __shfl_xor(cnt, o);
  }
  if ((tid & 63) == 0) {
    sh.red[0][tid >> 6] = sr;
    sh.red[1][tid >> 6] = sc;
    sh.red[2][tid >> 6] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    if (cent) {
      const double c = (double)(sh.red[2][0] + sh.red[2][1] + sh.red[2][2] + sh.red[2][3]);
      cent[2 * (size_t)s + 0] = (double)(sh.red[1][0] + sh.red[1][1] + sh.red[1][2] + sh.red[1][3]) / c;
      cent[2 * (size_t)s + 1] = (double)(sh.red[0][0] + sh.red[0][1] + sh.red[0][2] + sh.red[0][3]) / c;
    }
    if (!ok && n_bad) atomicAdd(n_bad, 1u);
  }
  const int N = dh * dw;
  const bool ranges = (sh_ <= 1.0f) && (sw_ <= 1.0f);   // up-sampling: a cell samples contiguous source rows / columns
  for (int t0 = 0; t0 < nw * 64; t0 += RLE_THREADS) {
    const int t = t0 + tid;
    bool any = false;
    if (t < N) {
      const SvTokenCell tc = sv_token_cell(t, dh, dw, patch, H, W);
      if (ranges) {
        const int rlo = sv_src_index(tc.i0, sh_, Hm), rhi = sv_src_index(tc.i1, sh_, Hm);
        const int clo = sv_src_index(tc.j0, sw_, Wm), chi = sv_src_index(tc.j1, sw_, Wm);
        const int w0 = rlo >> 5, w1 = rhi >> 5;
        for (int c = clo; c <= chi && !any; ++c) {
          for (int wv = w0; wv <= w1; ++wv) {   // the row range as word masks of the source column
            const int lo_b = (wv == w0) ? (rlo & 31) : 0, hi_b = (wv == w1) ? (rhi & 31) : 31;
            const uint32_t msk = (hi_b == 31 ? 0xffffffffu : ((1u << (hi_b + 1)) - 1u)) & ~((1u << lo_b) - 1u);
            if (bits[c * wst + wv] & msk) { any = true; break; }
          }
        }
      } else {
        int pr = -1;
        for (int i = tc.i0; i <= tc.i1 && !any; ++i) {
          const int r = sv_src_index(i, sh_, Hm);
          if (r == pr) continue;
          pr = r;
          int pc = -1;
          for (int j = tc.j0; j <= tc.j1; ++j) {
            const int c = sv_src_index(j, sw_, Wm);
            if (c == pc) continue;
            pc = c;
            if ((bits[c * wst + (r >> 5)] >> (r & 31)) & 1u) { any = true; break; }
          }
        }
      }
    }
    const uint64_t b = __ballot(any);
    const int word = t >> 6;
    if ((tid & 63) == 0 && word < nw) inc[(size_t)s * nw + word] = b;
  }
}

// grid (S, n_ct * n_rt): window (ct, rt) = columns [ct tw, ...) x row words [rt thw, ...).  vec4: Wm, tw and the output pointer are
// multiples of 4 -- four columns per store.
__global__ __launch_bounds__(RLE_THREADS) void rle_decode_kernel(const uint32_t* __restrict__ counts, const int64_t* __restrict__ run_offsets,
                                                                int S, int Hm, int Wm, int tw, int n_ct, int thw, int wst, int vec4,
                                                                uint8_t* __restrict__ out, uint32_t* __restrict__ n_bad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* bits = reinterpret_cast<uint32_t*>(smem);
  __shared__ RleShared sh;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int ct = blockIdx.y % n_ct, rt = blockIdx.y / n_ct;
  const int wpc = (Hm + 31) >> 5;
  RleWindow win;
  win.c0 = ct * tw;
  win.nc = min(tw, Wm - win.c0);
  win.w0 = rt * thw;
  win.nw = min(thw, wpc - win.w0);
  for (int j = tid; j < win.nc * wst; j += RLE_THREADS) bits[j] = 0;
  __syncthreads();
  const int64_t nr = max(run_offsets[S], (int64_t)0);
  const int64_t lo = min(max(run_offsets[s], (int64_t)0), nr), hi = min(max(run_offsets[s + 1], lo), nr);
  const u64 P = (u64)Hm * (u64)Wm;
  const bool judge = ct == n_ct - 1 && rt == 0;   // one window per mask reads every run and reports the mask
  u64 sr = 0, sc = 0, cnt = 0;
  const bool ok = rle_build<false>(counts, lo, hi, (uint32_t)Hm, P, win, judge, bits, wst, sh, cnt, sr, sc);
  if (judge && !ok && n_bad && tid == 0) atomicAdd(n_bad, 1u);
  const int r0 = win.w0 * 32, nrows = min(Hm, (win.w0 + win.nw) * 32) - r0;
  uint8_t* o = out + (size_t)s * P;
  if (vec4) {
    const int q4 = win.nc >> 2;
    for (int q = tid; q < nrows * q4; q += RLE_THREADS) {
      const int rr = q / q4, cc = (q - rr * q4) * 4, r = r0 + rr;
      const uint32_t* p = bits + cc * wst + (rr >> 5);
      const int sft = r & 31;
      const uint32_t v = ((p[0] >> sft) & 1u) | (((p[wst] >> sft) & 1u) << 8) | (((p[2 * wst] >> sft) & 1u) << 16) |
                         (((p[3 * wst] >> sft) & 1u) << 24);
      *reinterpret_cast<uint32_t*>(o + (size_t)r * Wm + win.c0 + cc) = v;
    }
  } else {
    for (int q = tid; q < nrows * win.nc; q += RLE_THREADS) {
      const int rr = q / win.nc, cc = q - rr * win.nc, r = r0 + rr;
      o[(size_t)r * Wm + win.c0 + cc] = (uint8_t)((bits[cc * wst + (rr >> 5)] >> (r & 31)) & 1u);
    }
  }
}

}  // extern "C"

// ---- host side -----------------------------------------------------------------------------------------------------------------
// words between two columns of the bitmap: odd when that still fits (consecutive columns then start on different banks)
static int rle_word_stride(int cols, int words) {
  return ((size_t)cols * (size_t)(words | 1) * 4 <= RLE_LDS_BOUND) ? (words | 1) : words;
}

// The batch's pointers as device pointers.  Host run_offsets are checked here (they index `counts`); device ones are the caller's word,
// like every offset array the library takes in device memory.
static int rle_batch_in(segvlad_ctx* ctx, const char* what, const uint32_t* counts, const int64_t* run_offsets, int S, const uint32_t** dcounts,
                        const int64_t** doffs) {
  int64_t n_runs = 0;
  const bool offs_dev = sv_is_device_ptr(run_offsets), counts_dev = counts && sv_is_device_ptr(counts);
  if (!offs_dev) {
    if (run_offsets[0] < 0) return ctx->fail(SEGVLAD_ERR_ARG, "%s: run_offsets[0] < 0", what);
    for (int s = 0; s < S; ++s)
      if (run_offsets[s + 1] < run_offsets[s]) return ctx->fail(SEGVLAD_ERR_ARG, "%s: run_offsets decrease at %d", what, s);
    n_runs = run_offsets[S];
  } else if (!counts_dev) {   // host counts under device offsets: the staging copy needs its length
    SV_HIP(hipMemcpyAsync(&n_runs, run_offsets + S, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    if (n_runs < 0) return ctx->fail(SEGVLAD_ERR_ARG, "%s: run_offsets[S] < 0", what);
  }
  if (!counts && (offs_dev || n_runs > 0)) return ctx->fail(SEGVLAD_ERR_ARG, "%s: null counts", what);
  const void *dc = counts, *dof;
  if (!counts_dev) SV_TRY(sv_in(ctx, counts, (size_t)n_runs * sizeof(uint32_t), &dc));
  SV_TRY(sv_in(ctx, run_offsets, ((size_t)S + 1) * sizeof(int64_t), &dof));
  *dcounts = (const uint32_t*)dc;
  *doffs = (const int64_t*)dof;
  return SEGVLAD_OK;
}

extern "C" int segvlad_incidence_rle(segvlad_ctx* ctx, const uint32_t* counts, const int64_t* run_offsets, int S, int Hm, int Wm, int H, int W,
                                     int patch, uint64_t* inc_bits, double* centroids, uint32_t* n_bad_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("incidence_rle");
  if (S < 0 || Hm <= 0 || Wm <= 0 || H <= 0 || W <= 0 || patch <= 0 || H / patch <= 0 || W / patch <= 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "incidence_rle: bad geometry S=%d masks %dx%d image %dx%d patch %d", S, Hm, Wm, H, W, patch);
  if (S == 0) return SEGVLAD_OK;
  if (!run_offsets || !inc_bits) return ctx->fail(SEGVLAD_ERR_ARG, "incidence_rle: null pointer");
  if (n_bad_out && !sv_is_device_ptr(n_bad_out)) return ctx->fail(SEGVLAD_ERR_ARG, "incidence_rle: n_bad_out must be device memory");
  const int wpc = (Hm + 31) / 32;
  const size_t bitmap = (size_t)Wm * (size_t)wpc * 4;
  if (bitmap > RLE_LDS_BOUND)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "incidence_rle: the %dx%d bitmap (%zu bytes) exceeds 150 KiB of LDS: inflate the batch with "
                     "segvlad_rle_decode and call segvlad_incidence_centroids", Hm, Wm, bitmap);
  const int dh = H / patch, dw = W / patch, N = dh * dw, nw = (N + 63) / 64;
  const uint32_t* dc;
  const int64_t* dof;
  SV_TRY(rle_batch_in(ctx, "incidence_rle", counts, run_offsets, S, &dc, &dof));
  void *dout, *dcent = nullptr;
  SV_TRY(sv_out(ctx, inc_bits, (size_t)S * nw * 8, &dout));
  if (centroids) SV_TRY(sv_out(ctx, centroids, (size_t)S * 2 * sizeof(double), &dcent));
  const int wst = rle_word_stride(Wm, wpc);
  const size_t lds = (size_t)Wm * wst * 4;
  if (lds + sizeof(RleShared) > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(incidence_rle_kernel), lds));
  StageScope sc(ctx, "incidence_rle");
  hipLaunchKernelGGL(incidence_rle_kernel, dim3(S), dim3(RLE_THREADS), lds, ctx->stream, dc, dof, S, Hm, Wm, H, W, patch, dh, dw,
                     (float)Hm / (float)H, (float)Wm / (float)W, wst, (uint64_t*)dout, nw, (double*)dcent, n_bad_out);
  SV_HIP(hipGetLastError());
  sc.count();
  return sv_finish(ctx);
}

extern "C" int segvlad_rle_decode(segvlad_ctx* ctx, const uint32_t* counts, const int64_t* run_offsets, int S, int Hm, int Wm, uint8_t* masks_out,
                                  uint32_t* n_bad_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("rle_decode");
  if (S < 0 || Hm <= 0 || Wm <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "rle_decode: bad geometry S=%d masks %dx%d", S, Hm, Wm);
  if (S == 0) return SEGVLAD_OK;
  if (!run_offsets || !masks_out) return ctx->fail(SEGVLAD_ERR_ARG, "rle_decode: null pointer");
  if (n_bad_out && !sv_is_device_ptr(n_bad_out)) return ctx->fail(SEGVLAD_ERR_ARG, "rle_decode: n_bad_out must be device memory");
  // the windows: whole columns while one fits the bound (as many per window as fit, a multiple of 4 for the wide stores, spread evenly),
  // else single columns cut into row-word ranges
  const int wpc = (Hm + 31) / 32;
  int tw, n_ct, thw, n_rt;
  if ((size_t)wpc * 4 <= RLE_LDS_BOUND) {
    int fit = (int)std::min<size_t>(RLE_LDS_BOUND / ((size_t)wpc * 4), (size_t)Wm);
    if (fit >= 4) fit &= ~3;
    n_ct = (Wm + fit - 1) / fit;
    tw = (Wm + n_ct - 1) / n_ct;
    if (fit >= 4) tw = (tw + 3) & ~3;
    n_ct = (Wm + tw - 1) / tw;
    thw = wpc, n_rt = 1;
  } else {
    tw = 1, n_ct = Wm;
    thw = (int)(RLE_LDS_BOUND / 4);
    n_rt = (wpc + thw - 1) / thw;
  }
  if ((int64_t)n_ct * n_rt > 65535)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "rle_decode: %dx%d masks need %lld windows per mask (at most 65535)", Hm, Wm, (long long)n_ct * n_rt);
  const uint32_t* dc;
  const int64_t* dof;
  SV_TRY(rle_batch_in(ctx, "rle_decode", counts, run_offsets, S, &dc, &dof));
  void* dout;
  SV_TRY(sv_out(ctx, masks_out, (size_t)S * Hm * Wm, &dout));
  const int wst = rle_word_stride(tw, thw);
  const size_t lds = (size_t)tw * wst * 4;
  const int vec4 = (Wm % 4 == 0 && tw % 4 == 0 && (reinterpret_cast<uintptr_t>(dout) & 3) == 0) ? 1 : 0;
  if (lds + sizeof(RleShared) > 64 * 1024) SV_HIP(sv_max_dyn_lds(reinterpret_cast<const void*>(rle_decode_kernel), lds));
  StageScope sc(ctx, "rle_decode");
  hipLaunchKernelGGL(rle_decode_kernel, dim3(S, n_ct * n_rt), dim3(RLE_THREADS), lds, ctx->stream, dc, dof, S, Hm, Wm, tw, n_ct, thw, wst, vec4,
                     (uint8_t*)dout, n_bad_out);
  SV_HIP(hipGetLastError());
  sc.count();
  return sv_finish(ctx);
}
