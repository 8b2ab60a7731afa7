// Small holes and small islands removed from a batch of dense masks on the device: remove_small_regions for every mask, mode
// "holes" and then mode "islands" (sam/segment_anything/utils/amg.py:267-291), the step SamAutomaticMaskGenerator.
// postprocess_small_regions runs before its second box NMS (automatic_mask_generator.py:325-376).  The reference labels with
// OpenCV on the host, one mask at a time; here the whole batch is labelled at once (segvlad_mask_regions).
//
// One PASS labels the 8-connected components of a working mask (holes: the complement of the input; islands: the result of the
// holes pass) and rewrites the mask from the components' sizes.  The label plane holds, per pixel, the index (inside its mask) of a
// pixel of the same component that comes no later in row-major order -- a union-find forest whose roots are the components' FIRST
// pixels --, or -1 for a pixel outside the working mask.  The size plane holds a component's pixel count at its root.
//   tile     one workgroup per (mask, tile of 32 x 32).  The forest of the tile's pixels is built in LDS: a pixel starts at the first
//            pixel of its horizontal run (a wave holds two tile rows; the run's start comes from the ballot of the working bits), then
//            the links to the row above (N, or NW and NE where N is clear) are united with atomicMin on LDS.  The tile-local
//            components are counted in LDS.  Out: every pixel's label = the global index of its tile-local root; the size plane =
//            the tile-local count at a tile-local root, 0 elsewhere.
//   border   every pixel on a tile's first row, first column or last column unites with those of its W / NW / N / NE neighbours that
//            lie in another tile -- the two diagonal links at every tile corner included -- with atomicMin on the global plane.
//            Links that others imply are left out: a W or N link that the pixel before it along the edge made between the same two
//            tile-local components, and a diagonal link whose two pixels share a set neighbour (W / N links join them through it).
//            A solid region costs one union per tile edge, not one per edge pixel.  The finds of this launch halve the paths.
//            The workgroups of a launch run on different XCDs whose L2s are not coherent with each other: EVERY access to the label
//            plane in this launch is an agent-scope atomic (a relaxed atomic load, or atomicMin).  Plain accesses are used only on
//            the far side of a kernel boundary.
//   flatten  every pixel's label becomes its root; a tile-local root that is not the root adds its tile-local count to the root's:
//            ONE global atomic per (tile, tile-local component), never one per pixel -- in the holes pass the background is one
//            component of nearly P pixels, and a single word takes on the order of a hundred returning atomics per microsecond.
//   decide   per mask over its roots: is any component smaller than min_area, is any at least that large, and the largest as one
//            packed 64-bit maximum of (area, ~root): among equal areas the component whose first pixel comes first wins.
//   apply    every pixel is rewritten.  holes: set if it was set, or if its component (of the complement) is small.  islands: kept
//            if no component is small; else if its component is large; else, when none is large, if its root is the winner.  The
//            islands apply also reduces the result's area and tight box.
// All sums are integers and all roots are minima: two calls write the same bytes.  No mask is held whole in LDS; the only size bound
// is the 32-bit label, Hm Wm <= 2^31 - 1.
//
// The tie for "largest" follows scipy.ndimage.label's numbering (first pixel in row-major order).  OpenCV's numbering under such a
// tie has not been checked against; see segvlad.h.
#include <algorithm>
#include <climits>

#include "ctx.h"

constexpr int RG_TILE = 32;                       // a tile is RG_TILE x RG_TILE pixels: two tile rows per wave
constexpr int RG_TILE_PIX = RG_TILE * RG_TILE;
constexpr int RG_THREADS = 256;
constexpr int RG_PER_THREAD = RG_TILE_PIX / RG_THREADS;
constexpr uint32_t RG_CHUNK = RG_THREADS * 16;    // pixels of one workgroup in the per-pixel kernels
constexpr uint32_t RG_ANY_SMALL = 1u, RG_ANY_LARGE = 2u;
static_assert(RG_TILE == 32 && RG_THREADS % 64 == 0, "the run start below reads one 32-bit half of a wave's ballot per tile row");

typedef unsigned long long u64;

// per mask: [0] the holes pass, [1] the islands pass
struct RgState {
  u64 best[2];        // (area << 32) | ~root of the largest component
  u64 area;           // set pixels of the result
  uint32_t flags[2];  // RG_ANY_SMALL | RG_ANY_LARGE
  int32_t x0, y0, x1, y1;
};

__device__ __forceinline__ int rg_ld_lds(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int rg_ld(const int* L, uint32_t i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int rg_find_lds(const int* L, int a) {
  for (int v; (v = rg_ld_lds(L, a)) != a;) a = v;
  return a;
}
__device__ __forceinline__ int rg_find(const int* L, int a) {
  for (int v; (v = rg_ld(L, (uint32_t)a)) != a;) a = v;
  return a;
}
// the same with path halving, for the launch that unites: every node on the way is hung below its grandparent (an ancestor, so the
// forest stays one of decreasing labels); the chains of tile roots that one large component builds stay short
__device__ __forceinline__ int rg_find_halving(int* L, int a) {
  int v = rg_ld(L, (uint32_t)a);
  while (v != a) {
    const int w = rg_ld(L, (uint32_t)v);
    if (w != v) atomicMin(&L[a], w);
    a = v, v = w;
  }
  return a;
}
// Both unite a root with a smaller root.  When the atomicMin finds that a is no longer a root, a has been hung below `old` by
// somebody else and now hangs below min(old, b): the loop goes on to unite old with b, which restores whichever link was lost.
__device__ __forceinline__ void rg_unite_lds(int* L, int a, int b) {
  for (;;) {
    a = rg_find_lds(L, a), b = rg_find_lds(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}
__device__ __forceinline__ void rg_unite(int* L, int a, int b) {
  for (;;) {
    a = rg_find_halving(L, a), b = rg_find_halving(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

// item -> (mask, [p0, p1) of its pixels); the per-pixel kernels give one workgroup RG_CHUNK pixels of ONE mask
__device__ __forceinline__ void rg_chunk(int64_t item, int64_t cpm, uint32_t P, int& s, uint32_t& p0, uint32_t& p1) {
  s = (int)(item / cpm);
  p0 = (uint32_t)(item % cpm) * RG_CHUNK;
  p1 = (uint32_t)min((u64)P, (u64)p0 + RG_CHUNK);
}

__global__ __launch_bounds__(RG_THREADS) void regions_init_kernel(RgState* __restrict__ st, int S) {
  const int s = blockIdx.x * RG_THREADS + threadIdx.x;
  if (s >= S) return;
  RgState z;
  z.best[0] = z.best[1] = 0, z.area = 0, z.flags[0] = z.flags[1] = 0;
  z.x0 = z.y0 = INT_MAX, z.x1 = z.y1 = -1;
  st[s] = z;
}

// label, tsize: [S][P]
__global__ __launch_bounds__(RG_THREADS) void regions_tile_kernel(const uint8_t* __restrict__ masks, int S, int Hm, int Wm, int ntx, int nty,
                                                                 int invert, int* __restrict__ label, uint32_t* __restrict__ tsize) {
  __shared__ int L[RG_TILE_PIX];
  __shared__ int cnt[RG_TILE_PIX];
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t P = (size_t)Hm * Wm;
  const int64_t tiles = (int64_t)ntx * nty, items = (int64_t)S * tiles;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int s = (int)(item / tiles), t = (int)(item % tiles);
    const int ty0 = (t / ntx) * RG_TILE, tx0 = (t % ntx) * RG_TILE;
    const uint8_t* m = masks + (size_t)s * P;
#pragma unroll
    for (int it = 0; it < RG_PER_THREAD; ++it) {   // i & 31 == lane & 31: a wave is two tile rows
      const int i = it * RG_THREADS + tid, ly = i >> 5, lx = i & 31, gy = ty0 + ly, gx = tx0 + lx;
      const bool w = gy < Hm && gx < Wm && ((m[(size_t)gy * Wm + gx] != 0) != (invert != 0));
      const u64 b = __ballot(w);
      const uint32_t row = lane < 32 ? (uint32_t)b : (uint32_t)(b >> 32);
      const uint32_t clear_before = ~row & ((1u << lx) - 1u);
      const int start = clear_before ? 32 - __clz(clear_before) : 0;   // the first pixel of this pixel's horizontal run
      L[i] = w ? ly * RG_TILE + start : -1;
      cnt[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RG_PER_THREAD; ++it) {
      const int i = it * RG_THREADS + tid, ly = i >> 5, lx = i & 31;
      if (ly == 0 || rg_ld_lds(L, i) < 0) continue;
      if (rg_ld_lds(L, i - RG_TILE) >= 0) {
        rg_unite_lds(L, i, i - RG_TILE);   // N: its run holds NW and NE when they are set
      } else {
        if (lx > 0 && rg_ld_lds(L, i - RG_TILE - 1) >= 0) rg_unite_lds(L, i, i - RG_TILE - 1);
        if (lx < RG_TILE - 1 && rg_ld_lds(L, i - RG_TILE + 1) >= 0) rg_unite_lds(L, i, i - RG_TILE + 1);
      }
    }
    __syncthreads();
    int root[RG_PER_THREAD];
#pragma unroll
    for (int it = 0; it < RG_PER_THREAD; ++it) {
      const int i = it * RG_THREADS + tid;
      const bool w = L[i] >= 0;
      root[it] = w ? rg_find_lds(L, i) : -1;
      // one LDS add per wave for the root its first working lane has (a tile inside one component: one add), one per lane for the others
      const u64 wb = __ballot(w);
      if (wb) {
        const int first = __shfl(root[it], __ffsll((long long)wb) - 1);
        const u64 same = __ballot(w && root[it] == first);
        if (w && root[it] != first) atomicAdd(&cnt[root[it]], 1);
        else if (w && lane == __ffsll((long long)same) - 1) atomicAdd(&cnt[first], __popcll(same));
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RG_PER_THREAD; ++it) {
      const int i = it * RG_THREADS + tid, ly = i >> 5, lx = i & 31, gy = ty0 + ly, gx = tx0 + lx;
      if (gy >= Hm || gx >= Wm) continue;
      const size_t at = (size_t)s * P + (size_t)gy * Wm + gx;
      const int r = root[it];
      label[at] = r < 0 ? -1 : (int)((uint32_t)(ty0 + (r >> 5)) * (uint32_t)Wm + (uint32_t)(tx0 + (r & 31)));
      tsize[at] = r == i ? (uint32_t)cnt[i] : 0u;
    }
    __syncthreads();   // L and cnt are the next item's
  }
}

// Every access to `label` here is an agent-scope atomic (see the head of the file).
__global__ __launch_bounds__(RG_THREADS) void regions_border_kernel(int* __restrict__ label, int S, int Hm, int Wm, int64_t cpm) {
  const uint32_t P = (uint32_t)Hm * (uint32_t)Wm;
  const int64_t items = (int64_t)S * cpm;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    int s;
    uint32_t p0, p1;
    rg_chunk(item, cpm, P, s, p0, p1);
    int* L = label + (size_t)s * P;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += RG_THREADS) {
      const uint32_t y = p / (uint32_t)Wm, x = p - y * (uint32_t)Wm;
      const bool top = (y & (RG_TILE - 1)) == 0, left = (x & (RG_TILE - 1)) == 0, right = (x & (RG_TILE - 1)) == RG_TILE - 1;
      if (!(top || left || right)) continue;
      const bool up = y > 0, lf = x > 0, rt = x + 1 < (uint32_t)Wm;
      if (!((left && lf) || (up && (top || (left && lf) || (right && rt))))) continue;
      const auto set = [&](uint32_t q) { return rg_ld(L, q) >= 0; };
      if (!set(p)) continue;
      const bool w = lf && set(p - 1), n = up && set(p - Wm);
      // W across a tile's left edge -- not where the row above made the same link: both pixels above are set and lie in these two tiles
      if (left && w && !(up && !top && n && set(p - Wm - 1))) rg_unite(L, (int)p, (int)(p - 1));
      // N across a tile's top edge -- not where the pixel before made the same link
      if (top && n && !(lf && !left && w && set(p - Wm - 1))) rg_unite(L, (int)p, (int)(p - Wm));
      // the diagonals, only where the two pixels they share as neighbours are both clear: a set one joins them through W / N links
      if (up && lf && (top || left) && !n && !w && set(p - Wm - 1)) rg_unite(L, (int)p, (int)(p - Wm - 1));
      if (up && rt && (top || right) && !n && !set(p + 1) && set(p - Wm + 1)) rg_unite(L, (int)p, (int)(p - Wm + 1));
    }
  }
}

// label[p] <- root(p); size[root] += the tile-local count of every tile-local root below it.  A tile-local root that is not the
// root is never added to (sums go to roots only), so its count is read plainly; the root's own word is only added to.
__global__ __launch_bounds__(RG_THREADS) void regions_flatten_kernel(int* __restrict__ label, uint32_t* __restrict__ size, int S, int Hm, int Wm,
                                                                    int64_t cpm) {
  const uint32_t P = (uint32_t)Hm * (uint32_t)Wm;
  const int64_t items = (int64_t)S * cpm;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    int s;
    uint32_t p0, p1;
    rg_chunk(item, cpm, P, s, p0, p1);
    int* L = label + (size_t)s * P;
    uint32_t* Z = size + (size_t)s * P;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += RG_THREADS) {
      const int l = rg_ld(L, p);
      if (l < 0) continue;
      const int r = rg_find(L, l);
      if (r != l) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r != (int)p) {
        const uint32_t n = Z[p];
        if (n) atomicAdd(&Z[r], n);
      }
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void regions_decide_kernel(const int* __restrict__ label, const uint32_t* __restrict__ size, int S, int Hm,
                                                                   int Wm, int64_t cpm, uint32_t min_area, int pass, RgState* __restrict__ st) {
  __shared__ u64 wbest[RG_THREADS / 64];
  __shared__ uint32_t wflags[RG_THREADS / 64];
  const uint32_t P = (uint32_t)Hm * (uint32_t)Wm;
  const int64_t items = (int64_t)S * cpm;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    int s;
    uint32_t p0, p1;
    rg_chunk(item, cpm, P, s, p0, p1);
    const int* L = label + (size_t)s * P;
    const uint32_t* Z = size + (size_t)s * P;
    u64 best = 0;
    uint32_t flags = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += RG_THREADS) {
      if (L[p] != (int)p) continue;
      const uint32_t n = Z[p];
      flags |= n < min_area ? RG_ANY_SMALL : RG_ANY_LARGE;
      best = max(best, ((u64)n << 32) | (u64)(~p));
    }
    for (int o = 32; o > 0; o >>= 1) {
      best = max(best, (u64)__shfl_xor(best, o));
      flags |= __shfl_xor(flags, o);
    }
    if (lane == 0) wbest[wv] = best, wflags[wv] = flags;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < RG_THREADS / 64; ++k) best = max(best, wbest[k]), flags |= wflags[k];
      if (flags) {
        atomicOr(&st[s].flags[pass], flags);
        atomicMax(&st[s].best[pass], best);
      }
    }
    __syncthreads();
  }
}

// MODE 0: the holes pass; 1: the islands pass (+ area and box of the result); 2: no pass at all (min_area <= 1): the bytes as 0 / 1
// (+ area and box).  in == out is allowed: a thread reads the byte it writes.
template <int MODE>
__global__ __launch_bounds__(RG_THREADS) void regions_apply_kernel(const uint8_t* in, uint8_t* out, const int* __restrict__ label,
                                                                  const uint32_t* __restrict__ size, int S, int Hm, int Wm, int64_t cpm,
                                                                  uint32_t min_area, RgState* __restrict__ st) {
  __shared__ uint32_t warea[RG_THREADS / 64];
  __shared__ int wbox[RG_THREADS / 64][4];
  const uint32_t P = (uint32_t)Hm * (uint32_t)Wm;
  const int64_t items = (int64_t)S * cpm;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    int s;
    uint32_t p0, p1;
    rg_chunk(item, cpm, P, s, p0, p1);
    const size_t base = (size_t)s * P;
    uint32_t flags = 0, winner = 0;
    if (MODE == 1) {
      flags = st[s].flags[1];   // written by the decide launch, read-only here
      winner = ~(uint32_t)st[s].best[1];
    }
    uint32_t area = 0;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += RG_THREADS) {
      bool v = in[base + p] != 0;
      if (MODE == 0) {
        const int r = label[base + p];
        v = v || (r >= 0 && size[base + (uint32_t)r] < min_area);
      } else if (MODE == 1) {
        if (v && (flags & RG_ANY_SMALL)) {
          const uint32_t r = (uint32_t)label[base + p];
          v = (flags & RG_ANY_LARGE) ? size[base + r] >= min_area : r == winner;
        }
      }
      out[base + p] = v ? 1 : 0;
      if (MODE != 0 && v) {
        const int y = (int)(p / (uint32_t)Wm), x = (int)(p - (uint32_t)y * (uint32_t)Wm);
        ++area;
        x0 = min(x0, x), x1 = max(x1, x), y0 = min(y0, y), y1 = max(y1, y);
      }
    }
    if (MODE != 0) {
      for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o);
        x0 = min(x0, __shfl_xor(x0, o)), y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)), y1 = max(y1, __shfl_xor(y1, o));
      }
      if (lane == 0) warea[wv] = area, wbox[wv][0] = x0, wbox[wv][1] = y0, wbox[wv][2] = x1, wbox[wv][3] = y1;
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int k = 1; k < RG_THREADS / 64; ++k) {
          area += warea[k];
          x0 = min(x0, wbox[k][0]), y0 = min(y0, wbox[k][1]), x1 = max(x1, wbox[k][2]), y1 = max(y1, wbox[k][3]);
        }
        if (area) {
          atomicAdd(&st[s].area, (u64)area);
          atomicMin(&st[s].x0, x0), atomicMin(&st[s].y0, y0), atomicMax(&st[s].x1, x1), atomicMax(&st[s].y1, y1);
        }
      }
      __syncthreads();
    }
  }
}

// changed [S]: bit 0 the holes pass, bit 1 the islands pass; boxes [S][4] XYXY inclusive, zeros for an empty mask; any may be null
__global__ __launch_bounds__(RG_THREADS) void regions_finish_kernel(const RgState* __restrict__ st, int S, int32_t* __restrict__ changed,
                                                                   int32_t* __restrict__ boxes, int64_t* __restrict__ area) {
  const int s = blockIdx.x * RG_THREADS + threadIdx.x;
  if (s >= S) return;
  const RgState z = st[s];
  if (changed) changed[s] = (int32_t)((z.flags[0] & RG_ANY_SMALL) | ((z.flags[1] & RG_ANY_SMALL) << 1));
  if (boxes) {
    const bool any = z.area != 0;
    boxes[4 * (size_t)s + 0] = any ? z.x0 : 0, boxes[4 * (size_t)s + 1] = any ? z.y0 : 0;
    boxes[4 * (size_t)s + 2] = any ? z.x1 : 0, boxes[4 * (size_t)s + 3] = any ? z.y1 : 0;
  }
  if (area) area[s] = (int64_t)z.area;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int segvlad_mask_regions(segvlad_ctx* ctx, const uint8_t* masks, int S, int Hm, int Wm, int min_area, uint8_t* masks_out,
                                    int32_t* changed_out, int32_t* boxes_out, int64_t* area_out) {
  CHECK_CTX();
  CHECK_NO_OPEN_DESCRIBE("mask_regions");
  if (S < 0 || Hm <= 0 || Wm <= 0 || min_area < 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "mask_regions: bad arguments S=%d masks %dx%d min_area %d", S, Hm, Wm, min_area);
  const u64 P = (u64)Hm * (u64)Wm;
  if (P > 0x7fffffffull)   // (before any pointer is looked at)
    return ctx->fail(SEGVLAD_ERR_LIMIT, "mask_regions: %dx%d masks have %llu pixels, a label is a 32-bit pixel index (at most 2^31 - 1)", Hm, Wm, P);
  if (S == 0) return SEGVLAD_OK;
  if (!masks || !masks_out) return ctx->fail(SEGVLAD_ERR_ARG, "mask_regions: null pointer");
  const size_t SP = (size_t)S * P;
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(masks), b = reinterpret_cast<uintptr_t>(masks_out);
    if (a != b && a < b + SP && b < a + SP) return ctx->fail(SEGVLAD_ERR_ARG, "mask_regions: masks_out overlaps masks without being masks");
  }
  const void* dm;
  SV_TRY(sv_in(ctx, masks, SP, &dm));
  void *dout, *dchg = nullptr, *dbox = nullptr, *darea = nullptr;
  SV_TRY(sv_out(ctx, masks_out, SP, &dout));
  if (changed_out) SV_TRY(sv_out(ctx, changed_out, (size_t)S * sizeof(int32_t), &dchg));
  if (boxes_out) SV_TRY(sv_out(ctx, boxes_out, (size_t)S * 4 * sizeof(int32_t), &dbox));
  if (area_out) SV_TRY(sv_out(ctx, area_out, (size_t)S * sizeof(int64_t), &darea));
  SV_HIP(ctx->s_rg_state.reserve((size_t)S * sizeof(RgState)));
  RgState* st = ctx->s_rg_state.as<RgState>();
  const int64_t cpm = (int64_t)((P + RG_CHUNK - 1) / RG_CHUNK);
  const int pgrid = (int)std::min<int64_t>((int64_t)S * cpm, 256 * 256), sgrid = (S + RG_THREADS - 1) / RG_THREADS;
  const uint8_t* in = (const uint8_t*)dm;
  uint8_t* out = (uint8_t*)dout;
  {
    StageScope sc(ctx, "mask_regions");
    hipLaunchKernelGGL(regions_init_kernel, dim3(sgrid), dim3(RG_THREADS), 0, ctx->stream, st, S);
    SV_HIP(hipGetLastError());
    sc.count();
    if (min_area <= 1) {   // no component is smaller than one pixel: nothing changes
      hipLaunchKernelGGL(regions_apply_kernel<2>, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, in, out, (const int*)nullptr, (const uint32_t*)nullptr, S,
                         Hm, Wm, cpm, 0u, st);
      SV_HIP(hipGetLastError());
      sc.count();
    } else {
      SV_HIP(ctx->s_rg_label.reserve(SP * sizeof(int32_t)));
      SV_HIP(ctx->s_rg_size.reserve(SP * sizeof(uint32_t)));
      int* label = ctx->s_rg_label.as<int>();
      uint32_t* size = ctx->s_rg_size.as<uint32_t>();
      const int ntx = (Wm + RG_TILE - 1) / RG_TILE, nty = (Hm + RG_TILE - 1) / RG_TILE;
      const int tgrid = (int)std::min<int64_t>((int64_t)S * ntx * nty, 256 * 256);
      for (int pass = 0; pass < 2; ++pass) {   // holes: the complement of the input; islands: the result of the holes pass
        hipLaunchKernelGGL(regions_tile_kernel, dim3(tgrid), dim3(RG_THREADS), 0, ctx->stream, pass == 0 ? in : (const uint8_t*)out, S, Hm, Wm, ntx, nty,
                           pass == 0 ? 1 : 0, label, size);
        SV_HIP(hipGetLastError());
        hipLaunchKernelGGL(regions_border_kernel, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, label, S, Hm, Wm, cpm);
        SV_HIP(hipGetLastError());
        hipLaunchKernelGGL(regions_flatten_kernel, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, label, size, S, Hm, Wm, cpm);
        SV_HIP(hipGetLastError());
        hipLaunchKernelGGL(regions_decide_kernel, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, (const int*)label, (const uint32_t*)size, S, Hm, Wm, cpm,
                           (uint32_t)min_area, pass, st);
        SV_HIP(hipGetLastError());
        if (pass == 0)
          hipLaunchKernelGGL(regions_apply_kernel<0>, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, in, out, (const int*)label, (const uint32_t*)size, S, Hm,
                             Wm, cpm, (uint32_t)min_area, st);
        else
          hipLaunchKernelGGL(regions_apply_kernel<1>, dim3(pgrid), dim3(RG_THREADS), 0, ctx->stream, (const uint8_t*)out, out, (const int*)label,
                             (const uint32_t*)size, S, Hm, Wm, cpm, (uint32_t)min_area, st);
        SV_HIP(hipGetLastError());
        sc.count(5);
      }
    }
    if (dchg || dbox || darea) {
      hipLaunchKernelGGL(regions_finish_kernel, dim3(sgrid), dim3(RG_THREADS), 0, ctx->stream, (const RgState*)st, S, (int32_t*)dchg, (int32_t*)dbox,
                         (int64_t*)darea);
      SV_HIP(hipGetLastError());
      sc.count();
    }
  }
  return sv_finish(ctx);   // host outputs: one synchronisation; device outputs: none
}
