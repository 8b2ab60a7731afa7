// The tile walk of the fp16 kNN filter (knn_f16_filter_kernel, knn_filter_kernels.hip), once, for the kernel and its launcher:
// which tile a position of an XCD's sequence is, how long that sequence is, how large the grid, and the order a step runs its
// k-tiles in.  Plain C++ (no HIP runtime, no ctx.h): tests/f16_walk_main.cpp runs the walk on the CPU.
//
//   f16_walk_geometry   tiles, requested block height, walk bits -> F16Walk {gm, seq_total}; f16_walk_grid: workgroups of a launch
//   f16_walk_tile_of    (position, XCD) -> (tm, tn) | none
//   f16_walk_rev_of, f16_walk_kofs   the k-order of a step
//
// XCD-aware tile order.  Workgroup ids are dealt round-robin to the 8 XCDs (each with its own 4 MiB L2); the 32
// workgroups an XCD runs side by side form one gm x (32/gm) block of tiles, so that they share their query and
// database rows in that L2 while they march over k (tm-fastest order made every XCD fetch every database row).
// An XCD's sequence has 32 positions per step: position sq is tile `sq & 31` of the block of step `sq >> 5`.  A plain launch has
// one workgroup per position and XCD; the persistent kernels keep `resident` workgroups per XCD, which walk the sequence
// `resident` positions at a time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SV_WALK_FN __host__ __device__ __forceinline__
#else
#define SV_WALK_FN inline
#endif

constexpr int SV_F16_HBK = 64;   // fp16 elements of a row per k-tile

// walk bit 0 ("query-block-resident"): an XCD keeps ONE block of gm query tiles while it steps through its share of the
// database blocks (blocks xcd, xcd + 8, ... -- the direction alternates from one query block to the next), instead of
// meeting a different query block at every step: the gm query tiles (gm x 512 KiB of fp16 rows at d = 1024) are then
// re-referenced by every step.  walk bit 1 ("serpentine k"): odd steps run their k-tiles from the END of the rows to the
// start.  Under an LRU-like L2 a cyclic re-reference of a working set larger than the cache (4 MiB of query tiles + 2 MiB
// of database tiles per step against 4 MiB of L2 per XCD) never hits; reversing the direction makes the most recently
// used half of the resident block hit (the filter's result does not depend on the accumulation order: the margin
// sv_f16_c_eps bounds ANY order).
// walk bit 2 ("rotated k start"): workgroup (i_m, i_n) of the XCD's gm x gn block starts its k-loop at k-tile
// (i_m ntiles / gm + i_n) mod ntiles and wraps around.  The gm workgroups that share a database tile (and the gn that share a
// query tile) otherwise ask for the same k-slice at the same moment: one L2 miss, everybody waiting out its HBM latency;
// rotated, a slice is fetched by the first workgroup that reaches it and is an L2 HIT for the others, one to two k-tiles
// later.  The k-order of a step: rot, rot + 1, ... (mod ntiles), or -- serpentine, odd steps -- rot - 1, rot - 2, ...: the
// reversed step starts on the slice the previous one ended on.

// The blocks of a walk: gm x gn tiles each, sm_cnt x sn_cnt of them.  Bit 0 cuts the sn_cnt database blocks into 8 nbf + rem:
// every XCD sweeps nbf of them per query block; the sm_cnt x rem left-over (query block, database block) pairs are dealt
// round-robin to the XCDs at the end of the sequence (all of a query block's left-overs on XCD 0 would lengthen that XCD's
// sequence by sm_cnt steps: +0.7 % on the bench shape).
// steps of an XCD's sequence: its share of the blocks (bit 0: of the swept pairs, then of the left-over pairs)
SV_WALK_FN int64_t f16_walk_steps(int tiles_m, int tiles_n, int gm, int walk) {
  const int gn = 32 / gm;
  const int64_t sm_cnt = (tiles_m + gm - 1) / gm, sn_cnt = (tiles_n + gn - 1) / gn, nbf = sn_cnt >> 3, rem = sn_cnt - 8 * nbf;
  return (walk & 1) ? sm_cnt * nbf + (sm_cnt * rem + 7) / 8 : (sm_cnt * sn_cnt + 7) / 8;
}

// tile of position sq in the sequence of XCD xcd; false: the position lies beyond the tiles (edge blocks, the last step).
// The body is a statement macro, expanded in f16_walk_tile_of below and in the kernel's own tile_of lambda: called as a function
// from that lambda (force-inlined or not, out-parameters or a returned struct) hipcc lays the walk's blocks out differently and
// every kernel gains 4 to 17 scalar instructions, on the path between a tile's k-loop and its epilogue -- measured as about 0.1 ms of
// the bench's 17.4 ms of filter launches (profiles/knn_filter_split_ab.txt).
#define SV_F16_WALK_TILE_OF(sq, xcd_arg, tiles_m, tiles_n, gm, walk, tm_, tn_)                      \
  const int xcd = (xcd_arg), within = (sq) & 31;                                                     \
  const int gn = 32 / (gm), sm_cnt = ((tiles_m) + (gm) - 1) / (gm);                                  \
  if ((walk) & 1) {                                                                                  \
    const int sn_cnt = ((tiles_n) + gn - 1) / gn, nbf = sn_cnt >> 3, rem = sn_cnt - 8 * nbf;         \
    const int s_ = (sq) >> 5;                                                                        \
    int qb, nb;                                                                                      \
    if (s_ < sm_cnt * nbf) {                                                                         \
      qb = s_ / nbf;                                                                                 \
      int j = s_ - qb * nbf;                                                                         \
      if (qb & 1) j = nbf - 1 - j;                                                                   \
      nb = j * 8 + xcd;                                                                              \
    } else {                                                                                         \
      const int idx = (s_ - sm_cnt * nbf) * 8 + xcd;                                                 \
      if (rem == 0 || idx >= sm_cnt * rem) return false;                                             \
      qb = idx / rem;                                                                                \
      nb = 8 * nbf + (idx - qb * rem);                                                               \
    }                                                                                                \
    tm_ = qb * (gm) + within % (gm);                                                                 \
    tn_ = nb * gn + within / (gm);                                                                   \
  } else {                                                                                           \
    const int st = ((sq) >> 5) * 8 + xcd;                                                            \
    tm_ = (st % sm_cnt) * (gm) + within % (gm);                                                      \
    tn_ = (st / sm_cnt) * gn + within / (gm);                                                        \
  }                                                                                                  \
  return tm_ < (tiles_m) && tn_ < (tiles_n);
SV_WALK_FN bool f16_walk_tile_of(int sq, int xcd_, int tiles_m, int tiles_n, int gm, int walk, int& tm_, int& tn_) {
  SV_F16_WALK_TILE_OF(sq, xcd_, tiles_m, tiles_n, gm, walk, tm_, tn_)
}

// The k-order of the step position sq belongs to (ntiles k-tiles; wave-uniform).  rev_of packs it: bit 0 = reversed, bits 1.. = rot;
// kofs: the element offset of the x-th k-tile the step runs.
SV_WALK_FN int f16_walk_rev_of(int sq, int gm, int ntiles, int walk) {
  int rot = 0;
  if (walk & 4) {
    const int within = sq & 31, im = within % gm, in_ = within / gm;
    rot = (im * (ntiles >= gm ? ntiles / gm : 1) + in_) % ntiles;
  }
  return 2 * rot + (((walk & 2) && ((sq >> 5) & 1)) ? 1 : 0);
}
SV_WALK_FN int f16_walk_kofs(int rev_, int x, int ntiles) {
  const int rot = rev_ >> 1;
  int i = (rev_ & 1) ? rot - 1 - x : rot + x;
  if (i < 0) i += ntiles;
  if (i >= ntiles) i -= ntiles;
  return i * SV_F16_HBK;
}

// Geometry of a launch over tiles_m x tiles_n tiles.  gm_req: the block height asked for (< 0: the default; 0: no walk, plain
// tm-fastest order, one workgroup per tile), clamped to a power of two <= 32 and halved while half of it still covers tiles_m.
// Every database tile is fetched once per block ROW of query tiles: with >= 16 query tiles (one pass over 10 000 queries has 40)
// blocks of 8 x 4 halve that re-read against 4 x 8 (10 -> 5 fetches of the fp16 plane per launch) at the same speed; 16 x 2 is 14 %
// slower (the 16 query tiles no longer stay in the XCD's L2).
struct F16Walk {
  int gm;              // block height (0: plain order)
  int64_t seq_total;   // positions of an XCD's sequence (0: plain order)
  int64_t tiles;       // tiles_m x tiles_n
};
SV_WALK_FN F16Walk f16_walk_geometry(int tiles_m, int tiles_n, int gm_req, int walk) {
  F16Walk g;
  g.gm = gm_req >= 0 ? gm_req : (tiles_m >= 16 ? 8 : 4);
  g.seq_total = 0;
  g.tiles = (int64_t)tiles_m * tiles_n;
  if (g.gm > 0) {
    g.gm = g.gm >= 32 ? 32 : g.gm >= 16 ? 16 : g.gm >= 8 ? 8 : g.gm >= 4 ? 4 : g.gm >= 2 ? 2 : 1;
    while (g.gm > 1 && g.gm / 2 >= tiles_m) g.gm >>= 1;
    g.seq_total = f16_walk_steps(tiles_m, tiles_n, g.gm, walk) * 32;
  }
  return g;
}
// workgroups of the launch.  resident > 0 (persistent kernels): 8 XCDs x `resident` workgroups, workgroup b starts at position
// b >> 3 of XCD b & 7 and steps by `resident`; otherwise one workgroup per position and XCD (plain order: per tile).
SV_WALK_FN int64_t f16_walk_grid(const F16Walk& g, int resident) {
  if (g.gm <= 0) return g.tiles;
  return resident > 0 ? 8 * (int64_t)resident : 8 * g.seq_total;
}
