// The fp16 kNN filter's tile walk (csrc/f16_walk.h) on the CPU: test_f16_walk_host.py compiles this with the host compiler and runs it.
// For every walk of the table below:
//   coverage   over the 8 XCDs and their resident workgroups, each stepping by the resident count up to seq_total, every tile
//              (tm, tn) with tm < tiles_m, tn < tiles_n is produced exactly once, and nothing outside that range;
//   k-order    for every position, {kofs(rev_of(sq), x) / 64 : 0 <= x < ntiles} is a permutation of 0 .. ntiles - 1.
// Prints "walk cases <n> k-order cases <n> failures <n>"; exit status 1 when a case failed.
#include <stdio.h>

#include <vector>

#include "f16_walk.h"

int main() {
  const int TILES_M[] = {1, 2, 3, 5, 12, 17, 40}, TILES_N[] = {1, 7, 8, 9, 33, 64, 65, 300}, GM[] = {-1, 1, 2, 4, 8, 16, 32};
  const int RESIDENT[] = {32, 5, 1}, NTILES[] = {1, 2, 3, 4, 16, 64};
  long walks = 0, korders = 0, failures = 0;
  std::vector<int> seen, kseen;
  for (int tiles_m : TILES_M)
    for (int tiles_n : TILES_N)
      for (int gm_req : GM)
        for (int walk = 0; walk < 8; ++walk)
          for (int resident : RESIDENT) {
            ++walks;
            const F16Walk g = f16_walk_geometry(tiles_m, tiles_n, gm_req, walk);
            bool ok = g.gm >= 1 && g.gm <= 32 && (g.gm & (g.gm - 1)) == 0 && g.seq_total > 0 && g.seq_total % 32 == 0 &&
                      g.tiles == (int64_t)tiles_m * tiles_n && f16_walk_grid(g, resident) == 8 * resident &&
                      f16_walk_grid(g, 0) == 8 * g.seq_total;
            seen.assign((size_t)tiles_m * tiles_n, 0);
            for (int wg = 0; ok && wg < f16_walk_grid(g, resident); ++wg)   // workgroup wg: XCD wg & 7, first position wg >> 3
              for (int64_t sq = wg >> 3; sq < g.seq_total; sq += resident) {
                int tm = -1, tn = -1;
                if (!f16_walk_tile_of((int)sq, wg & 7, tiles_m, tiles_n, g.gm, walk, tm, tn)) continue;
                if (tm < 0 || tm >= tiles_m || tn < 0 || tn >= tiles_n) {
                  ok = false;
                  break;
                }
                ++seen[(size_t)tn * tiles_m + tm];
              }
            for (int c : seen) ok = ok && c == 1;
            if (!ok) {
              ++failures;
              fprintf(stderr, "coverage: tiles %d x %d gm %d (-> %d) walk %d resident %d\n", tiles_m, tiles_n, gm_req, g.gm, walk, resident);
            }
            if (resident != RESIDENT[0]) continue;   // (the k-order of a position does not depend on who visits it)
            for (int ntiles : NTILES) {
              ++korders;
              bool kok = true;
              for (int64_t sq = 0; kok && sq < g.seq_total; ++sq) {
                const int rev = f16_walk_rev_of((int)sq, g.gm, ntiles, walk);
                kseen.assign(ntiles, 0);
                for (int x = 0; x < ntiles; ++x) {
                  const int ko = f16_walk_kofs(rev, x, ntiles);
                  if (ko < 0 || ko % SV_F16_HBK != 0 || ko / SV_F16_HBK >= ntiles || kseen[ko / SV_F16_HBK]++) kok = false;
                }
              }
              if (!kok) {
                ++failures;
                fprintf(stderr, "k-order: tiles %d x %d gm %d (-> %d) walk %d ntiles %d\n", tiles_m, tiles_n, gm_req, g.gm, walk, ntiles);
              }
            }
          }
  printf("walk cases %ld k-order cases %ld failures %ld\n", walks, korders, failures);
  return failures ? 1 : 0;
}
