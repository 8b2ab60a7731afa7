// Token cells and nearest-neighbour source indices of the incidence kernels: ONE definition for the kernels that read dense
// mask bytes (mask_kernels.hip) and the one that reads run-length masks (rle_kernels.hip), so that every path samples the
// same source pixels (func_vpr.py:1088-1092: F.interpolate(mode="nearest") to H x W, then the patch x patch cells).
#pragma once
#include <hip/hip_runtime.h>

// destination pixel rows i0 .. i1 and columns j0 .. j1 (inclusive) of token t; the last token row / column takes the ragged strip
struct SvTokenCell {
  int i0, i1, j0, j1;
};
__device__ __forceinline__ SvTokenCell sv_token_cell(int t, int dh, int dw, int patch, int H, int W) {
  const int ty = t / dw, tx = t - ty * dw;
  SvTokenCell c;
  c.i0 = ty * patch;
  c.i1 = (ty == dh - 1) ? H - 1 : c.i0 + patch - 1;
  c.j0 = tx * patch;
  c.j1 = (tx == dw - 1) ? W - 1 : c.j0 + patch - 1;
  return c;
}
// nearest: src = min(floor(dst * scale), n_in - 1), scale = fp32(n_in) / fp32(n_out)
__device__ __forceinline__ int sv_src_index(int dst, float scale, int n_in) { return min((int)floorf((float)dst * scale), n_in - 1); }
