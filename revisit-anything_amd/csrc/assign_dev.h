// What the kernels that score tokens against the vocabulary on the fp32 MFMA share (assign_kernel, assign_wide_kernel:
// assign_kernels.hip; soft_weights_kernel: soft_vlad_kernels.hip): the store of a wave's accumulators into the workgroup's score tile
// in LDS, and the hard assignment's pick of a token's label from its row of that tile.  How a kernel sums its scores is its own: the
// narrow kernel splits D over its waves and combines them in LDS, the wide ones keep one chain per score.
//
// Statement macros, not force-inlined functions: the compiler simplifies a function on its own before it inlines it, and the three
// kernels then come out as other machine code (the pick loop one move longer per cluster, the store scheduled differently).  Expanded in
// place they compile to exactly what they were when each kernel spelled them out (tools/compare_isa.py).
#pragma once
#include "mfma_f32_dev.h"

// Wave w owns tokens 32 w .. 32 w + 31 of the tile for all d: its NT accumulator tiles acc[NT] go to sc [tokens][32 NT + 1] (row =
// token, column = cluster), the squared norm of its tokens -- ss, one half of it in each lane half; summed in place -- to
// ssum [tokens].  (i, kk) = (lane & 31, lane >> 5).  The caller's barrier follows.
#define SV_SCORE_TILE_STORE(NT, acc, ss, sc, ssum, w, i, kk)                                                   \
  do {                                                                                                         \
    (ss) += __shfl_xor((ss), 32);                                                                              \
    if ((kk) == 0) (ssum)[32 * (w) + (i)] = (ss);                                                              \
    _Pragma("unroll") for (int n_ = 0; n_ < (NT); ++n_)                                                        \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_)                                                        \
        (sc)[(32 * (w) + sv_frag_row(r_, (kk))) * ((NT) * 32 + 1) + n_ * 32 + (i)] = (acc)[n_][r_];            \
  } while (0)

// One thread per token: from the token's K scores sc[row0 .. row0 + K) (its row of the score tile) and its squared norm s2, the FIRST
// maximum as the label, 1 / ||x||, and the normalised gap to the runner-up (inf for a vocabulary of one; gap may be null) to position o
// of the three outputs.
#define SV_ASSIGN_TOKEN(sc, row0, K, s2, o, labels, rnorm, gap)            \
  do {                                                                     \
    const float rn_ = 1.0f / fmaxf(sqrtf(s2), 1e-12f);                     \
    float best_ = -INFINITY, second_ = -INFINITY;                          \
    int bi_ = 0;                                                           \
    for (int k_ = 0; k_ < (K); ++k_) {                                     \
      const float v_ = (sc)[(row0) + k_];                                  \
      if (v_ > best_) {                                                    \
        second_ = best_;                                                   \
        best_ = v_;                                                        \
        bi_ = k_;                                                          \
      } else if (v_ > second_) {                                           \
        second_ = v_;                                                      \
      }                                                                    \
    }                                                                      \
    const size_t o_ = (o);                                                 \
    (labels)[o_] = (uint8_t)bi_;                                           \
    (rnorm)[o_] = rn_;                                                     \
    if (gap) (gap)[o_] = ((K) > 1) ? (best_ - second_) * rn_ : INFINITY;   \
  } while (0)
