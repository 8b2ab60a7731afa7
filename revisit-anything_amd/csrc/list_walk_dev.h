// The wave walk over a (distance, id)-ordered list that ex_compact_kernel (exclude_kernels.hip), group_collapse_kernel and
// group_tail_kernel (group_kernels.hip) share: chunks of 64 entries, a rule says which to keep, the kept ones are placed by
// ballot + mbcnt, the walk stops at k kept, (+inf, -1) goes behind them.
//
// A Source gives the entry at position j < n: its distance, its id, and whether it is a real entry.  The entries that are not
// real are a SUFFIX of every list the walk is given -- the inner search pads a list of fewer than k finite distances with
// (+inf, -1) (include/segvlad.h), the all-ones words of the exact sweep order behind every entry -- so the walk stops in the chunk
// that holds the first of them: nothing behind it could be kept, and reading on (as ex_compact_kernel once did) gives the same bits.
// The Rule is called by the WHOLE wave, once per chunk, with each lane's (id, real): the grouped rules read other lanes.
#pragma once
#include "knn_dev.h"

// the inner search's lists: d2 / idx [n], a real entry has id >= 0
struct SvListArrays {
  const float* d2;
  const int64_t* idx;
  int n;
  __device__ __forceinline__ bool get(int j, float& dd, int64_t& id) const {
    dd = d2[j];
    id = idx[j];
    return id >= 0;
  }
};

// the exact sweep's ordered words [n]: distance key << 32 | id, all ones = no entry
struct SvListWords {
  const unsigned long long* w;
  int64_t n;
  __device__ __forceinline__ bool get(int64_t j, float& dd, int64_t& id) const {
    const unsigned long long wd = w[j];
    dd = sv_word_d2(wd);
    id = sv_word_id(wd);
    return wd != SV_WORD_NONE;
  }
};

struct SvWalked {
  int kept;       // entries the rule kept (>= k: the row is full; may exceed k by the rest of the last chunk)
  bool ended;     // the list ran into an entry that is not real before k were kept
  int64_t read;   // entries read up to: through the k-th kept one, or up to the first that is not real, or n
};

// lane = 0 .. 63; od / oi: the row's k output slots.  Every value returned is wave-uniform.
template <class Source, class Rule>
__device__ __forceinline__ SvWalked sv_list_walk(const Source& src, Rule&& rule, int k, int lane, float* __restrict__ od,
                                                 int64_t* __restrict__ oi) {
  typedef decltype(src.n) pos_t;   // int for the lists of <= 1024 entries, 64 bits for a row's n words
  SvWalked r = {0, false, src.n};
  for (pos_t c = 0; c < src.n && r.kept < k; c += 64) {
    const pos_t j = c + lane;
    int64_t id = -1;
    float dd = INFINITY;
    const bool real = j < src.n && src.get(j, dd, id);
    const uint64_t endm = __builtin_amdgcn_ballot_w64(j < src.n && !real);
    const bool keep = rule(id, real);
    const uint64_t mk = __builtin_amdgcn_ballot_w64(keep);
    const int pos = r.kept + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (keep && pos < k) {
      od[pos] = dd;
      oi[pos] = id;
    }
    r.kept += (int)__popcll(mk);
    if (r.kept >= k) r.read = c + (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(keep && pos == k - 1)) + 1;
    else if (endm) {
      r.read = c + (int)__builtin_ctzll(endm);
      r.ended = true;
      break;
    }
  }
  for (int j = min(r.kept, k) + lane; j < k; j += 64) {
    od[j] = INFINITY;
    oi[j] = -1;
  }
  return r;
}
