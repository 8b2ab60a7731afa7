// The word every exact path of the search orders by, its only definition: (f2key_(d2) << 32) | id compares as (distance, id),
// all ones means "no entry".  Plain C++ (nothing but <stdint.h>): knn_dev.h includes it for the kernels and the launchers,
// tests/key_word_main.cpp runs it on the CPU.
//
//   f2key_, key2f_            the order-preserving float <-> key map: x < y  =>  f2key_(x) < f2key_(y), -0 below +0
//   sv_word_key, sv_word      pack a key / a distance with an id;  SV_WORD_NONE: the empty word (no finite distance packs to it)
//   sv_word_d2, sv_word_id    unpack
//   sv_np2                    the sort length of an n-entry list: the smallest power of two >= n, at least 2
#pragma once
#include <stdint.h>

// (under hipcc the includer has the HIP runtime header in front of this one: knn_dev.h)
#if defined(__HIPCC__)
#define SV_KEY_FN __host__ __device__ __forceinline__
#else
#define SV_KEY_FN inline
#endif

SV_KEY_FN uint32_t f2key_(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SV_KEY_FN float key2f_(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __builtin_bit_cast(float, u);
}

constexpr uint64_t SV_WORD_NONE = ~0ull;
SV_KEY_FN uint64_t sv_word_key(uint32_t key, uint32_t id) { return ((uint64_t)key << 32) | id; }
SV_KEY_FN uint64_t sv_word(float d2, uint32_t id) { return sv_word_key(f2key_(d2), id); }
SV_KEY_FN float sv_word_d2(uint64_t w) { return key2f_((uint32_t)(w >> 32)); }
SV_KEY_FN int64_t sv_word_id(uint64_t w) { return (int64_t)(uint32_t)w; }

SV_KEY_FN int sv_np2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

#undef SV_KEY_FN
