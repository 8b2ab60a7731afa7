// The (distance, id) word of the exact search paths on the CPU: csrc/key_word.h compiled by the host compiler (no HIP), checked over
// a table of floats and list lengths.  Prints one line: "keys <n> order pairs <n> words <n> np2 cases <n> failures <n>".
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "key_word.h"

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static long failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      fprintf(stderr, "FAIL " __VA_ARGS__); \
      fprintf(stderr, "\n");              \
    }                                     \
  } while (0)

int main() {
  // ascending as real numbers; -0 and +0 are equal as floats and adjacent here
  const float table[] = {-INFINITY,
                         -FLT_MAX,
                         -1.f,
                         -FLT_MIN,
                         -from_bits(0x007fffffu),   // largest denormal
                         -from_bits(0x00000001u),   // smallest denormal
                         -0.f,
                         0.f,
                         from_bits(0x00000001u),
                         from_bits(0x007fffffu),
                         FLT_MIN,
                         1.f,
                         from_bits(0x3f800001u),    // the float after 1
                         FLT_MAX,
                         INFINITY};
  const int nt = (int)(sizeof(table) / sizeof(table[0]));
  long keys = 0, pairs = 0, words = 0, np2_cases = 0;

  // key round trip: the bits of x come back
  for (int i = 0; i < nt; ++i, ++keys)
    CHECK(bits(key2f_(f2key_(table[i]))) == bits(table[i]), "round trip of %a: %08x -> %08x", table[i], bits(table[i]),
          bits(key2f_(f2key_(table[i]))));
  // key order: x < y => key(x) < key(y); the map orders by sign and magnitude, so it also puts -0 strictly below +0 (equal as floats)
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nt; ++j, ++pairs) {
      if (table[i] < table[j]) CHECK(f2key_(table[i]) < f2key_(table[j]), "order of %a, %a", table[i], table[j]);
      if (i < j) CHECK(f2key_(table[i]) < f2key_(table[j]), "table order of %a, %a", table[i], table[j]);   // (includes -0 < +0)
    }
  CHECK(f2key_(-0.f) + 1u == f2key_(0.f), "-0 is the key just below +0: %08x %08x", f2key_(-0.f), f2key_(0.f));

  // words: (distance, then id) order, never the empty word for a finite distance, both halves come back
  const uint32_t ids[] = {0u, 1u, 0xffffffffu};
  for (int i = 0; i < nt; ++i)
    for (int a = 0; a < 3; ++a) {
      const uint64_t w = sv_word(table[i], ids[a]);
      ++words;
      CHECK(bits(sv_word_d2(w)) == bits(table[i]) && sv_word_id(w) == (int64_t)ids[a], "unpack of (%a, %u)", table[i], ids[a]);
      CHECK(w == sv_word_key(f2key_(table[i]), ids[a]), "sv_word is sv_word_key of the key");
      if (isfinite(table[i])) CHECK(w != SV_WORD_NONE, "(%a, %u) packs to the empty word", table[i], ids[a]);
      for (int j = 0; j < nt; ++j)
        for (int b = 0; b < 3; ++b) {
          const uint64_t x = sv_word(table[j], ids[b]);
          const bool less = i < j || (i == j && ids[a] < ids[b]);   // (table order = key order, checked above)
          CHECK((w < x) == less, "word order of (%a, %u), (%a, %u)", table[i], ids[a], table[j], ids[b]);
        }
    }
  CHECK(SV_WORD_NONE == 0xffffffffffffffffull, "the empty word is all ones");

  // sort length: 2 for n = 0, 1, 2; else the least power of two >= n -- at the powers up to 2^20 and their neighbours
  for (int n = 0; n <= 2; ++n, ++np2_cases) CHECK(sv_np2(n) == 2, "sv_np2(%d) = %d", n, sv_np2(n));
  for (int e = 2; e <= 20; ++e)
    for (int dn = -1; dn <= 1; ++dn, ++np2_cases) {
      const int n = (1 << e) + dn, p = sv_np2(n);
      CHECK((p & (p - 1)) == 0 && p >= n && p / 2 < n, "sv_np2(%d) = %d", n, p);
      CHECK(p == (dn <= 0 ? (1 << e) : (2 << e)), "sv_np2(%d) = %d", n, p);
    }
  printf("keys %ld order pairs %ld words %ld np2 cases %ld failures %ld\n", keys, pairs, words, np2_cases, failures);
  return failures ? 1 : 0;
}
