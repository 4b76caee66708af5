// pbs_sign_forms.cpp -- the gadget digits of SET_1's CMUX step (N = 1024, l = 2, Bg = 2^8, negated resident accumulators) in their two integer forms, on the
// host (no GPU, no HIP): plain C++ copies of
//   * the form as it was (cmux_steps.h: rot_coeff; bootstrap_kernels.h: digit_source<.., NEG>, Digits<2, 8>::pack and digit): a compare for the rotation's sign, a conditional
//     64-bit negate, the home word and the offset added, the top 16 bits flipped by 0x8080 and cut by signed bit-field extracts;
//   * the sign-free form (cmux_digits<.., SF>, digit_source_hi, Digits<2, 8, RAW>): sign and index from ONE 11-bit subtraction, the sign applied by two XORs around
//     one carry-free 64-bit add, the high dword kept raw and digit lv taken as (byte 3 - lv) - 128;
//   * the reference's own formula on the plain accumulator (src/polynomial.c:74-89 on rot(acc)[j] - acc[j]).
// Checked, both digits of every coefficient: all 2048 rotations x all 1024 positions on polynomials of edge words; edge words that put (+-v) + h + off on both
// sides of every boundary (rounding bit 47 against low bits all zero / all ones, each byte field at 0x00 / 0x7f / 0x80 / 0xff, the low-dword add carrying and not,
// v and h at 0, 1, 2^32 - 1, 2^32, 2^63, 2^64 - 1) under both signs; and random triples.
// Build with -fsanitize=address,undefined; run: pbs_sign_forms [random triples, default 4000000].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static const int N = 1024, M = 512;
static const uint64_t kOff = (1ull << 63) + (1ull << 55) + (1ull << 47);

static long failures = 0;
static long checked = 0;

static int sbfe(uint32_t x, int pos, int width) {   // signed bit-field extract
  const uint32_t f = (x >> pos) & ((1u << width) - 1u);
  return (int)f - (int)((f >> (width - 1)) << width);
}

// ---- the form as it was: `staged` is the word read from the rotated position of -acc, `home` is -acc[j], `neg` what rot_coeff decides
static void old_sign_index(int j, int a_lo, bool flip, int *idx, bool *neg) {
  const int src = j - a_lo;
  *neg = (src < 0) != flip;
  *idx = src & (N - 1);
}
static void old_digits(uint64_t staged, uint64_t home, bool neg, int d[2]) {
  const uint64_t rotated = neg ? (0 - staged) : staged;
  const uint64_t dd = rotated + home + kOff;
  const uint32_t w = (uint32_t)(dd >> 48) ^ 0x8080u;
  d[0] = sbfe(w, 8, 8);
  d[1] = sbfe(w, 0, 8);
}

// ---- the sign-free form
static void new_sign_index(int j, int a_lo, bool flip, int *idx, uint32_t *mask) {
  const int abar2 = a_lo + (flip ? N : 0);
  const uint32_t s = (uint32_t)j - (uint32_t)abar2;
  *idx = (int)(s & (uint32_t)(N - 1));
  *mask = 0u - ((s >> 10) & 1u);   // v_bfe_i32 s, 10, 1
}
static void new_digits(uint64_t staged, uint64_t home, uint32_t mask, int d[2]) {
  const uint64_t wide = ((uint64_t)mask << 32) | mask;
  const uint64_t y = staged + (home ^ wide);                              // v_xor_b32 x 2, v_lshl_add_u64
  const uint32_t hi = ((uint32_t)(y >> 32) ^ mask) + (uint32_t)(kOff >> 32);   // v_xad_u32
  d[0] = (int)((hi >> 24) & 255u) - 128;
  d[1] = (int)((hi >> 16) & 255u) - 128;
}

// ---- the reference on the plain accumulator: acc X^abar - acc at coefficient j, then src/polynomial.c:74-89
static void ref_digits(const uint64_t *acc, int j, int abar, int d[2]) {
  const int a_lo = abar & (N - 1);
  const int src = j - a_lo;
  const bool neg = (src < 0) != ((abar & N) != 0);
  const uint64_t v = acc[src & (N - 1)];
  const uint64_t dd = (neg ? (0 - v) : v) - acc[j] + kOff;
  for (int lv = 0; lv < 2; lv++) d[lv] = (int)((dd >> (64 - (lv + 1) * 8)) & 255u) - 128;
}

static void check_words(uint64_t staged, uint64_t home, bool neg, const char *what) {
  int a[2], b[2];
  old_digits(staged, home, neg, a);
  new_digits(staged, home, neg ? ~0u : 0u, b);
  checked++;
  if (a[0] != b[0] || a[1] != b[1]) {
    if (failures++ < 20)
      printf("%s staged %016llx home %016llx neg %d: digits %d %d vs %d %d\n", what, (unsigned long long)staged, (unsigned long long)home, (int)neg, a[0], a[1], b[0],
             b[1]);
  }
}

static uint64_t rng_state = 0x4D4F5346ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char **argv) {
  const long randoms = argc > 1 ? atol(argv[1]) : 4000000L;
  const uint64_t edges[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull, 0x8000000000000000ull, 0xffffffffffffffffull};
  const int n_edges = (int)(sizeof(edges) / sizeof(edges[0]));

  // (1) every rotation x every position: sign and index, and the digits of polynomials whose words are edge words and digit-field boundaries
  uint64_t *acc = (uint64_t *)malloc(sizeof(uint64_t) * N), *nacc = (uint64_t *)malloc(sizeof(uint64_t) * N);
  if (!acc || !nacc) return 2;
  for (int abar = 0; abar < 2 * N; abar++) {
    for (int i = 0; i < N; i++) {
      const int k = (i * 7 + abar) % (n_edges + 4);
      acc[i] = k < n_edges ? edges[k] : (rnd() & 0xffff000000000000ull) + (k & 1 ? 0x0000ffffffffffffull : 0) + (k & 2 ? 0x0000800000000000ull : 0);
      nacc[i] = 0 - acc[i];
    }
    const int a_lo = abar & (N - 1);
    const bool flip = ((abar & N) != 0) != true;   // pbs_body.inc: inverted, since what is rotated is -acc
    for (int j = 0; j < N; j++) {
      int i_old, i_new, a[2], b[2], r[2];
      bool neg;
      uint32_t mask;
      old_sign_index(j, a_lo, flip, &i_old, &neg);
      new_sign_index(j, a_lo, flip, &i_new, &mask);
      old_digits(nacc[i_old], nacc[j], neg, a);
      new_digits(nacc[i_new], nacc[j], mask, b);
      ref_digits(acc, j, abar, r);
      checked++;
      if (i_old != i_new || mask != (neg ? ~0u : 0u) || a[0] != b[0] || a[1] != b[1] || a[0] != r[0] || a[1] != r[1]) {
        if (failures++ < 20)
          printf("ROTATION abar %d j %d: index %d vs %d, neg %d mask %08x, digits old %d %d new %d %d reference %d %d\n", abar, j, i_old, i_new, (int)neg, mask, a[0],
                 a[1], b[0], b[1], r[0], r[1]);
      }
    }
    // the other polarity as well (the identity of sign and index holds for both flips; the kernels' first rotation of the test vector passes either)
    for (int j = 0; j < N; j++) {
      int i_old, i_new;
      bool neg;
      uint32_t mask;
      old_sign_index(j, a_lo, !flip, &i_old, &neg);
      new_sign_index(j, a_lo, !flip, &i_new, &mask);
      checked++;
      if (i_old != i_new || mask != (neg ? ~0u : 0u)) {
        if (failures++ < 20) printf("ROTATION (other flip) abar %d j %d: index %d vs %d, neg %d mask %08x\n", abar, j, i_old, i_new, (int)neg, mask);
      }
    }
  }
  free(acc);
  free(nacc);
  printf("rotations: %d x %d positions, both polarities\n", 2 * N, N);
  (void)M;

  // (2) words at the boundaries: the word the digits are cut from, W = (+-v) + h + off, is chosen; one of v, h is an edge word, the other follows
  const uint32_t fields[] = {0x00u, 0x7fu, 0x80u, 0xffu};
  const uint64_t lows[] = {0ull, 1ull, 0x00007fffffffffffull, 0x0000800000000000ull, 0x0000ffffffffffffull, 0x00000000ffffffffull, 0x0000000100000000ull,
                           0x0000ffff00000000ull};
  long edge_cases = 0;
  for (int f0 = 0; f0 < 4; f0++)
    for (int f1 = 0; f1 < 4; f1++)
      for (unsigned lo = 0; lo < sizeof(lows) / sizeof(lows[0]); lo++) {
        const uint64_t W = ((uint64_t)fields[f0] << 56) | ((uint64_t)fields[f1] << 48) | lows[lo];
        for (int delta = -1; delta <= 1; delta++) {      // ... and one word to either side of it
          const uint64_t sum = W + (uint64_t)(int64_t)delta - kOff;   // (+-v) + h
          for (int e = 0; e < n_edges; e++)
            for (int neg = 0; neg < 2; neg++) {
              const uint64_t h = edges[e], pv = sum - h;    // h an edge word
              check_words(neg ? 0 - pv : pv, h, neg != 0, "EDGE(h)");
              const uint64_t v = edges[e], h2 = sum - (neg ? 0 - v : v);   // v an edge word
              check_words(v, h2, neg != 0, "EDGE(v)");
              edge_cases += 2;
            }
        }
      }
  // the low-dword add v.lo + (h ^ M).lo carrying and not carrying, with every pair of edge words
  for (int a = 0; a < n_edges; a++)
    for (int b = 0; b < n_edges; b++)
      for (int neg = 0; neg < 2; neg++) {
        check_words(edges[a], edges[b], neg != 0, "PAIR");
        check_words(edges[a] + 0xfffffffeull, edges[b] + 1ull, neg != 0, "PAIR");
        check_words(edges[a] + 0xfffffffeull, edges[b] + 2ull, neg != 0, "PAIR");
        edge_cases += 3;
      }
  printf("boundary words: %ld\n", edge_cases);

  // (3) random triples (staged word, home word, sign); every fourth with an edge word
  for (long i = 0; i < randoms; i++) {
    const uint64_t r = rnd();
    const uint64_t v = (i & 3) == 1 ? edges[r % n_edges] : rnd(), h = (i & 3) == 3 ? edges[(r >> 8) % n_edges] : rnd();
    check_words(v, h, (r >> 63) != 0, "RANDOM");
  }
  printf("random triples: %ld\n", randoms);

  printf("%ld checks, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
