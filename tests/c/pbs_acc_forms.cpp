// pbs_acc_forms.cpp -- the integer arithmetic of SET_1's CMUX step in its two forms, on the host (no GPU, no HIP): plain C++ copies of
//   * the step's tail as it was, acc + round(v) with an explicit carry (negacyclic_fft.h: add_rounded<false>), and as the kernels with a NEGATED resident
//     accumulator do it, (-acc) + (-round(v)) with the increment assembled as one 64-bit value from fma(-v, ..) (neg_rounded + add_pairs);
//   * the word the gadget digits are cut from, rot(acc)[j] - acc[j] + off, and its negated-accumulator form (bootstrap_kernels.h: digit_source).
// Checked: new(-acc, -v) == -old(acc, v) mod 2^64 and both against an independent rounding in long double / 128-bit integers, on products at the edges (exact ties
// of both rounding levels, +-0, +-(2^50 - 1), the largest the kernel's bound admits) times accumulators at the edges of both halves, and on random ones.
// Build with -ffp-contract=off (and -fsanitize=address,undefined); run: pbs_acc_forms [random cases, default 10000000].
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const double kMagic = 0x1.8p52, kTwo32 = 0x1p32;
static const double kScale32 = 0x1p-32 / 512.0;   // (2^-64 / M) 2^32 at M = N / 2 = 512
static const long double kScale64 = 1.0L / 512.0L;   // (2^-64 / M) 2^64

static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

// add_rounded<false>: the parent's tail
static uint64_t old_tail(uint64_t acc, double v) {
  const double A = fma(v, kScale32, kMagic);
  const double B = A - kMagic;
  const double q = fma(v, kScale32, -B);
  const double C = fma(q, kTwo32, kMagic);
  const uint64_t a = bits(A), c = bits(C);
  const uint32_t c_lo = (uint32_t)c;
  const uint32_t lo = (uint32_t)acc + c_lo;
  const uint32_t carry = lo < c_lo ? 1u : 0u;
  const uint32_t borrow = 0u - ((uint32_t)(c >> 32) & 1u);
  const uint32_t hi = (uint32_t)(acc >> 32) + (uint32_t)a + borrow + carry;
  return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// neg_rounded + add_pairs: `nv` is what the fmas see behind their source modifier, `nacc` the resident word
static uint64_t new_tail(uint64_t nacc, double nv) {
  const double A = fma(nv, kScale32, kMagic);
  const double B = A - kMagic;
  const double q = fma(nv, kScale32, -B);
  const double C = fma(q, kTwo32, kMagic);
  const uint64_t a = bits(A), c = bits(C);
  const uint32_t hi = (uint32_t)a + (uint32_t)(c >> 32) + (0u - 0x43380000u);
  const uint64_t inc = ((uint64_t)hi << 32) | (uint64_t)(uint32_t)c;
  return nacc + inc;
}

// rint(v 2^-64 / M 2^64) mod 2^64 without the magic number: v / M is exact in long double (64-bit significand), |v / M| < 2^74 fits 128 bits
static uint64_t independent_round(double v) {
  const long double r = rintl((long double)v * kScale64);
  return (uint64_t)(unsigned __int128)(__int128)r;
}

static long failures = 0;
static long checked = 0;

static void check_tail(uint64_t acc, double v) {
  const uint64_t want = old_tail(acc, v);
  const uint64_t got = 0 - new_tail(0 - acc, -v);
  const uint64_t ind = acc + independent_round(v);
  checked++;
  if (want != got || want != ind) {
    if (failures++ < 20)
      printf("TAIL acc %016llx v %a: old %016llx  -new(-acc, -v) %016llx  independent %016llx\n", (unsigned long long)acc, v, (unsigned long long)want,
             (unsigned long long)got, (unsigned long long)ind);
  }
}

// rot_coeff: the staged word, negated where the rotation wraps an odd number of times
static uint64_t rot_word(uint64_t staged, bool neg) { return neg ? (0 - staged) : staged; }

static void check_digits(uint64_t rotated_src, uint64_t home, bool neg, uint64_t off) {
  const uint64_t want = rot_word(rotated_src, neg) - home + off;
  // negated residency: staged and home words are negated, the caller inverts the polarity, the home word is added
  const uint64_t got = rot_word(0 - rotated_src, !neg) + (0 - home) + off;
  checked++;
  if (want != got || ((uint32_t)(want >> 48) ^ 0x8080u) != ((uint32_t)(got >> 48) ^ 0x8080u)) {
    if (failures++ < 20)
      printf("DIGITS src %016llx home %016llx neg %d: %016llx vs %016llx\n", (unsigned long long)rotated_src, (unsigned long long)home, (int)neg,
             (unsigned long long)want, (unsigned long long)got);
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
  const long randoms = argc > 1 ? atol(argv[1]) : 10000000L;
  const uint64_t accs[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull, 0x8000000000000000ull, 0xffffffffffffffffull,
                           0xfffffffeull, 0xffffffff00000000ull, 0x7fffffffffffffffull, 0x00000000ffffffffull + 0x100000000ull};
  const int n_accs = (int)(sizeof(accs) / sizeof(accs[0]));

  // y = v scale 2^32 = f 2^32: the value whose rounding gives the high half.  v = y / scale32 = y 2^41, exact.
  static double ys[4096];
  int n = 0;
  const double ks[] = {0, 1, 2, 3, 4, 5, 255, 256, 65535, 65536, 0x1p31 - 2, 0x1p31 - 1, 0x1p31, 0x1p31 + 1, 0x1p32 - 2, 0x1p32 - 1, 0x1p32, 0x1p32 + 1,
                       0x1p33 - 1, 0x1p40, 0x1p49, 0x1p50 - 2, 0x1p50 - 1, 0x1p50, 0x1p51 - 2, 0x1p51 - 1};
  for (unsigned i = 0; i < sizeof(ks) / sizeof(ks[0]); i++) {
    const double k = ks[i];
    const double cand[] = {k, k + 0.5, k - 0.5, k + 0.25, k + 0.75, k + 0x1p-33, k + 0.5 + 0x1p-33, k + 0.5 - 0x1p-33, k + 0x1p-32, k + 0x1p-31};
    for (unsigned j = 0; j < sizeof(cand) / sizeof(cand[0]); j++) {
      if (fabs(cand[j]) >= 0x1p51) continue;   // the kernel's bound: |f 2^32| < 2^51
      ys[n++] = cand[j];
      ys[n++] = -cand[j];
    }
  }
  // ties of the second level: q 2^32 = m + 1/2, where the significand has room for them (h + (m + 1/2) 2^-32 needs log2 h + 33 bits)
  const double hs[] = {0, 1, 2, 3, 0x1p18, 0x1p19 - 1};
  const double ms[] = {0, 1, 2, 3, 0x1p30, 0x1p31 - 2, 0x1p31 - 1};
  for (unsigned i = 0; i < sizeof(hs) / sizeof(hs[0]); i++)
    for (unsigned j = 0; j < sizeof(ms) / sizeof(ms[0]); j++) {
      const double y = hs[i] + (ms[j] + 0.5) * 0x1p-32;
      ys[n++] = y;
      ys[n++] = -y;
      ys[n++] = hs[i] - (ms[j] + 0.5) * 0x1p-32;
      ys[n++] = -(hs[i] - (ms[j] + 0.5) * 0x1p-32);
    }
  ys[n++] = 0.0;
  ys[n++] = -0.0;
  for (int i = 0; i < n; i++)
    for (int a = 0; a < n_accs; a++) check_tail(accs[a], ys[i] * 0x1p41);
  printf("tail, edges: %d products x %d accumulators\n", n, n_accs);

  for (long i = 0; i < randoms; i++) {
    // a random significand at a random magnitude below the bound 2^83 (2^41 2^51 = 2^92 would be the rounding's own limit; the kernel's products stay below 2^83),
    // every fourth one with a short significand so that ties and exact integers come up
    const uint64_t r = rnd();
    const int e = (int)(rnd() % 84);
    double v = ldexp((double)((r >> 11) | 1ull), e - 53);
    if ((i & 3) == 0) v = ldexp((double)((r >> 40) | 1ull), e - 24);
    if (r & 1) v = -v;
    const uint64_t acc = (i & 7) == 7 ? accs[rnd() % n_accs] : rnd();
    check_tail(acc, v);
  }
  printf("tail, random: %ld\n", randoms);

  // digits: rot - home + off with rot - home at the edges of the offset and of the digit fields (SET_1: l = 2, Bg = 2^8: off = 2^63 + 2^55 + 2^47, digits = bits 48 .. 63)
  const uint64_t off = (1ull << 63) + (1ull << 55) + (1ull << 47);
  const uint64_t diffs[] = {0, 1, off - 1, off, off + 1, (1ull << 47) - 1, 1ull << 47, (1ull << 48) - 1, 1ull << 48, (1ull << 63), ~0ull};
  for (unsigned i = 0; i < sizeof(diffs) / sizeof(diffs[0]); i++)
    for (int s = 0; s < 2; s++)
      for (int a = 0; a < n_accs; a++)
        for (int neg = 0; neg < 2; neg++) {
          const uint64_t d = s ? 0 - diffs[i] : diffs[i];
          const uint64_t home = accs[a], rot = d + home;     // the rotated word the difference asks for ...
          check_digits(neg ? 0 - rot : rot, home, neg != 0, off);   // ... and the staged word it comes from
        }
  for (long i = 0; i < randoms / 10; i++) check_digits(rnd(), (i & 3) ? rnd() : accs[rnd() % n_accs], (rnd() & 1) != 0, off);
  printf("digits: edges and %ld random\n", randoms / 10);

  printf("%ld checks, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
