// cmux_steps.h -- the small steps every CMUX / external-product kernel shares, each defined ONCE: the bit-exactness of every call family against the oracle
// rests on these being the same everywhere.  All of them inline to the expression they replace (tools/kernel_listing_diff.py shows that a change here left
// every kernel's instructions alone, or which kernels it reached).
#pragma once
#include "negacyclic_fft.h"

namespace mosfhet {

// src/misc.c:18-22 with log_scale = log2(2N)
template <int LOG2N>
__device__ __forceinline__ uint32_t modswitch(uint64_t x) {
  return (uint32_t)((x + (1ull << (63 - LOG2N))) >> (64 - LOG2N));
}

// src/bootstrap.c:213-217 (P: PbsParams or any parameter block with its pre / kappa / theta)
template <class P>
__device__ __forceinline__ uint64_t pbs_pre(uint64_t x, const P &p, int log2N2) {
  if (!p.pre) return x;
  const uint64_t rnd = 1ull << (64 - log2N2 + p.theta - 1);
  const uint64_t msk = ~((1ull << (64 - log2N2 + p.theta)) - 1);
  return ((x << p.kappa) + rnd) & msk;
}

// A rotation amount a in [0, 2N) as X^a = (-1)^flip X^a_lo, a_lo in [0, N).
struct Rotation {
  int a_lo;
  bool flip;
};
__device__ __forceinline__ Rotation split_rotation(int a, int N) { return Rotation{a & (N - 1), (a & N) != 0}; }
// the first rotation of a bootstrap, X^(2N - bbar) from the switched body word (src/bootstrap.c:194-195)
__device__ __forceinline__ Rotation first_rotation(uint32_t bbar, int N) { return split_rotation((2 * N - (int)bbar) & (2 * N - 1), N); }

// coefficient i of poly * X^a  (a in [0, 2N)), poly in LDS/global; src/polynomial.c:184-199
template <int N>
__device__ __forceinline__ uint64_t rot_coeff(const uint64_t *poly, int i, int a_lo, bool flip) {
  const int src = i - a_lo;
  const bool neg = (src < 0) != flip;
  const uint64_t v = poly[src & (N - 1)];
  return neg ? (0 - v) : v;
}

// coefficient j of the mask of trlwe_extract_tlwe(., 0) from component a (src/trlwe.c:540-552 at idx = 0)
__device__ __forceinline__ uint64_t extract0_coeff(const uint64_t *a, int j, int N) { return j == 0 ? a[0] : 0 - a[N - j]; }

// The offset of a signed decomposition into l digits of bg bits (src/polynomial.c:74-89): half a unit of the last digit, so that cutting the word at bit
// 64 - l bg rounds, plus half a digit range per level, so that every digit is read as an unsigned field and re-centred.  The key switches' t digits of base_bit
// bits are the same formula.  A macro (a statement expression) and not a function: an inlined function is optimised on its own first, and with a run-time
// digit count or digit width its callers then compile to different, if equivalent, code (113 of 329 kernels: another order of the sum, inverted branches and
// with them another register allocation); as text in the kernel every listing stays what it was.
#define GADGET_OFFSET(l, bg)                                             \
  ({                                                                     \
    uint64_t off_ = 1ull << (63 - (l) * (bg));                           \
    for (int i_ = 0; i_ < (l); i_++) off_ += 1ull << (63 - i_ * (bg));   \
    off_;                                                                \
  })

// o += (re + i im) k: THE complex multiply-accumulate, the one place that fixes the order of its four fmas -- that of orc_dft_mul_addto (oracle/oracle_fft.c;
// src/polynomial.c:406-426).  The order decides the bits.
__device__ __forceinline__ void cmac(double &o_re, double &o_im, double re, double im, const d2 &k) {
  o_re = __builtin_fma(-im, k.y, __builtin_fma(re, k.x, o_re));
  o_im = __builtin_fma(im, k.x, __builtin_fma(re, k.y, o_im));
}
// (the accumulator as one complex value: a vector's elements cannot be bound to references)
__device__ __forceinline__ void cmac(d2 &o, double re, double im, const d2 &k) {
  double o_re = o.x, o_im = o.y;
  cmac(o_re, o_im, re, im, k);
  o = d2{o_re, o_im};
}

template <int X>
struct kCeilLog2 { static constexpr int value = X <= 1 ? 0 : 1 + kCeilLog2<(X + 1) / 2>::value; };
template <>
struct kCeilLog2<1> { static constexpr int value = 0; };

// Does the rounding of an external product's output need its reduction mod 1 in front (add_rounded<REDUCE>)?  Every output is a sum of 2L * N products
// digit * key coefficient with |digit| <= 2^(BG-1) and |key| <= 2^63 (the key is (double)(int64_t) of torus words): |sum| <= 2^(ceil log2(2L) + log2 N + BG - 1 + 63).
// Below 2^83 it does not; that holds for SET_1's 2 x 2^8 gadget at N = 1024 (2^82) and is decided at compile time (a run-time gadget, BG = 0, always reduces).
template <class F, int L, int BG>
constexpr bool kProductNeedsReduce = !(BG > 0 && kCeilLog2<2 * L>::value + (F::LOGM + 1) + BG - 1 + 63 < 83);

// the rounding context of a ring of N = 2M coefficients: the inverse transform's 1 / M and the torus scale 2^-64 in one factor
template <int M>
__device__ __forceinline__ RoundCtx round_scale() {
  return RoundCtx(0x1p-64 / (double)M);
}

}  // namespace mosfhet
