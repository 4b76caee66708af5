// trace_kernels.h -- device code of mosfhet_hip_tlwe_trace_pack_batch, mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch and mosfhet_hip_trgsw_from_gadget_batch
// (gfx950).  Own code; the functions they stand for: trlwe_packing1_keyswitch_CDKS21 (src/keyswitch.c:526-546), trlwe_RLWE_priv_keyswitch (:65-97) and
// trgsw_from_gadget (:559-572) of the reference.
//
// One kernel, trace_conversions_kernel<F>, with the work named at run time (TraceParams::kind) -- three instantiations, one per ring, for the three calls: the
// library's kernel table is held below a fixed number of instantiations (tests/test_host_and_abi.py).  The bodies share nothing but the transform set-up.
//
//   trace_pack_body<F>             one team (F::THREADS) per LWE sample, all log2 N trace steps inside:
//                                    out = (a', in.b X^0),  a'[0] = in.a[0], a'[N - i] = -in.a[i]
//                                    for j < log2 N:  out += KeySwitch_j(out(X^(N / 2^j + 1)))         (KeySwitch = trlwe_keyswitch: (0, b) - as(a; KS_j))
//                                  The accumulator stays on chip: component a in registers, component b in LDS, as in pbs_ga_kernel.  A step is the permutation of
//                                  ga_eval_automorphism (scatter through LDS, signs by bit N of i gen) -- component a into the staging buffer for the digit words,
//                                  component b ADDED into the accumulator in place (a permutation: every word has one writer) -- then ks_rows_rt on the entry's t
//                                  rows, two inverse transforms, and the rounded pair subtracted from the accumulator.  Every word mod 2^64 equals the sequence
//                                  permute, trlwe_fft_keyswitch_kernel mode 0, add: one chain over rows 0 .. t - 1, the same rounding.
//                                  Key rows come straight from global memory: a set of log2 N entries is 1.4 MiB at N = 2048, t = 4 and every team reads it.
//   rlwe_priv_keyswitch_body<F>
//                                  one team per TRLWE sample, two passes:  out = round(as(in.b; KS1)) - round(as(in.a; KS0)), each pass with an accumulator pair,
//                                  two inverse transforms and a rounding of its own (the two trlwe_keyswitch calls, the negation and the addition of the host
//                                  loop, word for word).  It decomposes in.b, not -in.b: not mode 1 of trlwe_fft_keyswitch_kernel.  In place is fine: a thread
//                                  writes the words it read, after both passes.
//                                  sel != nullptr: team c l + i takes gadget row i of input c and writes rows i (the switched sample) and l + i (the row itself) of
//                                  selector c in the DFT domain, each polynomial exactly as torus_to_dft_kernel transforms the torus words (torus_to_double,
//                                  fft.forward); no torus-domain word is written.  The tail is mode 3's, rolled for the same reason.
// Launch bound 1 like trlwe_fft_keyswitch_kernel: digit words, accumulator and the two product pairs are live together.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "bootstrap_kernels.h"

namespace mosfhet {

template <class F>
__device__ __forceinline__ void trace_pack_body(d2 *xch, uint64_t *acc1, const F &fft, const d2 *__restrict__ key /* entry0 */, const uint64_t *__restrict__ in /*[count][N + 1]*/,
                                                uint64_t *__restrict__ out /*[count][2][N]*/, int t, int base_bit, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS, LOGN = F::LOGM + 1;
  static_assert(F::XCH_SLOTS * sizeof(d2) >= N * sizeof(uint64_t), "the exchange buffer stages one polynomial of torus words");
  const uint64_t *c = in + (size_t)blockIdx.x * (N + 1);
  uint64_t off = 1ull << (63 - t * base_bit);
  for (int i = 0; i < t; i++) off += 1ull << (63 - i * base_bit);
  const RoundCtx scale(0x1p-64 / (double)M);
  const size_t entry_sz = (size_t)t * 2 * M;
  // the LWE mask as the polynomial whose constant term pairs with the key (src/keyswitch.c:530-533); coefficient x = m T + tid resp. M + m T + tid
  uint64_t al[8], ah[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int x = m * T + tid;
    al[m] = x == 0 ? c[0] : 0 - c[N - x];
    ah[m] = 0 - c[M - x];           // coefficient M + x: N - (M + x)
    acc1[x] = x == 0 ? c[N] : 0;
    acc1[M + x] = 0;
  }
  F::sync();
  uint64_t *st = reinterpret_cast<uint64_t *>(xch);
#pragma unroll 1
  for (int j = 0; j < LOGN; j++) {
    const int gen = (N >> j) + 1;
    uint64_t dd_lo[8], dd_hi[8];
    {
      // component a: scatter through the staging buffer, read back in coefficient order, keep only the digit words
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int i0 = (m * T + tid) * gen, i1 = (M + m * T + tid) * gen;
        st[i0 & (N - 1)] = (i0 & N) ? (0 - al[m]) : al[m];
        st[i1 & (N - 1)] = (i1 & N) ? (0 - ah[m]) : ah[m];
      }
      F::sync();
#pragma unroll
      for (int m = 0; m < 8; m++) { dd_lo[m] = st[m * T + tid] + off; dd_hi[m] = st[M + m * T + tid] + off; }
      F::sync();
    }
    {
      // component b: acc1 += acc1(X^gen) in place (read everything, barrier, scatter-add: word (i gen) mod N has this one writer)
      uint64_t v_lo[8], v_hi[8];
#pragma unroll
      for (int m = 0; m < 8; m++) { v_lo[m] = acc1[m * T + tid]; v_hi[m] = acc1[M + m * T + tid]; }
      F::sync();
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int i0 = (m * T + tid) * gen, i1 = (M + m * T + tid) * gen;
        acc1[i0 & (N - 1)] += (i0 & N) ? (0 - v_lo[m]) : v_lo[m];
        acc1[i1 & (N - 1)] += (i1 & N) ? (0 - v_hi[m]) : v_hi[m];
      }
      F::sync();
    }
    double o_re[2][8], o_im[2][8];
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
      for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
    ks_rows_rt<F>(dd_lo, dd_hi, o_re, o_im, xch, fft, key + (size_t)j * entry_sz, t, base_bit, tid);
    fft.inverse(o_re[0], o_im[0], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      al[m] -= round_mod_2_64(o_re[0][m], scale);
      ah[m] -= round_mod_2_64(o_im[0][m], scale);
    }
    fft.inverse(o_re[1], o_im[1], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      acc1[m * T + tid] -= round_mod_2_64(o_re[1][m], scale);
      acc1[M + m * T + tid] -= round_mod_2_64(o_im[1][m], scale);
    }
    F::sync();
  }
  uint64_t *o = out + (size_t)blockIdx.x * (2 * N);
#pragma unroll
  for (int m = 0; m < 8; m++) {
    o[m * T + tid] = al[m];
    o[M + m * T + tid] = ah[m];
    o[N + m * T + tid] = acc1[m * T + tid];
    o[N + M + m * T + tid] = acc1[M + m * T + tid];
  }
}

// ks0: the entry that switches from s_in v, ks1: the one from v (trlwe_new_RLWE_priv_KS_key).  in / out: samples 2N words apart.  sel != nullptr: in = [count][l][2][N],
// sel = [count][2l][2][M] complex, blockIdx.x = c l + i.
template <class F>
__device__ __forceinline__ void rlwe_priv_keyswitch_body(d2 *xch, const F &fft, const d2 *__restrict__ ks0, const d2 *__restrict__ ks1, const uint64_t *in,
                                                         uint64_t *out,   // in place is allowed: no __restrict__
                                                         int t, int base_bit, d2 *__restrict__ sel, int l, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  const uint64_t *c = in + (size_t)blockIdx.x * (2 * N);
  uint64_t off = 1ull << (63 - t * base_bit);
  for (int i = 0; i < t; i++) off += 1ull << (63 - i * base_bit);
  const RoundCtx scale(0x1p-64 / (double)M);
  uint64_t res_a_lo[8], res_a_hi[8], res_b_lo[8], res_b_hi[8];
#pragma unroll
  for (int m = 0; m < 8; m++) { res_a_lo[m] = 0; res_a_hi[m] = 0; res_b_lo[m] = 0; res_b_hi[m] = 0; }
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    // pass 0: - as(in.a; ks0), pass 1: + as(in.b; ks1)
    const d2 *__restrict__ entry = pass ? ks1 : ks0;
    const uint64_t *src = c + pass * N;
    uint64_t dd_lo[8], dd_hi[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { dd_lo[m] = src[m * T + tid] + off; dd_hi[m] = src[M + m * T + tid] + off; }
    double o_re[2][8], o_im[2][8];
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
      for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
    ks_rows_rt<F>(dd_lo, dd_hi, o_re, o_im, xch, fft, entry, t, base_bit, tid);
    fft.inverse(o_re[0], o_im[0], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const uint64_t lo = round_mod_2_64(o_re[0][m], scale), hi = round_mod_2_64(o_im[0][m], scale);
      res_a_lo[m] = pass ? res_a_lo[m] + lo : 0 - lo;
      res_a_hi[m] = pass ? res_a_hi[m] + hi : 0 - hi;
    }
    fft.inverse(o_re[1], o_im[1], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const uint64_t lo = round_mod_2_64(o_re[1][m], scale), hi = round_mod_2_64(o_im[1][m], scale);
      res_b_lo[m] = pass ? res_b_lo[m] + lo : 0 - lo;
      res_b_hi[m] = pass ? res_b_hi[m] + hi : 0 - hi;
    }
  }
  if (sel) {
    const size_t row = (size_t)2 * M;
    const unsigned ct = blockIdx.x / (unsigned)l, i = blockIdx.x % (unsigned)l;
    d2 *row_a = sel + ((size_t)ct * 2 * l + i) * row, *row_b = row_a + (size_t)l * row;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {   // res.a, res.b, in.a, in.b -- one rolled body (trlwe_fft_keyswitch_kernel mode 3)
      double re[8], im[8];
      if (q >= 2) {
        const uint64_t *src = c + (q - 2) * N;
#pragma unroll
        for (int m = 0; m < 8; m++) { re[m] = torus_to_double(src[m * T + tid]); im[m] = torus_to_double(src[M + m * T + tid]); }
      } else {
#pragma unroll
        for (int m = 0; m < 8; m++) { re[m] = torus_to_double(q ? res_b_lo[m] : res_a_lo[m]); im[m] = torus_to_double(q ? res_b_hi[m] : res_a_hi[m]); }
      }
      fft.forward(re, im, xch, tid);
      d2 *dst = (q < 2 ? row_a : row_b) + (q & 1) * M;
#pragma unroll
      for (int m = 0; m < 8; m++) dst[m * T + tid] = d2{re[m], im[m]};
    }
  } else {
    uint64_t *o = out + (size_t)blockIdx.x * (2 * N);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      o[m * T + tid] = res_a_lo[m];
      o[M + m * T + tid] = res_a_hi[m];
      o[N + m * T + tid] = res_b_lo[m];
      o[N + M + m * T + tid] = res_b_hi[m];
    }
  }
}

enum { TRACE_KIND_PACK = 0, TRACE_KIND_PRIV = 1, TRACE_KIND_GADGET = 2 };

struct TraceParams {
  const d2 *__restrict__ key;   // the first entry the call uses: [log2 N or 2][t][2][M] complex
  const d2 *__restrict__ tw;
  const uint64_t *in;           // kind 0: [count][N + 1]; 1: [count][2][N]; 2: [count][l][2][N]
  uint64_t *out;                // kind 0, 1: [count][2][N] (kind 1: may be `in`)
  d2 *sel;                      // kind 2: [count][2l][2][M] complex
  int kind, t, base_bit, l;
};

template <class F>
__global__ __launch_bounds__(F::THREADS, 1) void trace_conversions_kernel(TraceParams p) {
  __shared__ __attribute__((aligned(16))) d2 xch[F::XCH_SLOTS];
  __shared__ __attribute__((aligned(16))) uint64_t acc1[F::N];   // the trace's component b (kind 0)
  const int tid = threadIdx.x;
  F fft;
  fft.init(p.tw, tid);
  if (p.kind == TRACE_KIND_PACK) trace_pack_body<F>(xch, acc1, fft, p.key, p.in, p.out, p.t, p.base_bit, tid);
  else rlwe_priv_keyswitch_body<F>(xch, fft, p.key, p.key + (size_t)p.t * 2 * F::M, p.in, p.out, p.t, p.base_bit, p.kind == TRACE_KIND_GADGET ? p.sel : nullptr, p.l, tid);
}

}  // namespace mosfhet
