// trace_kernels.h -- device code of mosfhet_hip_tlwe_trace_pack_batch, mosfhet_hip_tlwe_trace_pack_many_batch, mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch and
// mosfhet_hip_trgsw_from_gadget_batch (gfx950).  Own code; the functions they stand for: trlwe_packing1_keyswitch_CDKS21 (src/keyswitch.c:526-546), trlwe_RLWE_priv_keyswitch (:65-97) and
// trgsw_from_gadget (:559-572) of the reference.
//
// One kernel, trace_conversions_kernel<F>, with the work named at run time (TraceParams::kind) -- three instantiations, one per ring, for the four calls: the
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
//                                  kind 3 (mosfhet_hip_tlwe_trace_pack_many_batch; include/mosfhet_hip.h has the definition): the same body with another prologue and
//                                  fewer steps -- one team per MERGE of the packing tree.  Merge r of output o at level lvl loads E = P[r] and O = X^(N / 2^lvl)
//                                  P[r + n / 2^lvl] (at level 1 embedded straight from the two LWE samples), keeps U = E + O as the accumulator and runs one step
//                                  whose switched operand is V = E - O, with generator 2^lvl + 1 and entry log2 N - lvl (trace_step<F, true>: the step of the trace
//                                  with "kept" and "switched" apart).  The last level's teams go on with trace steps 0 .. log2 N - L - 1 on chip.
//   rlwe_priv_keyswitch_body<F>
//                                  one team per TRLWE sample, two passes:  out = round(as(in.b; KS1)) - round(as(in.a; KS0)), each pass with an accumulator pair,
//                                  two inverse transforms and a rounding of its own (the two trlwe_keyswitch calls, the negation and the addition of the host
//                                  loop, word for word).  It decomposes in.b, not -in.b: not mode 1 of trlwe_fft_keyswitch_kernel.  In place is fine: a thread
//                                  writes the words it read, after both passes.
//                                  sel != nullptr: team c l + i takes gadget row i of input c and writes rows i (the switched sample) and l + i (the row itself) of
//                                  selector c in the DFT domain, each polynomial exactly as torus_to_dft_kernel transforms the torus words (torus_to_double,
//                                  fft.forward); no torus-domain word is written.  The tail is mode 3's, rolled for the same reason.
//   polylinear_body<F>           kind 4 (mosfhet_hip_trlwe_linear_batch / _extract_batch; trlwe_DFT_mul_by_polynomial / trlwe_DFT_mul_addto_by_polynomial, src/trlwe.c:491-505,
//                                  trlwe_from_DFT and trlwe_extract_tlwe :540-552): one team per (batch element b, output row j).  The inputs were transformed by
//                                  torus_to_dft_kernel into the pool, the weight polynomials at creation, both in slot order: the team walks row j's entries in the
//                                  stored order, loads the two input components and the weight row 16 bytes per lane, and accumulates the pair in registers with the
//                                  two-FMA complex multiply-add of ks_rows_rt (input first, weight second); then two inverse transforms, the general rounding, the
//                                  bias, and either the TRLWE sample or the extracted LWE row written straight from the registers.  It has no LDS exchange of its
//                                  own: the only barriers are the inverse transforms'.  It lives here because this kernel already holds what it needs -- row
//                                  multiply-accumulate from global memory, the two inverse transforms, the general rounding -- and its register need (two
//                                  accumulator pairs and three operands) is below the other kinds': the kernel's allocation does not move.
//   gsw_digits_body<F>,          kinds 5 and 6 (mosfhet_hip_trlwe_gsw_linear_batch / _extract_batch; sums of trgsw_mul_trlwe_DFT, src/trgsw.c:385-423, with ONE rounding, then
//   gsw_sum_body<F>                trlwe_from_DFT / trlwe_extract_tlwe): the layer of kind 4 with the operands' roles exchanged -- the weights are TRGSW_DFT samples
//                                  [2l][2][M], the input is decomposed.  Kind 5, one team per (batch element, input sample): the 2N words plus the gadget offset,
//                                  then per component and level the digit polynomial formed as ks_rows_rt forms it, fft.forward, and the M complex values stored 16
//                                  bytes per lane into the pool [b][rows_in][2l][M] -- every digit transform is made once and read by all rows_out teams.  Kind 6, one
//                                  team per (batch element, output row): per entry and row r < 2l the digit transform and the two halves of weight row r, 16 bytes
//                                  per lane, two cmacs per point (digit first, row second) into the accumulator pair; then polylinear_finish, the tail kind 4 runs.
//                                  Registers: kind 5 holds one component's digit words and one transform, kind 6 two accumulator pairs and three operand rows --
//                                  what kind 4 holds.
//   sel_gate_body<F>             kind 7 (mosfhet_hip_trgsw_logic_batch; trgsw_mul_DFT2, src/trgsw.c:425-442, and its ring combinations): one team per (batch element,
//                                  gate of the level, row r) -- the row of X (and Y) back to torus words, the external product of that row with the right operand
//                                  as ks_rows_rt forms it, the op's integer combination, and the forward tail of kind 2.  No torus-domain word is written.
// Launch bound 1 like trlwe_fft_keyswitch_kernel: digit words, accumulator and the two product pairs are live together.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "bootstrap_kernels.h"

namespace mosfhet {

enum { TRACE_KIND_PACK = 0, TRACE_KIND_PRIV = 1, TRACE_KIND_GADGET = 2, TRACE_KIND_MANY = 3, TRACE_KIND_POLYLINEAR = 4, TRACE_KIND_GSW_DIGITS = 5,
       TRACE_KIND_GSW_SUM = 6, TRACE_KIND_SEL_GATE = 7 };

struct TraceParams {
  const d2 *__restrict__ key;   // the first entry the call uses: [log2 N or 2][t][2][M] complex
  const d2 *__restrict__ tw;
  const uint64_t *in;           // kind 0: [count][N + 1]; 1: [count][2][N]; 2: [count][l][2][N]; 3: level 1: the LWE samples of the round [total][N + 1], level > 1: the
                                // results of the level before [outputs][2 cnt][2][N]
  uint64_t *out;                // kind 0, 1: [count][2][N] (kind 1: may be `in`); 3: [outputs][cnt][2][N]
  d2 *sel;                      // kind 2: [count][2l][2][M] complex
  int kind, t, base_bit, l;
  int lvl, cnt_log, tail, total;   // kind 3: merge level (>= 1), log2 of the results per output it writes (cnt = n / 2^lvl), trace steps behind the merge (last level only),
                                   // samples `in` holds at level 1 (a sample index >= total stands for the all-zero sample)
  // kind 4: key = the weight polynomials [entries][M] complex, out = [teams][2][N] or, idx >= 0, [teams][N + 1]
  const d2 *__restrict__ xin;        // the transformed inputs of the round [count][rows_in][2][M] complex
  const int *__restrict__ row_ptr;   // [rows_out + 1]
  const int *__restrict__ col;       // [entries]
  const uint64_t *__restrict__ bias; // [rows_out][N] or null
  int rows_out, rows_in, idx;        // idx < 0: the TRLWE sample; else trlwe_extract_tlwe(., idx)
  // kind 5: in = the inputs of the round [count][rows_in][2][N], sel = the pool [count][rows_in][2l][M] complex, (l, base_bit) = the gadget
  // kind 6: key = the weights [entries][2l][2][M] complex, xin = the pool, l; row_ptr, col, bias, rows_out, rows_in, idx, out as kind 4
  // kind 7: xin = the input selectors of the launch [count][rows_in][2l][2][M] complex, sel = every gate's output [count][rows_out][2l][2][M] complex, row_ptr = the
  //         level's SelGate records, idx = gates of the level, (l, base_bit) = the gadget
};

// One step on the accumulator (a in al / ah, b in acc1):  acc += KeySwitch_entry(v(X^gen)).  The permutation of ga_eval_automorphism (scatter through LDS, signs by bit N
// of i gen): v.a into the staging buffer for the digit words, v.b ADDED into acc1 in place (a permutation: every word has one writer); then ks_rows_rt on the entry's t
// rows, two inverse transforms, and the rounded pair subtracted from the accumulator.  MERGE = false: v is the accumulator itself (va_* alias al / ah, v.b is read from
// acc1) -- the trace step.  MERGE = true: v = (va, vb) in registers and the accumulator holds the kept operand -- a merge of the packing tree.
template <class F, bool MERGE>
__device__ __forceinline__ void trace_step(uint64_t (&al)[8], uint64_t (&ah)[8], uint64_t *acc1, const uint64_t (&va_lo)[8], const uint64_t (&va_hi)[8],
                                           const uint64_t (&vb_lo)[8], const uint64_t (&vb_hi)[8], int gen, d2 *xch, const F &fft, const d2 *__restrict__ entry, int t,
                                           int base_bit, uint64_t off, const RoundCtx &scale, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  uint64_t *st = reinterpret_cast<uint64_t *>(xch);
  uint64_t dd_lo[8], dd_hi[8];
  {
    // component a: scatter through the staging buffer, read back in coefficient order, keep only the digit words
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int i0 = (m * T + tid) * gen, i1 = (M + m * T + tid) * gen;
      st[i0 & (N - 1)] = (i0 & N) ? (0 - va_lo[m]) : va_lo[m];
      st[i1 & (N - 1)] = (i1 & N) ? (0 - va_hi[m]) : va_hi[m];
    }
    F::sync();
#pragma unroll
    for (int m = 0; m < 8; m++) { dd_lo[m] = st[m * T + tid] + off; dd_hi[m] = st[M + m * T + tid] + off; }
    F::sync();
  }
  {
    // component b: acc1 += v.b(X^gen) in place (the trace step: read everything, barrier; then scatter-add: word (i gen) mod N has this one writer)
    uint64_t v_lo[8], v_hi[8];
    if constexpr (MERGE) {
#pragma unroll
      for (int m = 0; m < 8; m++) { v_lo[m] = vb_lo[m]; v_hi[m] = vb_hi[m]; }
    } else {
#pragma unroll
      for (int m = 0; m < 8; m++) { v_lo[m] = acc1[m * T + tid]; v_hi[m] = acc1[M + m * T + tid]; }
      F::sync();
    }
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
  ks_rows_rt<F>(dd_lo, dd_hi, o_re, o_im, xch, fft, entry, t, base_bit, tid);
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

// prologue (kind 0: embed | kind 3: merge) + trace steps 0 .. steps - 1
template <class F>
__device__ __forceinline__ void trace_pack_body(d2 *xch, uint64_t *acc1, const F &fft, const TraceParams &p, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS, LOGN = F::LOGM + 1;
  static_assert(F::XCH_SLOTS * sizeof(d2) >= N * sizeof(uint64_t), "the exchange buffer stages one polynomial of torus words");
  const int t = p.t, base_bit = p.base_bit;
  const uint64_t off = GADGET_OFFSET(t, base_bit);
  const RoundCtx scale = round_scale<M>();
  const size_t entry_sz = (size_t)t * 2 * M;
  uint64_t al[8], ah[8];   // component a, coefficient x = m T + tid resp. M + m T + tid
  int steps = LOGN;
  if (p.kind == TRACE_KIND_PACK) {
    // the LWE mask as the polynomial whose constant term pairs with the key (src/keyswitch.c:530-533)
    const uint64_t *c = p.in + (size_t)blockIdx.x * (N + 1);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int x = m * T + tid;
      al[m] = extract0_coeff(c, x, N);
      ah[m] = 0 - c[M - x];           // coefficient M + x: N - (M + x)
      acc1[x] = x == 0 ? c[N] : 0;
      acc1[M + x] = 0;
    }
    F::sync();
  } else {
    // merge r of output o at level lvl:  E = P[r], O = X^s P[r + cnt], s = N / 2^lvl;  acc = U = E + O, v = V = E - O;  acc += KeySwitch_(log2 N - lvl)(V(X^(2^lvl + 1)))
    const int lvl = p.lvl;
    const unsigned cnt = 1u << p.cnt_log, o = blockIdx.x >> p.cnt_log, r = blockIdx.x & (cnt - 1);
    const size_t first = (size_t)o * 2 * cnt + r;
    uint64_t va_lo[8], va_hi[8], vb_lo[8], vb_hi[8];
    if (lvl == 1) {
      // the leaves are LWE samples first and first + cnt, embedded on the fly (s = M): O.a[x] = -a'[x + M] = in.a[M - x], O.a[M + x] = a'[x], O.b = in.b X^M.  A sample
      // past the end is read as sample 0 and masked to zero: no load depends on a branch
      const uint64_t k0 = first < (size_t)p.total ? ~0ull : 0ull, k1 = first + cnt < (size_t)p.total ? ~0ull : 0ull;
      const uint64_t *c0 = p.in + (k0 ? first : 0) * (N + 1), *c1 = p.in + (k1 ? first + cnt : 0) * (N + 1);
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int x = m * T + tid;
        const uint64_t e_lo = extract0_coeff(c0, x, N) & k0, e_hi = (0 - c0[M - x]) & k0;
        const uint64_t o_lo = c1[M - x] & k1, o_hi = extract0_coeff(c1, x, N) & k1;
        const uint64_t eb = x == 0 ? c0[N] & k0 : 0, ob = x == 0 ? c1[N] & k1 : 0;
        al[m] = e_lo + o_lo; va_lo[m] = e_lo - o_lo;
        ah[m] = e_hi + o_hi; va_hi[m] = e_hi - o_hi;
        acc1[x] = eb; vb_lo[m] = eb;
        acc1[M + x] = ob; vb_hi[m] = 0 - ob;
      }
    } else {
      // s <= N / 4: only the low half wraps, X^s p [x] = -p[x - s + N] for x < s
      const int s = N >> lvl;
      const uint64_t *s0 = p.in + first * (2 * N), *s1 = s0 + (size_t)cnt * (2 * N);
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int x = m * T + tid;
        const uint64_t a0 = s1[(x - s) & (N - 1)], b0 = s1[N + ((x - s) & (N - 1))];
        const uint64_t oa_lo = x < s ? 0 - a0 : a0, ob_lo = x < s ? 0 - b0 : b0, oa_hi = s1[M + x - s], ob_hi = s1[N + M + x - s];
        const uint64_t ea_lo = s0[x], ea_hi = s0[M + x], eb_lo = s0[N + x], eb_hi = s0[N + M + x];
        al[m] = ea_lo + oa_lo; va_lo[m] = ea_lo - oa_lo;
        ah[m] = ea_hi + oa_hi; va_hi[m] = ea_hi - oa_hi;
        acc1[x] = eb_lo + ob_lo; vb_lo[m] = eb_lo - ob_lo;
        acc1[M + x] = eb_hi + ob_hi; vb_hi[m] = eb_hi - ob_hi;
      }
    }
    F::sync();
    trace_step<F, true>(al, ah, acc1, va_lo, va_hi, vb_lo, vb_hi, (1 << lvl) + 1, xch, fft, p.key + (size_t)(LOGN - lvl) * entry_sz, t, base_bit, off, scale, tid);
    steps = p.tail;
  }
#pragma unroll 1
  for (int j = 0; j < steps; j++) trace_step<F, false>(al, ah, acc1, al, ah, al, ah, (N >> j) + 1, xch, fft, p.key + (size_t)j * entry_sz, t, base_bit, off, scale, tid);
  uint64_t *o = p.out + (size_t)blockIdx.x * (2 * N);
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
  const uint64_t off = GADGET_OFFSET(t, base_bit);
  const RoundCtx scale = round_scale<M>();
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

// An entry of a layer handle's lists (row_ptr, col) through the constant address space: the handle's image is not written while a kernel runs, so the word is a
// scalar load whatever else the kernel's other kinds store -- as a vector load the column costs the entry loop a vmcnt wait of its own in front of its operand loads.
__device__ __forceinline__ int list_word(const int *list, int i) {
  typedef const int __attribute__((address_space(4))) *const_ints_t;
  return ((const_ints_t)list)[i];
}

// The tail of a linear layer on packed samples, defined once for kinds 4 and 6: the accumulator pair of team blockIdx.x = b rows_out + j through two inverse transforms
// and the general rounding, the bias on component b, and either the TRLWE sample or trlwe_extract_tlwe(., idx) written straight from the registers.
template <class F>
__device__ __forceinline__ void polylinear_finish(double (&o_re)[2][8], double (&o_im)[2][8], d2 *xch, const F &fft, const TraceParams &p, unsigned j, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  const RoundCtx scale = round_scale<M>();
  const uint64_t *bias = p.bias ? p.bias + (size_t)j * N : nullptr;
  const int idx = p.idx;
  uint64_t *o = p.out + (size_t)blockIdx.x * (idx < 0 ? (size_t)2 * N : (size_t)N + 1);
  fft.inverse(o_re[0], o_im[0], xch, tid);
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int c0 = m * T + tid, c1 = M + c0;
    const uint64_t lo = round_mod_2_64(o_re[0][m], scale), hi = round_mod_2_64(o_im[0][m], scale);
    if (idx < 0) {
      o[c0] = lo;
      o[c1] = hi;
    } else {
      // trlwe_extract_tlwe: a[i] = out.a[idx - i] for i <= idx, -out.a[N + idx - i] above: coefficient c goes to word (idx - c) mod N, negated when c > idx
      o[(idx - c0) & (N - 1)] = c0 <= idx ? lo : 0 - lo;
      o[(idx - c1) & (N - 1)] = c1 <= idx ? hi : 0 - hi;
    }
  }
  fft.inverse(o_re[1], o_im[1], xch, tid);
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int c0 = m * T + tid, c1 = M + c0;
    const uint64_t lo = round_mod_2_64(o_re[1][m], scale) + (bias ? bias[c0] : 0), hi = round_mod_2_64(o_im[1][m], scale) + (bias ? bias[c1] : 0);
    if (idx < 0) {
      o[N + c0] = lo;
      o[N + c1] = hi;
    } else {
      if (c0 == idx) o[N] = lo;
      if (c1 == idx) o[N] = hi;
    }
  }
}

// out[b][j] = G(sum_e F(in[b][col_e]) (.) F(val_e)) + (0, bias[j]), the sum in the stored order of row j's entries from +0.0; blockIdx.x = b rows_out + j
template <class F>
__device__ __forceinline__ void polylinear_body(d2 *xch, const F &fft, const TraceParams &p, int tid) {
  constexpr int M = F::M, T = F::THREADS;
  const unsigned b = blockIdx.x / (unsigned)p.rows_out, j = blockIdx.x % (unsigned)p.rows_out;
  const d2 *__restrict__ x = p.xin + (size_t)b * p.rows_in * (2 * M);
  double o_re[2][8], o_im[2][8];
#pragma unroll
  for (int cc = 0; cc < 2; cc++)
#pragma unroll
    for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
  const int end = list_word(p.row_ptr, j + 1);
#pragma unroll 1
  for (int e = list_word(p.row_ptr, j); e < end; e++) {
    const d2 *__restrict__ w = p.key + (size_t)e * M;
    const d2 *__restrict__ xa = x + (size_t)list_word(p.col, e) * (2 * M);
    d2 wv[8], a[8], bb[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { wv[m] = w[m * T + tid]; a[m] = xa[m * T + tid]; bb[m] = xa[M + m * T + tid]; }
#pragma unroll
    for (int m = 0; m < 8; m++) {
      cmac(o_re[0][m], o_im[0][m], a[m].x, a[m].y, wv[m]);
      cmac(o_re[1][m], o_im[1][m], bb[m].x, bb[m].y, wv[m]);
    }
  }
  polylinear_finish<F>(o_re, o_im, xch, fft, p, j, tid);
}

// kind 5: pool[blockIdx.x][c l + i] = F(dec_i(in[blockIdx.x].c)), blockIdx.x = b rows_in + input; the digit is ks_rows_rt's: an unsigned field of the word plus
// GADGET_OFFSET, re-centred
template <class F>
__device__ __forceinline__ void gsw_digits_body(d2 *xch, const F &fft, const TraceParams &p, int tid) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  const int l = p.l, base_bit = p.base_bit;
  const uint64_t *c = p.in + (size_t)blockIdx.x * (2 * N);
  d2 *__restrict__ dst = p.sel + (size_t)blockIdx.x * 2 * l * M;
  const uint64_t off = GADGET_OFFSET(l, base_bit);
  const uint32_t mask = (1u << base_bit) - 1;
  const int half = 1 << (base_bit - 1);
#pragma unroll 1
  for (int cc = 0; cc < 2; cc++) {
    uint64_t dd_lo[8], dd_hi[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { dd_lo[m] = c[cc * N + m * T + tid] + off; dd_hi[m] = c[cc * N + M + m * T + tid] + off; }
#pragma unroll 1
    for (int i = 0; i < l; i++) {
      const int shift = 64 - (i + 1) * base_bit;
      double re[8], im[8];
#pragma unroll
      for (int m = 0; m < 8; m++) {
        re[m] = (double)((int)((uint32_t)(dd_lo[m] >> shift) & mask) - half);
        im[m] = (double)((int)((uint32_t)(dd_hi[m] >> shift) & mask) - half);
      }
      fft.forward(re, im, xch, tid);
#pragma unroll
      for (int m = 0; m < 8; m++) dst[m * T + tid] = d2{re[m], im[m]};
      dst += M;
    }
  }
}

// kind 6: out[b][j] = G(sum_e sum_r pool[b][col_e][r] (.) W_e[r]) + (0, bias[j]), one chain per component over the entries in the stored order and the rows r = 0 .. 2l - 1
// from +0.0; blockIdx.x = b rows_out + j
template <class F>
__device__ __forceinline__ void gsw_sum_body(d2 *xch, const F &fft, const TraceParams &p, int tid) {
  constexpr int M = F::M, T = F::THREADS;
  const unsigned b = blockIdx.x / (unsigned)p.rows_out, j = blockIdx.x % (unsigned)p.rows_out;
  const int rows = 2 * p.l;
  const d2 *__restrict__ x = p.xin + (size_t)b * p.rows_in * rows * M;
  double o_re[2][8], o_im[2][8];
#pragma unroll
  for (int cc = 0; cc < 2; cc++)
#pragma unroll
    for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
  const int end = list_word(p.row_ptr, j + 1);
#pragma unroll 1
  for (int e = list_word(p.row_ptr, j); e < end; e++) {
    const d2 *__restrict__ w = p.key + (size_t)e * rows * (2 * M);
    const d2 *__restrict__ dg = x + (size_t)list_word(p.col, e) * rows * M;
#pragma unroll 1
    for (int r = 0; r < rows; r++) {
      d2 d[8], k0[8], k1[8];
#pragma unroll
      for (int m = 0; m < 8; m++) { d[m] = dg[m * T + tid]; k0[m] = w[m * T + tid]; k1[m] = w[M + m * T + tid]; }
#pragma unroll
      for (int m = 0; m < 8; m++) {
        cmac(o_re[0][m], o_im[0][m], d[m].x, d[m].y, k0[m]);
        cmac(o_re[1][m], o_im[1][m], d[m].x, d[m].y, k1[m]);
      }
      dg += M;
      w += 2 * M;
    }
  }
  polylinear_finish<F>(o_re, o_im, xch, fft, p, j, tid);
}

// kind 7's gate record, one per gate in the handle's level-sorted table: op_row = op | (gate index << 4); x, y, z = wire indices (-1: unused)
struct __attribute__((aligned(16))) SelGate {
  int op_row, x, y, z;
};
enum { SEL_NOT = 0, SEL_AND, SEL_NAND, SEL_OR, SEL_NOR, SEL_XOR, SEL_XNOR, SEL_ANDNOT, SEL_MUX, SEL_OPS };

// T(S)_r.c: one polynomial of a selector row back in the torus domain, the words torus_to_dft_kernel's inverse direction writes
template <class F>
__device__ __forceinline__ void sel_row_words(uint64_t (&lo)[8], uint64_t (&hi)[8], const d2 *poly, d2 *xch, const F &fft, const RoundCtx &scale, int tid) {
  constexpr int T = F::THREADS;
  double re[8], im[8];
#pragma unroll
  for (int m = 0; m < 8; m++) { const d2 v = poly[m * T + tid]; re[m] = v.x; im[m] = v.y; }
  fft.inverse(re, im, xch, tid);
#pragma unroll
  for (int m = 0; m < 8; m++) { lo[m] = round_mod_2_64(re[m], scale); hi[m] = round_mod_2_64(im[m], scale); }
}

// kind 7: row r of gate k of the level on batch element b, blockIdx.x = (b gates + k) 2l + r:
//   out[r] = F(h H_r + cx T(X)_r + cy T(Y)_r + cp E(L, W)),   L = T(X)_r (MUX: T(X)_r - T(Y)_r),  W = Y (MUX: Z)
//   op      NOT  AND  NAND  OR  NOR  XOR  XNOR  ANDNOT  MUX
//   h        1    0    1    0    1    0    1      0      0
//   cx      -1    0    0    1   -1    1   -1      1      0
//   cy       0    0    0    1   -1    1   -1      0      1
//   cp       0    1   -1   -1    1   -2    2     -1      1
// E is the external product of the other calls: the digits of L.a against W's rows 0 .. l - 1, then those of L.b against rows l .. 2l - 1, into ONE accumulator pair from
// +0.0 (ks_rows_rt twice), two inverse transforms, the general rounding.  Only the product's words stay in registers across the tail: the rows of X and Y are loaded
// and inverted again behind it (lut_cmux_kernel mode 4 re-reads its base the same way), so the kind holds less than rlwe_priv_keyswitch_body does.  Wires below rows_in
// are rows of xin, the others rows of sel written by EARLIER launches: a gate never reads the level it belongs to.
template <class F>
__device__ __forceinline__ void sel_gate_body(d2 *xch, const F &fft, const TraceParams &p, int tid) {
  constexpr int M = F::M, T = F::THREADS;
  const int l = p.l, base_bit = p.base_bit;
  const unsigned rows = 2 * l, r = blockIdx.x % rows, u = blockIdx.x / rows, k = u % (unsigned)p.idx, b = u / (unsigned)p.idx;
  // through the constant address space: the handle's table is not written while a kernel runs, so the record is one 16-byte scalar load (LutStep's idiom)
  typedef const SelGate __attribute__((address_space(4))) *const_gates_t;
  const const_gates_t table = (const_gates_t) reinterpret_cast<const SelGate *>(p.row_ptr);
  const SelGate e = {table[k].op_row, table[k].x, table[k].y, table[k].z};
  const int op = e.op_row & 15;
  const size_t row = (size_t)2 * M, sample = rows * row;
  const d2 *in = p.xin + (size_t)b * p.rows_in * sample;
  d2 *mine = p.sel + (size_t)b * p.rows_out * sample;   // read (earlier gates) and written (this gate): no __restrict__
  const d2 *X = (e.x < p.rows_in ? in + (size_t)e.x * sample : mine + (size_t)(e.x - p.rows_in) * sample) + r * row;
  const int wy = op == SEL_NOT ? e.x : e.y, wz = op == SEL_MUX ? e.z : wy;
  const d2 *Ys = wy < p.rows_in ? in + (size_t)wy * sample : mine + (size_t)(wy - p.rows_in) * sample;
  const d2 *W = wz < p.rows_in ? in + (size_t)wz * sample : mine + (size_t)(wz - p.rows_in) * sample;
  const d2 *Y = Ys + r * row;
  const bool h = (0x055u >> op) & 1;
  const uint64_t cx = (uint64_t)(int64_t)((int)(((0x07743u >> (2 * op)) & 3) ^ 2) - 2), cy = (uint64_t)(int64_t)((int)(((0x13740u >> (2 * op)) & 3) ^ 2) - 2);
  const uint64_t cp = (uint64_t)(int64_t)((int)(((uint32_t)(0x1F2E1FF10ull >> (4 * op)) & 15) ^ 8) - 8);
  const RoundCtx scale = round_scale<M>();
  uint64_t pa_lo[8], pa_hi[8], pb_lo[8], pb_hi[8];
#pragma unroll
  for (int m = 0; m < 8; m++) { pa_lo[m] = 0; pa_hi[m] = 0; pb_lo[m] = 0; pb_hi[m] = 0; }
  if (cp) {
    const uint64_t off = GADGET_OFFSET(l, base_bit);
    double o_re[2][8], o_im[2][8];
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
      for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
#pragma unroll 1
    for (int cc = 0; cc < 2; cc++) {
      uint64_t dd_lo[8], dd_hi[8];
      sel_row_words<F>(dd_lo, dd_hi, X + cc * M, xch, fft, scale, tid);
      if (op == SEL_MUX) {
        uint64_t y_lo[8], y_hi[8];
        sel_row_words<F>(y_lo, y_hi, Y + cc * M, xch, fft, scale, tid);
#pragma unroll
        for (int m = 0; m < 8; m++) { dd_lo[m] -= y_lo[m]; dd_hi[m] -= y_hi[m]; }
      }
#pragma unroll
      for (int m = 0; m < 8; m++) { dd_lo[m] += off; dd_hi[m] += off; }
      ks_rows_rt<F>(dd_lo, dd_hi, o_re, o_im, xch, fft, W + (size_t)cc * l * row, l, base_bit, tid);
    }
    fft.inverse(o_re[0], o_im[0], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) { pa_lo[m] = cp * round_mod_2_64(o_re[0][m], scale); pa_hi[m] = cp * round_mod_2_64(o_im[0][m], scale); }
    fft.inverse(o_re[1], o_im[1], xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) { pb_lo[m] = cp * round_mod_2_64(o_re[1][m], scale); pb_hi[m] = cp * round_mod_2_64(o_im[1][m], scale); }
  }
  // H_r: 2^(64 - (i + 1) Bg_bit) at coefficient 0 (thread 0, word 0) of component c, r = c l + i
  const unsigned c = r >= (unsigned)l, i = r - c * l;
  const uint64_t hw = h ? 1ull << (64 - (i + 1) * base_bit) : 0;
  d2 *dst = mine + (size_t)(e.op_row >> 4) * sample + r * row;
#pragma unroll 1
  for (int q = 0; q < 2; q++) {   // one rolled body, as rlwe_priv_keyswitch_body's tail
    uint64_t v_lo[8], v_hi[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { v_lo[m] = q ? pb_lo[m] : pa_lo[m]; v_hi[m] = q ? pb_hi[m] : pa_hi[m]; }
    if (cx) {
      uint64_t t_lo[8], t_hi[8];
      sel_row_words<F>(t_lo, t_hi, X + q * M, xch, fft, scale, tid);
#pragma unroll
      for (int m = 0; m < 8; m++) { v_lo[m] += cx * t_lo[m]; v_hi[m] += cx * t_hi[m]; }
    }
    if (cy) {
      uint64_t t_lo[8], t_hi[8];
      sel_row_words<F>(t_lo, t_hi, Y + q * M, xch, fft, scale, tid);
#pragma unroll
      for (int m = 0; m < 8; m++) { v_lo[m] += cy * t_lo[m]; v_hi[m] += cy * t_hi[m]; }
    }
    if ((unsigned)q == c && tid == 0) v_lo[0] += hw;
    double re[8], im[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { re[m] = torus_to_double(v_lo[m]); im[m] = torus_to_double(v_hi[m]); }
    fft.forward(re, im, xch, tid);
#pragma unroll
    for (int m = 0; m < 8; m++) dst[q * M + m * T + tid] = d2{re[m], im[m]};
  }
}

template <class F>
__global__ __launch_bounds__(F::THREADS, 1) void trace_conversions_kernel(TraceParams p) {
  __shared__ __attribute__((aligned(16))) d2 xch[F::XCH_SLOTS];
  __shared__ __attribute__((aligned(16))) uint64_t acc1[F::N];   // the trace's component b (kind 0)
  const int tid = threadIdx.x;
  F fft;
  fft.init(p.tw, tid);
  if (p.kind == TRACE_KIND_PACK || p.kind == TRACE_KIND_MANY) trace_pack_body<F>(xch, acc1, fft, p, tid);
  else if (p.kind == TRACE_KIND_POLYLINEAR) polylinear_body<F>(xch, fft, p, tid);
  else if (p.kind == TRACE_KIND_GSW_DIGITS) gsw_digits_body<F>(xch, fft, p, tid);
  else if (p.kind == TRACE_KIND_GSW_SUM) gsw_sum_body<F>(xch, fft, p, tid);
  else if (p.kind == TRACE_KIND_SEL_GATE) sel_gate_body<F>(xch, fft, p, tid);
  else rlwe_priv_keyswitch_body<F>(xch, fft, p.key, p.key + (size_t)p.t * 2 * F::M, p.in, p.out, p.t, p.base_bit, p.kind == TRACE_KIND_GADGET ? p.sel : nullptr, p.l, tid);
}

}  // namespace mosfhet
