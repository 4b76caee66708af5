// pack_kernels.h -- device code of mosfhet_hip_tlwe_pack_batch (gfx950): batches of LWE samples packed into TRLWE samples, the reference's
// trlwe_full_packing_keyswitch (src/keyswitch.c:195-227) over a batch.  Own code.
//
//   output o packs samples o per .. min(total, (o + 1) per) - 1, sample j of it at coefficient j:
//     a_i(X) = sum_j in[o per + j].a[i] X^j                         (column i of the output's samples; coefficients past the last sample are 0)
//     as     = sum_{i < n_in} sum_{j < t} DFT(digit_j(a_i)) (.) KS[i][j]      (one accumulator pair, entries ascending, rows ascending)
//     out.a  = -round(as.a),   out.b[j] = in[o per + j].b - round(as.b)[j]
//
// Three kernels:
//   tlwe_pack_transpose_kernel   [samples][n_in + 1] -> staging [outputs of the round][n_in][N]: column i of an output's samples as one contiguous polynomial, so that
//                                the main kernel never gathers words (n_in + 1) * 8 bytes apart.  64 x 64 tiles through LDS (rows padded to 65 words: the transposed
//                                read walks a tile column at a stride of 65 words, odd, so the 64 lanes fall on different banks), 512-byte runs on both
//                                sides; sample rows are only 8-byte aligned, so words move one by one.  EVERY word of the staging is written, zeros included: a short
//                                output must not see the columns an earlier call left there.  The b column (i = n_in) goes straight to out.b (0 past the last sample),
//                                for every split: the main kernel (split = 1) or the sum kernel (split > 1) takes the products off it in place.
//   tlwe_pack_kernel<F>          one team (F::THREADS) per (output, part of the entries), launch bound 1 like trlwe_fft_keyswitch_kernel: the accumulators o_re / o_im[2][8]
//                                live across the whole entry loop, every entry runs ks_rows_rt (bootstrap_kernels.h) unchanged on its t key rows, the next entry's
//                                column is requested before the current entry's transforms; two inverse transforms at the end, rounded with the reducing
//                                round_mod_2_64 (the sums reach n_in t N 2^(base_bit - 1) 2^63: far past the bound of the reduction-free form).  Workgroup
//                                part * outputs + o: the teams of one part, which read the same key rows, are neighbours in launch order.
//   tlwe_pack_sum_kernel         split > 1: out = (0, b) - sum over the parts of their rounded pairs, as 64-bit integers (order-free: the words depend on the inputs,
//                                the key and the split only).
// No atomics, nothing to initialise: a replayed graph gives the same words.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "bootstrap_kernels.h"

namespace mosfhet {

constexpr int PACK_TILE = 64;

struct PackParams {
  const uint64_t *__restrict__ in;   // [samples of the round][n_in + 1], the first sample of the round's first output at in[0]
  uint64_t *__restrict__ cols;       // staging [outputs][n_in][N]
  uint64_t *__restrict__ parts;      // staging [outputs][split][2][N] (split > 1)
  uint64_t *out;                     // [outputs][2][N] (the b halves are written by the transposition and updated in place)
  int n_in, per, samples, outputs;   // samples, outputs: of this round
  int split, part_entries;
};

// grid (N / 64 * ceil((n_in + 1) / 64), outputs), block 256
__global__ __launch_bounds__(256) void tlwe_pack_transpose_kernel(PackParams p, int N) {
  __shared__ uint64_t tile[PACK_TILE][PACK_TILE + 1];
  const int jt = N / PACK_TILE;
  const int j0 = (int)(blockIdx.x % jt) * PACK_TILE, i0 = (int)(blockIdx.x / jt) * PACK_TILE, o = blockIdx.y;
  const int first = o * p.per;
  const int have = p.samples - first < p.per ? p.samples - first : p.per;   // samples of this output
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const size_t w = (size_t)p.n_in + 1;
  for (int r = ty; r < PACK_TILE; r += 4) {   // sample j0 + r, words i0 .. i0 + 63
    const int j = j0 + r, i = i0 + tx;
    tile[r][tx] = (j < have && i <= p.n_in) ? p.in[(size_t)(first + j) * w + i] : 0;
  }
  workgroup_sync();
  for (int r = ty; r < PACK_TILE; r += 4) {   // entry i0 + r, coefficients j0 .. j0 + 63
    const int i = i0 + r, j = j0 + tx;
    if (i < p.n_in) p.cols[((size_t)o * p.n_in + i) * N + j] = tile[tx][r];
    else if (i == p.n_in) p.out[(size_t)o * 2 * N + N + j] = tile[tx][r];
  }
}

template <class F>
__global__ __launch_bounds__(F::THREADS, 1) void tlwe_pack_kernel(PackParams p, const d2 *__restrict__ key, const d2 *__restrict__ tw, int t, int base_bit) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  __shared__ __attribute__((aligned(16))) d2 xch[F::XCH_SLOTS];
  const int tid = threadIdx.x;
  const int o = (int)(blockIdx.x % (unsigned)p.outputs), part = (int)(blockIdx.x / (unsigned)p.outputs);
  const int e0 = part * p.part_entries;
  const int e1 = e0 + p.part_entries < p.n_in ? e0 + p.part_entries : p.n_in;
  F fft;
  fft.init(tw, tid);
  const uint64_t off = GADGET_OFFSET(t, base_bit);
  const RoundCtx scale = round_scale<M>();
  const size_t entry_sz = (size_t)t * 2 * M;
  double o_re[2][8], o_im[2][8];
#pragma unroll
  for (int cc = 0; cc < 2; cc++)
#pragma unroll
    for (int m = 0; m < 8; m++) { o_re[cc][m] = 0.0; o_im[cc][m] = 0.0; }
  const uint64_t *__restrict__ col = p.cols + ((size_t)o * p.n_in + e0) * N;
  uint64_t nx_lo[8], nx_hi[8];
  if (e0 < e1) {
#pragma unroll
    for (int m = 0; m < 8; m++) { nx_lo[m] = col[m * T + tid]; nx_hi[m] = col[M + m * T + tid]; }
  }
#pragma unroll 1
  for (int i = e0; i < e1; i++) {
    uint64_t dd_lo[8], dd_hi[8];
#pragma unroll
    for (int m = 0; m < 8; m++) { dd_lo[m] = nx_lo[m] + off; dd_hi[m] = nx_hi[m] + off; }
    if (i + 1 < e1) {   // the next entry's column: in flight under this entry's transforms
      col += N;
#pragma unroll
      for (int m = 0; m < 8; m++) { nx_lo[m] = col[m * T + tid]; nx_hi[m] = col[M + m * T + tid]; }
    }
    ks_rows_rt<F>(dd_lo, dd_hi, o_re, o_im, xch, fft, key + (size_t)i * entry_sz, t, base_bit, tid);
  }
  // split = 1: out = (0, b) - as, in place on the b half the transposition wrote; split > 1: the rounded pair of this part, for tlwe_pack_sum_kernel
  const bool whole = p.split == 1;
  uint64_t *dst = whole ? p.out + (size_t)o * 2 * N : p.parts + ((size_t)o * p.split + part) * 2 * N;
  fft.inverse(o_re[0], o_im[0], xch, tid);
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const uint64_t lo = round_mod_2_64(o_re[0][m], scale), hi = round_mod_2_64(o_im[0][m], scale);
    dst[m * T + tid] = whole ? 0 - lo : lo;
    dst[M + m * T + tid] = whole ? 0 - hi : hi;
  }
  fft.inverse(o_re[1], o_im[1], xch, tid);
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const uint64_t lo = round_mod_2_64(o_re[1][m], scale), hi = round_mod_2_64(o_im[1][m], scale);
    dst[N + m * T + tid] = whole ? dst[N + m * T + tid] - lo : lo;
    dst[N + M + m * T + tid] = whole ? dst[N + M + m * T + tid] - hi : hi;
  }
}

// grid (ceil(2N / 256), outputs), block 256: word x of output o
__global__ __launch_bounds__(256) void tlwe_pack_sum_kernel(PackParams p, int N) {
  const int x = (int)(blockIdx.x * 256 + threadIdx.x), o = blockIdx.y;
  if (x >= 2 * N) return;
  uint64_t *dst = p.out + (size_t)o * 2 * N + x;
  const uint64_t *src = p.parts + (size_t)o * p.split * 2 * N + x;
  uint64_t v = x < N ? 0 : *dst;
  for (int q = 0; q < p.split; q++) v -= src[(size_t)q * 2 * N];
  *dst = v;
}

}  // namespace mosfhet
