// unpack_kernels.h -- device code of mosfhet_hip_trlwe_unpack_batch and of the table key switch that reads packed TRLWE samples (gfx950): the inverse layout of
// pack_kernels.h.  Own code.
//
//   in [outputs][2][N]; ciphertext c of a call is sample j = (first + c) % per of input o = (first + c) / per, the reference's trlwe_extract_tlwe (src/trlwe.c:540-552, k = 1):
//     extract(in[o], j).a[i] = (X^i in[o].a)[j] = i <= j ? a[j - i] : -a[N + j - i],      extract(in[o], j).b = in[o].b[j]
//   With a geometry (off, stride) sample j of an input is extract(in[o], off + j stride) instead: the launchers have checked off + (per - 1) stride <= N - 1, so no
//   coefficient index wraps; (0, 1) is the plain call and computes the same addresses.
//   Pure integer work: every word depends on the input words, per, the geometry and the index only.
//
// Two kernels:
//   trlwe_unpack_kernel              word (c, i) goes to out[c ldc + i ldi], the b word to out[c ldc + N ldi]: one kernel for both orientations.
//                                    ldi = 1 (rows of a [count][N + 1] batch, ldc = N + 1): a workgroup owns one input and `rows` of its samples, stages the mask polynomial once
//                                    into LDS (N words) and writes each row with the lanes along i -- the LDS read walks descending addresses, one word per lane, so the 64
//                                    lanes fall on different banks; the stores are 512-byte runs of words (rows are N + 1 words: only 8-byte aligned, as in
//                                    tlwe_pack_transpose_kernel).  The staged polynomial is 1 / rows of the bytes the workgroup writes.
//                                    ldc = 1 (the tiles' inT [N + 1][Bp], ldi = Bp): the lanes run along c; o and j come from c, so a run of 64 lanes may cross inputs
//                                    (per = 5 still writes full runs); for one i the lanes of one input read consecutive words, ascending (words `stride` apart with a
//                                    geometry: the 2N words of an input stay in the caches).  No LDS.
//   ks_words_entries_packed_kernel   ks_words_entries_kernel (keyswitch_words_kernels.h) from packed samples: the same entries and bvals, but the ciphertexts are already on
//                                    the fast index of the source, so no tile goes through LDS.
// No atomics, nothing to initialise: a replayed graph gives the same words.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "negacyclic_fft.h"   // workgroup_sync()

namespace mosfhet {

constexpr int UNPACK_THREADS = 256;
constexpr int UNPACK_COL_WORDS = 16;   // words i per thread of the column-major form

// mask word i of sample j of a packed input (a: its mask polynomial; N a power of two): one load, the wrapped part (i > j) negated
__device__ __forceinline__ uint64_t unpack_mask_word(const uint64_t *__restrict__ a, int N, int j, int i) {
  const uint64_t v = a[(j - i) & (N - 1)];
  return i <= j ? v : (uint64_t)0 - v;
}

// ldi == 1: grid inputs the call touches x ceil(per / rows), dynamic LDS N words.  ldc == 1: grid (ceil(count / 256), ceil((N + 1) / UNPACK_COL_WORDS)), no LDS.
__global__ __launch_bounds__(UNPACK_THREADS) void trlwe_unpack_kernel(uint64_t *__restrict__ out, const uint64_t *__restrict__ in, int N, int per, int first, int off,
                                                                      int stride, int count, size_t ldc, size_t ldi, int rows) {
  extern __shared__ uint64_t unpack_poly[];   // [N] (row-major form)
  const int tid = threadIdx.x;
  if (ldi == 1) {
    const int blocks = (per + rows - 1) / rows;   // per input
    const int o = first / per + (int)(blockIdx.x / (unsigned)blocks);
    const uint64_t *__restrict__ a = in + (size_t)o * 2 * N;
    for (int x = tid; x < N; x += UNPACK_THREADS) unpack_poly[x] = a[x];
    workgroup_sync();
    const int j0 = (int)(blockIdx.x % (unsigned)blocks) * rows;
    for (int r = 0; r < rows; r++) {
      const int j = j0 + r;
      const long long c = (long long)o * per + j - first;   // the call's ciphertext index
      if (j >= per || c >= count) break;
      if (c < 0) continue;
      const int jc = off + j * stride;   // the coefficient sample j sits at
      uint64_t *__restrict__ row = out + (size_t)c * ldc;
      for (int i = tid; i < N; i += UNPACK_THREADS) {
        const uint64_t v = unpack_poly[(jc - i) & (N - 1)];
        row[i] = i <= jc ? v : (uint64_t)0 - v;
      }
      if (tid == 0) row[N] = a[N + jc];
    }
    return;
  }
  const int c = (int)blockIdx.x * UNPACK_THREADS + tid;
  if (c >= count) return;
  const int g = first + c, o = g / per, j = off + (g - o * per) * stride;
  const uint64_t *__restrict__ a = in + (size_t)o * 2 * N;
  const int i0 = (int)blockIdx.y * UNPACK_COL_WORDS;
#pragma unroll 4
  for (int k = 0; k < UNPACK_COL_WORDS; k++) {
    const int i = i0 + k;
    if (i < N) out[(size_t)c * ldc + (size_t)i * ldi] = unpack_mask_word(a, N, j, i);
    else if (i == N) out[(size_t)c * ldc + (size_t)N * ldi] = a[N + j];
  }
}

// entries [n_in = N][chunks][ctwaves][JB][64] uint16 and bvals [count], as ks_words_entries_kernel writes them (padding ciphertexts: digit 0).
// grid (ctwaves, ceil(N / 64)), block (64, 4): lane tx = ciphertext, ty strides the 64 input words of the block
__global__ __launch_bounds__(256) void ks_words_entries_packed_kernel(const uint64_t *__restrict__ in, int N, int per, int first, int off, int stride, int count, int t,
                                                                     int base_bit, int JB, int ctwaves, uint16_t *__restrict__ entries, uint64_t *__restrict__ bvals) {
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int c = (int)blockIdx.x * 64 + tx, i0 = (int)blockIdx.y * 64;
  const bool live = c < count;
  const int g = first + (live ? c : 0), o = g / per, j = off + (g - o * per) * stride;
  const uint64_t *__restrict__ a = in + (size_t)o * 2 * N;
  if (blockIdx.y == 0 && ty == 0 && live) bvals[c] = a[N + j];
  const uint64_t round_off = 1ull << (63 - base_bit * t);
  const uint32_t mask = (1u << base_bit) - 1;
  const int chunks = t / JB;
  // the block's 16 source words of this lane first, as independent loads: one memory latency instead of sixteen in a row
  uint64_t w[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = i0 + ty + 4 * k;
    w[k] = (live && i < N) ? unpack_mask_word(a, N, j, i) + round_off : 0;
  }
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = i0 + ty + 4 * k;
    for (int q = 0; q < t && i < N; q++) {
      const uint32_t v = live ? ((uint32_t)(w[k] >> (64 - (q + 1) * base_bit)) & mask) : 0;
      const size_t e = ((((size_t)i * chunks + q / JB) * ctwaves + blockIdx.x) * JB + q % JB) * 64 + tx;
      entries[e] = (uint16_t)(0x1000u | (2 * v));
    }
  }
}

}  // namespace mosfhet
