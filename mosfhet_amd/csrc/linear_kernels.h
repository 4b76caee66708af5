// linear_kernels.h -- device code of mosfhet_hip_tlwe_linear_batch (gfx950): y = W x + bias with cleartext integer weights on batches of LWE samples, the
// reference's tlwe_scale / tlwe_scale_addto / tlwe_scale_subto / tlwe_add / tlwe_sub (src/tlwe.c:143-191) applied row by row.  Own code.
//
//   out[b][j][c] = (c == n ? bias[j] : 0) + sum_i W[j][i] in[b][i][c]   (mod 2^64),   samples of w = n + 1 words, the b word last
//
// One kernel, one instantiation: words on the lanes, weights on the scalar path.  A wavefront is one unit of work: a strip of 64 word columns c of one batch
// element b and a tile of TJ output rows, whose TJ 64-bit accumulators (2 VGPRs each) live in registers.  The four wavefronts of a workgroup are four
// independent units; there is no LDS and no barrier.
//   dense   the wavefront walks i = 0 .. rows_in - 1: ONE coalesced load of in[b][i][c ..] feeds all TJ accumulators, so the input is read ceil(rows_out / TJ)
//           times, not rows_out times.  The weights of a tile are stored tile-major, [tile][i][TJ] (rows past rows_out padded with zeros), so the TJ weights of a
//           step are 64 contiguous bytes at a wave-uniform address: one scalar load.
//   sparse  the wavefront walks the CSR list of each of its TJ rows in turn (column and weight by scalar loads).  A list of the FIRST launch never holds more
//           than LINEAR_CHUNK entries: the handle cuts longer rows into chunks at creation (capi_linear.inc), whose partial sums go to a staging row each, and a
//           second launch of this same kernel adds a row's partial sums (weights 1) -- integer sums do not depend on the order, so the cut changes no word, and
//           the longest serial walk of a row of E entries is max(LINEAR_CHUNK, ceil(E / LINEAR_CHUNK)) loads instead of E (the second-level lists are not cut
//           again).  What the cut buys on a skewed matrix has not been measured.
// Multiply: low 64 bits of x * w for a signed 64-bit w.  A weight in [-2^31, 2^31) (`narrow`, decided at creation for the whole matrix) takes one
// v_mad_u64_u32 on the low halves plus a 32-bit correction of the high half.  Written on the weight as it stands that correction is x_hi * w_lo - (w < 0 ? x_lo : 0),
// five vector instructions per product with the select -- measured SLOWER than the wide form's four.  So the walk multiplies by the unsigned
// u = w + 2^31 = w_lo ^ 2^31 (a scalar instruction), whose correction is x_hi * u alone (on paper a v_mad_u64_u32, a v_mul_lo_u32 and a 32-bit add), and takes
// 2^31 * (the sum of the list's inputs) off at the end -- one more 64-bit add per loaded word, shared by the TJ rows of a dense tile.  Exact mod 2^64: no word
// changes.  Measured: faster than the first form, but as the compiler writes it still slower than the wide form, in the call and alone
// (tools/ubench/linear_mac.hip): `narrow` does not select a cheaper sequence yet.
// Any other weight takes the three-product form (v_mad_u64_u32, two v_mul_lo_u32, one three-operand add).  The choice is one wave-uniform branch around
// the walk, not a second instantiation.
// Grid: the units are numbered [b][strip][tile], tile fastest (neighbouring wavefronts read the same input strip); the launcher folds the workgroup index over
// gridDim.x and gridDim.y (capi_linear.inc: linear_plan) and the kernel unfolds it, so no count is placed raw on a dimension limited to 65535.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace mosfhet {

constexpr int LINEAR_TJ = 8;        // output rows per wavefront
constexpr int LINEAR_CHUNK = 64;    // entries of a sparse list at most (longer rows are cut at creation)

struct LinearParams {
  const uint64_t *__restrict__ in;       // [count][in_rows][w]
  uint64_t *__restrict__ out;            // [count][out_rows][w]
  uint64_t *__restrict__ part;           // [count][part_rows][w]: staging rows of the chunks of cut rows (sparse, first launch)
  const int64_t *__restrict__ W;         // dense: [tiles][rows_in][TJ]
  const int *__restrict__ row_ptr;       // sparse: [lists + 1]
  const int *__restrict__ col;           // sparse: [entries]
  const int64_t *__restrict__ val;       // sparse: [entries]
  const int *__restrict__ dst;           // sparse: [lists] d >= 0: row d of out; d < 0: row ~d of part.  null: list j is row j of out
  const uint64_t *__restrict__ bias;     // [out_rows] or null; added to word n of the rows written to out
  int lists;                             // rows of W (dense) or lists (sparse)
  int rows_in, w, sparse, narrow;
  unsigned strips, tiles, units;         // strips of 64 words per sample, tiles of TJ lists, units = count * strips * tiles
  size_t in_rows, out_rows, part_rows;
};

// acc += x * w (low 64 bits).  NARROW: wt holds u = w + 2^31 in its low dword; the caller takes 2^31 * (sum of the x) off afterwards.
template <bool NARROW>
__device__ __forceinline__ uint64_t linear_mac(uint64_t acc, uint64_t x, int64_t wt) {
  if constexpr (NARROW) {
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32), u = (uint32_t)wt;
    const uint64_t a = (uint64_t)xl * u + acc;                         // v_mad_u64_u32
    const uint32_t hi = (uint32_t)(a >> 32) + xh * u;                  // only the high dword takes x_hi * u
    return ((uint64_t)hi << 32) | (uint32_t)a;
  } else {
    return acc + x * (uint64_t)wt;
  }
}
constexpr int64_t LINEAR_NARROW_BIAS = (int64_t)1 << 31;   // u = w + 2^31 = (low dword of w) ^ 2^31 for w in [-2^31, 2^31)

template <int TJ, bool NARROW>
__device__ __forceinline__ void linear_walk(const LinearParams &p, const uint64_t *__restrict__ x0, unsigned tile, uint64_t (&acc)[TJ]) {
  const size_t w = (size_t)p.w;
  if (!p.sparse) {
    const int64_t *__restrict__ wt = p.W + (size_t)tile * (size_t)p.rows_in * TJ;
    uint64_t sum = 0;
#pragma unroll 4
    for (int i = 0; i < p.rows_in; i++) {
      const uint64_t x = x0[(size_t)i * w];
      if constexpr (NARROW) sum += x;
#pragma unroll
      for (int t = 0; t < TJ; t++) acc[t] = linear_mac<NARROW>(acc[t], x, NARROW ? wt[(size_t)i * TJ + t] ^ LINEAR_NARROW_BIAS : wt[(size_t)i * TJ + t]);
    }
    if constexpr (NARROW) {
#pragma unroll
      for (int t = 0; t < TJ; t++) acc[t] -= sum << 31;
    }
  } else {
#pragma unroll
    for (int t = 0; t < TJ; t++) {
      const unsigned j = tile * TJ + t;
      if (j < (unsigned)p.lists) {
        const int end = p.row_ptr[j + 1];
        uint64_t sum = 0;
#pragma unroll 4
        for (int q = p.row_ptr[j]; q < end; q++) {
          const uint64_t x = x0[(size_t)p.col[q] * w];
          if constexpr (NARROW) sum += x;
          acc[t] = linear_mac<NARROW>(acc[t], x, NARROW ? p.val[q] ^ LINEAR_NARROW_BIAS : p.val[q]);
        }
        if constexpr (NARROW) acc[t] -= sum << 31;
      }
    }
  }
}

template <int TJ>
__global__ __launch_bounds__(256) void tlwe_linear_kernel(const LinearParams p) {
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const unsigned unit = (blockIdx.y * gridDim.x + blockIdx.x) * 4u + wave;   // units <= INT_MAX (linear_plan): no wrap
  if (unit >= p.units) return;
  const unsigned tile = unit % p.tiles, rest = unit / p.tiles, strip = rest % p.strips, b = rest / p.strips;
  const unsigned c = strip * 64 + lane;
  const bool live = c < (unsigned)p.w;
  const uint64_t *__restrict__ x0 = p.in + (size_t)b * p.in_rows * (size_t)p.w + (live ? c : (unsigned)p.w - 1);   // lanes past the sample read its last word
  uint64_t acc[TJ];
#pragma unroll
  for (int t = 0; t < TJ; t++) acc[t] = 0;
  if (p.narrow) linear_walk<TJ, true>(p, x0, tile, acc);
  else linear_walk<TJ, false>(p, x0, tile, acc);
#pragma unroll
  for (int t = 0; t < TJ; t++) {
    const unsigned j = tile * TJ + t;
    if (j >= (unsigned)p.lists || !live) continue;
    const int d = p.dst ? p.dst[j] : (int)j;
    if (d >= 0) {
      uint64_t v = acc[t];
      if (p.bias && c == (unsigned)p.w - 1) v += p.bias[d];
      p.out[((size_t)b * p.out_rows + (size_t)d) * (size_t)p.w + c] = v;
    } else {
      p.part[((size_t)b * p.part_rows + (size_t)~d) * (size_t)p.w + c] = acc[t];
    }
  }
}

}  // namespace mosfhet
