// leveled_lut_kernels.h -- device code of mosfhet_hip_leveled_lut_batch (gfx950): eval_LUT of the reference's leveled application
// (applications/leveled_lut/vertical_packing.c:24-52: a CMUX tree over the top bits of the index, blind_rotate with the low selectors as key and the
// powers of two as mask, sample extract) for a batch of INDEPENDENT inputs, each given bit by bit as TRGSW_DFT selectors, against ONE shared table.
//
// What the batch shares, and what is therefore done once per call instead of once per input: on tree level 0 both CMUX operands are rows of the
// table, so T[j + half] - T[j], its 2l gadget digit polynomials and their forward transforms do not depend on the input.
//   lut_prepare_kernel   D[j][r] = DFT(digit_r(table[j + half] - table[j]))                              one workgroup per (node, row)
//   lut_level0_kernel    T[b][j] = table[j] + round(inverse(sum_r D[j][r] sel[b][size-1][r]))            no forward transform at all
//   lut_cmux_kernel      mode 0: one deeper tree level in place on the per-input intermediates, T[b][j] += sel[b][s] (.) (T[b][j + half] - T[b][j])
//                        mode 1: one workgroup per input, accumulator in LDS across the min(size, log2 N) rotate-CMUX steps, then SampleExtract_0
//                        (workgroups of two teams that share the rows of every product: half the forward transforms on the critical path, one inverse each)
// The gadget (l, Bg_bit) is a run-time argument of all three (one instantiation per ring): level 0 uses l only as the trip count of its
// multiply-add loop, and a CMUX is a loop over (component, digit) -- digit r of the difference, forward transform, two multiply-adds.
// Arithmetic: digits as Digits<L, 0> extracts them (src/polynomial.c:74-89), the transforms of negacyclic_fft.h, the fma chain of cmux_rows over rows
// 0 .. 2l-1 starting from zero, the inverse transforms, add_rounded<true> (selectors are caller-held DFT content and carry no magnitude bound): the words of
// external_product_kernel<.., CMUX> and pbs_kernel at the run-time gadget, i.e. the reference's order.
//
// Several tables over the SAME selectors (mosfhet_hip_leveled_lut_tables_batch): a table is one more index of the same units -- a grid dimension of the
// preparation, the slow part of the node index of level 0 (whose intermediates are [input][table][node]) and of a deeper level's units -- and
//   lut_tables_finish_kernel   one workgroup per (input, group of G tables): the G accumulators in LDS, the rotate steps outermost, so that a selector is
//                              fetched from memory once per group and re-read from the caches for the other tables of the group; SampleExtract_0 per table
// The one-table call is the case tables = 1 of the first three kernels and keeps lut_cmux_kernel's mode 1 as its finish.
//
// Several outputs packed into one table (mosfhet_hip_leveled_lut_packed_batch): an entry occupies m = 2^pack_log adjacent coefficients, so a table of 2^size entries
// is 2^(size + pack_log) / N TRLWEs.  The tree kernels do not know: they take their node count and table stride from the launcher.  The finish -- always
// lut_tables_finish_kernel, also at one table -- rotates by m 2^i in step i, for log2 N - pack_log steps at most, and extracts the m coefficients 0 .. m-1 of the
// rotated accumulator; both are run-time arguments (LutParams::pack_log, 0 for every other call, where they reduce to the words above).
//
// Memories that belong to the input (mosfhet_hip_trlwe_ram_read_batch / _write_batch, capi_ram.inc): 2^size TRLWE cells per input, the selectors its address bits.
// Two further run-time modes of lut_cmux_kernel, no kernel of their own: mode 2 is mode 0's tree level from one place to another (memory -> workspace -> output),
// mode 3 the chain of `size` CMUXes between a cell and the value to write, the difference in LDS across the products as mode 1 keeps its accumulator.
//
// Automata over encrypted words (mosfhet_hip_trlwe_automaton_batch, capi_automaton.inc): a vector of `states` TRLWE samples per input, one backward step per symbol.
// One further run-time mode of lut_cmux_kernel, mode 4: mode 2's "from one place to another" with the two operands picked by the layer's transition entries and
// rotated exactly (rot_coeff, as mode 1 rotates) on their way into the difference and, for the base, again at the store.
#pragma once
#include "bootstrap_kernels.h"

namespace mosfhet {

struct LutParams {
  const d2 *__restrict__ sel;        // [count][size][2l][2][M] complex, slot order: selector i of input b encrypts bit i of b's index
  const d2 *__restrict__ tw;         // twiddle table of the ring
  const uint64_t *__restrict__ lut;  // [n_luts][2][N] the shared table (read only)
  d2 *dtab;                          // [half0][2l][M] complex: the transformed digit rows of level 0's differences
  uint64_t *work;                    // [inputs of the chunk][half0][2][N] intermediates of the tree (null without a tree)
  uint64_t *out;                     // [count][N + 1]
  int size, l, Bg_bit;
  int half0;                         // nodes of tree level 0 (0: no tree)
  int first, inputs;                 // the chunk: inputs first .. first + inputs - 1 of the batch
  int mode, half, sel_index;         // lut_cmux_kernel: mode 0 = the tree level with `half` nodes and selector `sel_index`; mode 1 = finish
                                     // modes 2 and 3, the per-input memories of capi_ram.inc (no table, no tree of this struct's): the fields mean
                                     //   mode 2 (a level of a read): lut = the level's source rows, lut_stride = words from one input's rows to the next;
                                     //          out = its destination rows, half0 = destination rows per input; half, sel_index as in mode 0
                                     //   mode 3 (a write): lut = the values [count][2][N]; out = the memories [count][2^size][2][N], updated in place
                                     // mode 4, a step of an automaton (capi_automaton.inc): lut = the state vectors V_{t+1}, lut_stride = words from one input's vector
                                     //          to the next (0: one vector shared by the batch); out = V_t, half0 = destination rows per input; half = states computed
                                     //          per input, the first of them state `steps` (all: half = states, steps = 0; one: half = 1, steps = start);
                                     //          size = the word's length, sel_index = t; dtab = the layer's transition entries, one 16-byte {next0, next1, rot0, rot1}
                                     //          per state (read as LutStep through scalar loads: the state of a unit is uniform)
  int steps;                         // mode 1: min(size, log2 N) rotation steps
  // several tables over the same selectors (1 and unused strides for the one-table call)
  int tables;                        // tables of this pass: `lut` and `out` point at the first of them
  int out_tables;                    // tables of the whole call: out is [count][out_tables][N + 1]
  int group;                         // lut_tables_finish_kernel: tables per workgroup (the last group of a pass may hold fewer)
  size_t lut_stride;                 // words from one table to the next: n_luts * 2 * N
  // several outputs packed into one table (0 everywhere but in mosfhet_hip_leveled_lut_packed_batch)
  int pack_log;                      // lut_tables_finish_kernel: an entry is m = 2^pack_log adjacent coefficients; step i rotates by m 2^i, m extractions; out is [count][out_tables][m][N + 1]
};

// mode 4's transition entry of one (layer, state): the sources V_{t+1}[next0], V_{t+1}[next1] and the exponents of their rotations, in [0, 2N)
struct __attribute__((aligned(16))) LutStep {
  int next0, next1, rot0, rot1;
};
static_assert(sizeof(LutStep) == sizeof(d2), "a transition entry travels in the place of one complex slot");

// GADGET_OFFSET as a function: these kernels have always taken it through one, and the loop compiles differently as text in the kernel (cmux_steps.h)
__device__ __forceinline__ uint64_t lut_gadget_offset(int l, int Bg_bit) { return GADGET_OFFSET(l, Bg_bit); }

// Table preparation: block (j, r = q l + lv) of table blockIdx.y writes D[table][j][r] = DFT(digit lv of (table[j + half0] - table[j]).component q), slot order [m][thread].
template <class F>
__global__ __launch_bounds__(F::THREADS) void lut_prepare_kernel(LutParams p) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  __shared__ __attribute__((aligned(16))) d2 xch[F::XCH_SLOTS];
  const int t = threadIdx.x;
  const int rows = 2 * p.l;
  const int j = blockIdx.x / rows, r = blockIdx.x % rows, q = r / p.l, lv = r % p.l;
  F fft;
  fft_setup(fft, p.tw, t);
  const uint64_t off = lut_gadget_offset(p.l, p.Bg_bit);
  const uint64_t *__restrict__ lut = p.lut + (size_t)blockIdx.y * p.lut_stride;   // blockIdx.y: the table
  const uint64_t *__restrict__ lo = lut + ((size_t)j * 2 + q) * N, *__restrict__ hi = lut + ((size_t)(j + p.half0) * 2 + q) * N;
  double re[8], im[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    re[m] = Digits<1, 0>::digit(hi[m * T + t] - lo[m * T + t] + off, 0, 0, lv, p.Bg_bit);
    im[m] = Digits<1, 0>::digit(hi[M + m * T + t] - lo[M + m * T + t] + off, 0, 1, lv, p.Bg_bit);
  }
  fft.forward(re, im, xch, t);
  d2 *dst = p.dtab + (((size_t)blockIdx.y * p.half0 + (size_t)j) * rows + r) * M;
#pragma unroll
  for (int m = 0; m < 8; m++) dst[m * T + t] = d2{re[m], im[m]};
}

// Level 0: workgroup (slice, b) works for input b and walks the nodes u = slice, slice + slices, ... of ALL tables, u = table * half0 + j (every workgroup in the
// same direction, so the rows of D are shared through the L2s; the input is the slow index of the grid, so that the workgroups that read one input's selector run
// together); per node 2l complex multiply-add rows per output component, the inverse pair and the rounded addition onto the table row.
template <class F>
__global__ __launch_bounds__(F::THREADS, 2) void lut_level0_kernel(LutParams p) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  __shared__ __attribute__((aligned(16))) d2 xch[F::XCH_SLOTS];
  const int t = threadIdx.x;
  const int rows = 2 * p.l;
  const size_t b = blockIdx.y;
  F fft;
  fft_setup(fft, p.tw, t);
  const RoundCtx scale = round_scale<M>();
  const d2 *__restrict__ sel = p.sel + (((size_t)p.first + b) * p.size + (size_t)(p.size - 1)) * ((size_t)rows * 2 * M);
  const int nodes = p.tables * p.half0;
  for (int u = blockIdx.x; u < nodes; u += gridDim.x) {
    const int tb = u / p.half0, j = u - tb * p.half0;
    const d2 *__restrict__ drow = p.dtab + (size_t)u * rows * M;
    double o_re[2][8], o_im[2][8];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int m = 0; m < 8; m++) { o_re[c][m] = 0.0; o_im[c][m] = 0.0; }
#pragma unroll 1
    for (int r = 0; r < rows; r++) {
      const d2 *__restrict__ row = sel + (size_t)r * (2 * M);
      d2 x[8], k0[8], k1[8];
#pragma unroll
      for (int m = 0; m < 8; m++) x[m] = drow[(size_t)r * M + m * T + t];
#pragma unroll
      for (int m = 0; m < 8; m++) k0[m] = row[m * T + t];
#pragma unroll
      for (int m = 0; m < 8; m++) k1[m] = row[M + m * T + t];
#pragma unroll
      for (int m = 0; m < 8; m++) cmac(o_re[0][m], o_im[0][m], x[m].x, x[m].y, k0[m]);
#pragma unroll
      for (int m = 0; m < 8; m++) cmac(o_re[1][m], o_im[1][m], x[m].x, x[m].y, k1[m]);
    }
    fft.inverse2(o_re[0], o_im[0], o_re[1], o_im[1], xch, t);
    const uint64_t *__restrict__ base = p.lut + (size_t)tb * p.lut_stride + (size_t)j * 2 * N;
    uint64_t *dst = p.work + (b * nodes + (size_t)u) * 2 * N;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int m = 0; m < 8; m++) {
        dst[c * N + m * T + t] = add_rounded<true>(base[c * N + m * T + t], o_re[c][m], scale);
        dst[c * N + M + m * T + t] = add_rounded<true>(base[c * N + M + m * T + t], o_im[c][m], scale);
      }
  }
}

// sel (.) d by the TWO TEAMS of a workgroup (F::THREADS threads each), the form of pbs_wide_team_kernel with the gadget length as the loop bound: in phase ph team w
// owns row 2 ph + w (component q = row / l, digit row % l): its digits, its forward transform, the transformed digits handed over through its exchange buffer;
// then team w multiplies the phase's two rows with ITS output component of the selector -- in row order, the fma chain of cmux_rows starting from zero --
// and after the last phase runs the inverse transform of that component.  Critical path per product: l forward transforms + 1 inverse instead of 2l + 2.
// `home` (LDS, [2][N]): rotate -- the accumulator, d = (X^abar - 1) home; else the difference itself, or with `negate` its negative (every word 0 - home[j]).
// Leaves the inverse's output (unscaled) in o_re / o_im.
template <class F>
__device__ __forceinline__ void lut_team_product(const uint64_t *home, bool rotate, bool negate, int a_lo, bool flip, const d2 *__restrict__ sel, int l, int Bg_bit, uint64_t off,
                                                 const F &fft, d2 *xch_all, int team, int t, double (&o_re)[8], double (&o_im)[8]) {
  constexpr int N = F::N, M = F::M, T = F::THREADS;
  d2 *xch = xch_all + (size_t)team * F::XCH_SLOTS;
  const uint32_t mask = (1u << Bg_bit) - 1;
  const int half_bg = 1 << (Bg_bit - 1);
#pragma unroll
  for (int m = 0; m < 8; m++) { o_re[m] = 0.0; o_im[m] = 0.0; }
#pragma unroll 1
  for (int ph = 0; ph < l; ph++) {
    // this team's component of the phase's two selector rows: requested now, under the digit extraction and the forward transform
    d2 kk[2][8];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int m = 0; m < 8; m++) kk[r][m] = sel[(size_t)(2 * ph + r) * (2 * M) + (size_t)team * M + m * T + t];
    const int row = 2 * ph + team, q = row / l, shift = 64 - (row % l + 1) * Bg_bit;
    const uint64_t *hq = home + (size_t)q * N;
    double re[8], im[8];
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int j = m * T + t;
      const uint64_t d_lo = (rotate ? rot_coeff<N>(hq, j, a_lo, flip) - hq[j] : negate ? 0 - hq[j] : hq[j]) + off;
      const uint64_t d_hi = (rotate ? rot_coeff<N>(hq, j + M, a_lo, flip) - hq[j + M] : negate ? 0 - hq[j + M] : hq[j + M]) + off;
      re[m] = (double)((int)((uint32_t)(d_lo >> shift) & mask) - half_bg);
      im[m] = (double)((int)((uint32_t)(d_hi >> shift) & mask) - half_bg);
    }
    fft.forward(re, im, xch, t);
#pragma unroll
    for (int m = 0; m < 8; m++) xch[m * T + t] = d2{re[m], im[m]};
    workgroup_sync();
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const d2 *__restrict__ dr = xch_all + (size_t)r * F::XCH_SLOTS;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const d2 d = dr[m * T + t], k = kk[r][m];
        cmac(o_re[m], o_im[m], d.x, d.y, k);
      }
    }
    workgroup_sync();   // the transformed digits are consumed: the buffers are free for the next phase's exchanges / the inverse
  }
  fft.inverse(o_re, o_im, xch, t);   // (at N = 2048 workgroup barriers inside: both teams walk them)
}

// Workgroups of two teams (lut_team_product); dynamic LDS: two exchange buffers and [2][N] words (lut_cmux_lds<F>()).
// mode 0: persistent workgroups over the units (b, table, j) of one tree level below the first, in place: T[b][tb][j] += sel[b][sel_index] (.) (T[b][tb][j + half] - T[b][tb][j]).
//         Units touch disjoint rows (j < half <= j + half), so the order of the units does not matter.  The difference waits in LDS.
// mode 1: workgroup b finishes input b: acc = T[b][0] (the table's row 0 without a tree), `steps` times acc += sel[b][i] (.) ((X^(2N - 2^i) - 1) acc)
//         (src/bootstrap.c:107-122 with a[i] = int2torus(2N - 2^i, log2(2N)): never zero, no skipped step), then trlwe_extract_tlwe(acc, 0).
//         Both accumulator components stay in LDS across the steps.
// The per-input memories (capi_ram.inc; a memory is [2^size][2][N] words per input, the selectors are its address bits):
// mode 2: a level of a read, mode 0's step from one place to another: persistent workgroups over the units (b, j), j < half,
//         dst[b][j] = src[b][j] + sel[b][sel_index] (.) (src[b][j + half] - src[b][j]).  src = dst (a level in place in the workspace) is allowed: a unit reads
//         rows j and j + half and writes row j, which no other unit of the level reads.
// mode 3: a write: persistent workgroups over the units (b, cell i).  e = val[b] - cell in the [2][N] LDS words; for bit j of i, from the least significant:
//         bit 1: e = sel[b][j] (.) e;  bit 0: e = e + sel[b][j] (.) (-e);  then cell += e.  These are the words of the CMUX chain v = val[b]; bit 1:
//         v = cell + sel (.) (v - cell), bit 0: v = v + sel (.) (cell - v) with e = v - cell throughout (word arithmetic mod 2^64 is exact).  A thread reads its own 16
//         words of the cell in front of the chain and again behind it, where it stores them: held in registers across the products they are 32 registers on top of
//         the product's own, which at N = 2048 the 256 of a wavefront do not hold (28 bytes of scratch).  A unit reads and writes its own cell and reads val[b],
//         which nobody writes.
// The automata of capi_automaton.inc (a state vector is [states][2][N] words per input, selector t encrypts symbol t of the input's word):
// mode 4: one backward step: persistent workgroups over the units (b, j), j < half, state q = steps + j with the layer's entry e = dtab[q]:
//         dst[b][j] = R0 + sel[b][sel_index] (.) (R1 - R0), R0 = X^e.rot0 src[b][e.next0], R1 = X^e.rot1 src[b][e.next1].  R1 - R0 waits in LDS; R0 is rotated
//         again out of the source row at the store (its pointer and rotation are uniform: scalar registers, nothing of it is held across the product).  src and dst
//         are different buffers (any unit may read any source row): a unit writes one row of its own, no workgroup waits on or reads from another.
template <class F>
constexpr size_t lut_cmux_lds() { return sizeof(d2) * 2 * F::XCH_SLOTS + sizeof(uint64_t) * 2 * F::N; }

template <class F>
__global__ __launch_bounds__(2 * F::THREADS, 2) void lut_cmux_kernel(LutParams p) {
  constexpr int N = F::N, M = F::M, T = F::THREADS, WG = 2 * T;
  extern __shared__ __attribute__((aligned(16))) unsigned char lut_lds[];
  d2 *xch_all = reinterpret_cast<d2 *>(lut_lds);                                                 // [2][F::XCH_SLOTS]
  uint64_t *acc = reinterpret_cast<uint64_t *>(lut_lds + sizeof(d2) * 2 * F::XCH_SLOTS);         // [2][N]
  const int tid = threadIdx.x, team = __builtin_amdgcn_readfirstlane(tid / T), t = tid % T;
  const int l = p.l, Bg_bit = p.Bg_bit;
  F fft;
  fft_setup(fft, p.tw, t);
  const uint64_t off = lut_gadget_offset(l, Bg_bit);
  const RoundCtx scale = round_scale<M>();
  const size_t sel_sz = (size_t)2 * l * 2 * M;   // one selector, in complex slots
  double o_re[8], o_im[8];

  if (p.mode == 0) {
    const size_t units = (size_t)p.inputs * p.tables * p.half;
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
      const size_t bt = u / (size_t)p.half, j = u % (size_t)p.half, b = bt / (size_t)p.tables;   // bt = b * tables + table: the intermediates are [input][table][node]
      uint64_t *x = p.work + (bt * p.half0 + j) * 2 * N;   // (read and written by this unit alone)
      const uint64_t *y = x + (size_t)p.half * 2 * N;
      for (int w = tid; w < 2 * N; w += WG) acc[w] = y[w] - x[w];
      workgroup_sync();
      lut_team_product(acc, false, false, 0, false, p.sel + (((size_t)p.first + b) * p.size + (size_t)p.sel_index) * sel_sz, l, Bg_bit, off, fft, xch_all, team, t, o_re, o_im);
      uint64_t *xc = x + (size_t)team * N;                // this team's output component
#pragma unroll
      for (int m = 0; m < 8; m++) {
        xc[m * T + t] = add_rounded<true>(xc[m * T + t], o_re[m], scale);
        xc[M + m * T + t] = add_rounded<true>(xc[M + m * T + t], o_im[m], scale);
      }
      workgroup_sync();
    }
    return;
  }

  if (p.mode == 2) {
    const size_t units = (size_t)p.inputs * p.half;
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
      const size_t b = u / (size_t)p.half, j = u % (size_t)p.half;
      const uint64_t *x = p.lut + b * p.lut_stride + j * 2 * N;
      const uint64_t *y = x + (size_t)p.half * 2 * N;
      for (int w = tid; w < 2 * N; w += WG) acc[w] = y[w] - x[w];
      workgroup_sync();
      lut_team_product(acc, false, false, 0, false, p.sel + (((size_t)p.first + b) * p.size + (size_t)p.sel_index) * sel_sz, l, Bg_bit, off, fft, xch_all, team, t, o_re, o_im);
      const uint64_t *xc = x + (size_t)team * N;          // this team's output component
      uint64_t *dc = p.out + (b * p.half0 + j) * 2 * N + (size_t)team * N;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        dc[m * T + t] = add_rounded<true>(xc[m * T + t], o_re[m], scale);
        dc[M + m * T + t] = add_rounded<true>(xc[M + m * T + t], o_im[m], scale);
      }
      workgroup_sync();
    }
    return;
  }

  if (p.mode == 3) {
    const size_t units = (size_t)p.inputs << p.size;
    uint64_t *ec = acc + (size_t)team * N;                // this thread's 16 words of e: [m * T + t] and [M + m * T + t]
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
      const size_t b = u >> p.size;
      const unsigned cell_index = (unsigned)(u & (((size_t)1 << p.size) - 1));
      uint64_t *cc = p.out + u * 2 * N + (size_t)team * N;
      const uint64_t *vc = p.lut + b * 2 * N + (size_t)team * N;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        ec[m * T + t] = vc[m * T + t] - cc[m * T + t];
        ec[M + m * T + t] = vc[M + m * T + t] - cc[M + m * T + t];
      }
      workgroup_sync();
      for (int i = 0; i < p.size; i++) {
        const bool keep = (cell_index >> i) & 1;          // bit 1: e = sel (.) e;  bit 0: e = e + sel (.) (-e)
        lut_team_product(acc, false, !keep, 0, false, p.sel + (((size_t)p.first + b) * p.size + (size_t)i) * sel_sz, l, Bg_bit, off, fft, xch_all, team, t, o_re, o_im);
        // (every read of the old e stands in front of the last phase's barriers: the update below is this thread's own 16 words)
#pragma unroll
        for (int m = 0; m < 8; m++) {
          ec[m * T + t] = add_rounded<true>(keep ? 0 : ec[m * T + t], o_re[m], scale);
          ec[M + m * T + t] = add_rounded<true>(keep ? 0 : ec[M + m * T + t], o_im[m], scale);
        }
        workgroup_sync();
      }
#pragma unroll
      for (int m = 0; m < 8; m++) {
        cc[m * T + t] += ec[m * T + t];
        cc[M + m * T + t] += ec[M + m * T + t];
      }
      // (the next unit's first stores to e are again this thread's own words, read last by this thread)
    }
    return;
  }

  if (p.mode == 4) {
    const size_t units = (size_t)p.inputs * p.half;
    // through the constant address space: the handle's table is not written while a kernel runs, so an entry is one scalar load (as list_word of trace_kernels.h)
    typedef const LutStep __attribute__((address_space(4))) *const_steps_t;
    const const_steps_t table = (const_steps_t) reinterpret_cast<const LutStep *>(p.dtab);
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
      const size_t b = u / (size_t)p.half, j = u % (size_t)p.half;
      const size_t q = (size_t)p.steps + j;
      const LutStep e = {table[q].next0, table[q].next1, table[q].rot0, table[q].rot1};
      const uint64_t *vec = p.lut + b * p.lut_stride;
      const uint64_t *x = vec + (size_t)e.next0 * 2 * N, *y = vec + (size_t)e.next1 * 2 * N;
      const Rotation r0 = split_rotation(e.rot0, N), r1 = split_rotation(e.rot1, N);
      for (int w = tid; w < 2 * N; w += WG) {
        const int c = w / N, i = w & (N - 1);
        acc[w] = rot_coeff<N>(y + (size_t)c * N, i, r1.a_lo, r1.flip) - rot_coeff<N>(x + (size_t)c * N, i, r0.a_lo, r0.flip);
      }
      workgroup_sync();
      lut_team_product(acc, false, false, 0, false, p.sel + (((size_t)p.first + b) * p.size + (size_t)p.sel_index) * sel_sz, l, Bg_bit, off, fft, xch_all, team, t, o_re, o_im);
      const uint64_t *xc = x + (size_t)team * N;          // this team's output component
      uint64_t *dc = p.out + (b * p.half0 + j) * 2 * N + (size_t)team * N;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        dc[m * T + t] = add_rounded<true>(rot_coeff<N>(xc, m * T + t, r0.a_lo, r0.flip), o_re[m], scale);
        dc[M + m * T + t] = add_rounded<true>(rot_coeff<N>(xc, M + m * T + t, r0.a_lo, r0.flip), o_im[m], scale);
      }
      workgroup_sync();
    }
    return;
  }

  const size_t b = blockIdx.x;
  const uint64_t *src = p.half0 ? p.work + b * p.half0 * 2 * N : p.lut;
  for (int w = tid; w < 2 * N; w += WG) acc[w] = src[w];
  workgroup_sync();
  for (int i = 0; i < p.steps; i++) {
    const Rotation step = split_rotation(2 * N - (1 << i), N);
    lut_team_product(acc, true, false, step.a_lo, step.flip, p.sel + (((size_t)p.first + b) * p.size + (size_t)i) * sel_sz, l, Bg_bit, off, fft, xch_all, team, t,
                     o_re, o_im);
    // (every read of the old accumulator stands in front of the last phase's barriers: the update below is this thread's own 16 words)
    uint64_t *ac = acc + (size_t)team * N;
#pragma unroll
    for (int m = 0; m < 8; m++) {
      ac[m * T + t] = add_rounded<true>(ac[m * T + t], o_re[m], scale);
      ac[M + m * T + t] = add_rounded<true>(ac[M + m * T + t], o_im[m], scale);
    }
    workgroup_sync();
  }
  // src/trlwe.c:540-552 at idx = 0: a[0] = acc_a[0], a[j] = -acc_a[N - j]; b = acc_b[0]
  uint64_t *dst = p.out + ((size_t)p.first + b) * (size_t)(N + 1);
  for (int j = tid; j < N; j += WG) dst[j] = extract0_coeff(acc, j, N);
  if (tid == 0) dst[N] = acc[N];
}

// The finish for several tables over the same selectors.  Workgroups of two teams as above; dynamic LDS: the two exchange buffers and `group` accumulators of
// [2][N] words (lut_tables_finish_lds<F>(group)).  Workgroup (b, g) finishes tables g * group .. of input b: all accumulators are loaded, then the ROTATE STEP
// is the outer loop and the table the inner one -- selector i of input b comes from memory for the first table and from the caches for the others, and with
// it every table of the group takes exactly lut_cmux_kernel mode 1's step, so the words are those of the one-table finish whatever the grouping.
// With more than one group per input the block index is dealt so that the groups of an input -- consecutive units -- run on ONE die's share of the grid (blocks
// id and id + 8 share an L2): the groups of an input then meet its selectors in that L2.  Speed only; no word depends on the placement.
template <class F>
constexpr size_t lut_tables_finish_lds(int group) { return sizeof(d2) * 2 * F::XCH_SLOTS + sizeof(uint64_t) * 2 * F::N * (size_t)group; }
template <class F>
constexpr int lut_tables_max_group() { return (int)((160 * 1024 - sizeof(d2) * 2 * F::XCH_SLOTS) / (sizeof(uint64_t) * 2 * F::N)); }

template <class F>
__global__ __launch_bounds__(2 * F::THREADS, 2) void lut_tables_finish_kernel(LutParams p) {
  constexpr int N = F::N, M = F::M, T = F::THREADS, WG = 2 * T;
  extern __shared__ __attribute__((aligned(16))) unsigned char lut_lds[];
  d2 *xch_all = reinterpret_cast<d2 *>(lut_lds);                                                 // [2][F::XCH_SLOTS]
  uint64_t *accs = reinterpret_cast<uint64_t *>(lut_lds + sizeof(d2) * 2 * F::XCH_SLOTS);        // [group][2][N]
  const int tid = threadIdx.x, team = __builtin_amdgcn_readfirstlane(tid / T), t = tid % T;
  const int l = p.l, Bg_bit = p.Bg_bit;
  const int groups = (p.tables + p.group - 1) / p.group;
  const size_t units = (size_t)p.inputs * groups;
  size_t unit = blockIdx.x;
  if (groups > 1) {
    const size_t share = gridDim.x / 8;   // (the launcher rounds the grid up to a multiple of 8)
    unit = (blockIdx.x % 8) * share + blockIdx.x / 8;
  }
  if (unit >= units) return;
  const size_t b = unit / (size_t)groups;
  const int tb0 = (int)(unit % (size_t)groups) * p.group;
  const int nt = p.tables - tb0 < p.group ? p.tables - tb0 : p.group;
  F fft;
  fft_setup(fft, p.tw, t);
  const uint64_t off = lut_gadget_offset(l, Bg_bit);
  const RoundCtx scale = round_scale<M>();
  const size_t sel_sz = (size_t)2 * l * 2 * M;   // one selector, in complex slots
  double o_re[8], o_im[8];

  for (int k = 0; k < nt; k++) {
    const uint64_t *src = p.half0 ? p.work + (b * p.tables + (size_t)(tb0 + k)) * p.half0 * 2 * N : p.lut + (size_t)(tb0 + k) * p.lut_stride;
    for (int w = tid; w < 2 * N; w += WG) accs[(size_t)k * 2 * N + w] = src[w];
  }
  workgroup_sync();
  for (int i = 0; i < p.steps; i++) {
    const Rotation step = split_rotation(2 * N - (1 << (i + p.pack_log)), N);   // (the launcher keeps i + pack_log < log2 N)
    const d2 *__restrict__ sel = p.sel + (((size_t)p.first + b) * p.size + (size_t)i) * sel_sz;
#pragma unroll 1
    for (int k = 0; k < nt; k++) {
      uint64_t *acc = accs + (size_t)k * 2 * N;
      lut_team_product(acc, true, false, step.a_lo, step.flip, sel, l, Bg_bit, off, fft, xch_all, team, t, o_re, o_im);
      // (every read of the old accumulator stands in front of the last phase's barriers: the update below is this thread's own 16 words)
      uint64_t *ac = acc + (size_t)team * N;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        ac[m * T + t] = add_rounded<true>(ac[m * T + t], o_re[m], scale);
        ac[M + m * T + t] = add_rounded<true>(ac[M + m * T + t], o_im[m], scale);
      }
      workgroup_sync();
    }
  }
  // src/trlwe.c:540-552 at idx = e for the m = 2^pack_log outputs e of the selected entry, per table: a[j] = acc_a[e - j] for j <= e, else -acc_a[N + e - j];
  // b = acc_b[e].  out is [count][out_tables][m][N + 1].  Consecutive threads read consecutive LDS words downwards (no bank conflict) and write consecutive
  // global words.  (e - j) & (N - 1) is e - j for j <= e and N + e - j behind it; at m = 1 this is the extraction at idx 0.
  const int m_out = 1 << p.pack_log;
  for (int k = 0; k < nt; k++) {
    const uint64_t *acc = accs + (size_t)k * 2 * N;
    uint64_t *dst = p.out + ((((size_t)p.first + b) * p.out_tables + (size_t)(tb0 + k)) << p.pack_log) * (size_t)(N + 1);
    for (int e = 0; e < m_out; e++, dst += N + 1) {
      for (int j = tid; j < N; j += WG) {
        const uint64_t w = acc[(e - j) & (N - 1)];
        dst[j] = (j <= e) ? w : (0 - w);
      }
      if (tid == 0) dst[N] = acc[N + e];
    }
  }
}

}  // namespace mosfhet
