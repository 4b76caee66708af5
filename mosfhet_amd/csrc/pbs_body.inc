// pbs_body.inc -- the body of pbs_kernel (G = 1) and pbs_group_kernel (G > 1), bootstrap_kernels.h: included inside the kernel, behind
// F, L, BG, BYC, G, p and parked.
  static_assert(!BYC || (F::N == 2048 && L % 2 == 0), "the by-component order exists where pbs_split_kernel does");
  static_assert(G == 1 || (F::THREADS == 64 && !BYC), "several teams per workgroup: their transforms must not use workgroup barriers");
  constexpr int N = F::N, M = F::M, T = F::THREADS, LOG2N2 = F::LOGM + 2;
  constexpr bool kReduce = kProductNeedsReduce<F, L, BG>;
  // SET_1's instantiation (G = 1 and G > 1) keeps both accumulator components NEGATED, -acc mod 2^64, from the first load to the last store: the digits then take
  // rot(acc) + (-acc[j]) + off and the step's tail (-acc) + (-increment), each by one carry-free 64-bit add, where +acc needs a 64-bit subtract for the digits and a
  // carry chain for the tail (cmux_digits: NEG; neg_rounded).  Component b's add is done by the LDS unit (a 64-bit DS add without return, on the team's own slice:
  // DS operations of a wavefront execute in order, as wave_lds_sync relies on).  Same increments, same bits.  The one switch:
#ifndef MOSFHET_PBS_NEGACC
#define MOSFHET_PBS_NEGACC 1
#endif
  constexpr bool kNegAcc = MOSFHET_PBS_NEGACC && F::N == 1024 && L == 2 && BG == 8 && !kReduce && !BYC;
  // On top of it the digit words take the rotation's sign and index from one 11-bit subtraction, apply the sign by two XORs around the carry-free add, and keep
  // the high dword as it is: raw byte fields, the reference's digit formula (cmux_digits: SF; Digits: RAW).  Same digits.  The one switch (0: the kernels as before):
#ifndef MOSFHET_PBS_SIGNFREE
#define MOSFHET_PBS_SIGNFREE 1
#endif
  constexpr bool kSignFree = kNegAcc && MOSFHET_PBS_SIGNFREE;
  // (G > 1: one slice per team, its xch and acc1 side by side, so that every LDS address of a team is the G = 1 address plus one team offset)
  constexpr int kSlice = (int)sizeof(d2) * F::XCH_SLOTS + (int)sizeof(uint64_t) * N;
  __shared__ __attribute__((aligned(16))) d2 xch_all[G == 1 ? F::XCH_SLOTS : G * kSlice / (int)sizeof(d2)];
  __shared__ __attribute__((aligned(16))) uint64_t acc1_one[G == 1 ? N : 1];
  const int team = G == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x / T));   // wave-uniform: the ciphertext's words stay scalar loads
  // (G > 1: the lane index from the hardware, so that threadIdx.x is not held over the step loop next to it)
  const int t = G == 1 ? (int)threadIdx.x : (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  d2 *xch = G == 1 ? xch_all : xch_all + team * (kSlice / (int)sizeof(d2));
  uint64_t *acc1 = G == 1 ? acc1_one : reinterpret_cast<uint64_t *>(xch + F::XCH_SLOTS);
  const size_t b_own = (size_t)blockIdx.x * G + team;
  const bool live = G == 1 || b_own < (size_t)p.group_count;
  const size_t b = live ? b_own : (size_t)p.group_count - 1;   // a team past the end of a ragged workgroup: the last ciphertext's work, nothing stored
  const uint64_t *__restrict__ ct = p.in + (p.rows > 1 ? b / (size_t)p.rows : b) * (size_t)(p.n + 1);
  const int Bg_bit = BG > 0 ? BG : p.Bg_bit;

  F fft;
  fft_setup(fft, p.tw, t);

  uint64_t al[8], ah[8];
  if (p.skip_init) {
    const uint64_t *src = p.out + b * (size_t)(2 * N);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      al[m] = kNegAcc ? 0 - src[m * T + t] : src[m * T + t];
      ah[m] = kNegAcc ? 0 - src[M + m * T + t] : src[M + m * T + t];
      acc1[m * T + t] = kNegAcc ? 0 - src[N + m * T + t] : src[N + m * T + t];
      acc1[M + m * T + t] = kNegAcc ? 0 - src[N + M + m * T + t] : src[N + M + m * T + t];
    }
  } else {
    // src/bootstrap.c:194-195: acc = tv * X^(2N - bbar), gathered straight from global memory
    const uint64_t *__restrict__ tv = p.rows > 1 ? p.tv + (b % (size_t)p.rows) * (size_t)(2 * N) : p.tv + b * (size_t)p.tv_stride;
    const uint32_t bbar = modswitch<LOG2N2>(pbs_pre(ct[p.n], p, LOG2N2) + p.prec_offset);
    // (kNegAcc: -(tv X^r) = tv X^(r + N))
    const int rot = (2 * N - (int)bbar + (kNegAcc ? N : 0)) & (2 * N - 1);
    const auto [a_lo, flip] = split_rotation(rot, N);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      al[m] = rot_coeff<N>(tv, m * T + t, a_lo, flip);
      ah[m] = rot_coeff<N>(tv, M + m * T + t, a_lo, flip);
      acc1[m * T + t] = rot_coeff<N>(tv + N, m * T + t, a_lo, flip);
      acc1[M + m * T + t] = rot_coeff<N>(tv + N, M + m * T + t, a_lo, flip);
    }
  }
  F::sync();

  const uint64_t off = GADGET_OFFSET(L, Bg_bit);
  const RoundCtx scale = round_scale<M>();
  const size_t row_sz = (size_t)2 * L * 2 * M;

  int next_meet = __builtin_amdgcn_readfirstlane(G > 1 && p.phase_every > 0 ? 0 : -1);
  for (int i = 0; i < p.n; i++) {
    if (T > 64 && p.pace && i > 0 && i % p.pace_every == 0) pace_teams(p.pace, (unsigned)(i / p.pace_every), t, p.pace_limit);   // (before the skip: every team counts every step)
    if constexpr (G > 1) {   // (before the skip as well: i, n and phase_every are launch-uniform, the skip is not)
      if (i == next_meet) { workgroup_sync(); next_meet = __builtin_amdgcn_readfirstlane(next_meet + p.phase_every); }
    }
    // (G > 1: the mask word through the constant address space -- the input is not written while the kernel runs -- so that it is a scalar load with no vector
    // register and no vmcnt wait of its own in front of the step)
    typedef const uint64_t __attribute__((address_space(4))) *const_words_t;
    const uint64_t a_i = G == 1 ? ct[i] : ((const_words_t)ct)[i];
    int abar = (int)modswitch<LOG2N2>(pbs_pre(a_i, p, LOG2N2));
    if constexpr (G > 1) asm volatile("" : "+s"(abar));   // (the skip test on the scalar unit: as a 64-bit compare against a constant it holds two vector registers over the loop)
    if (abar == 0) continue;  // src/bootstrap.c:114
    const d2 *__restrict__ bkrow = p.bk + (size_t)i * row_sz;
    const Rotation step = split_rotation(abar, N);
    const int a_lo = step.a_lo;
    const bool flip = step.flip != kNegAcc;   // (kNegAcc: what is rotated is -acc, the digits want +rot(acc))
    double o_re[2][8], o_im[2][8];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int m = 0; m < 8; m++) { o_re[c][m] = 0.0; o_im[c][m] = 0.0; }
    {
      constexpr int kUnrollQ = L == 1 ? 2 : 1;
#pragma unroll kUnrollQ
      for (int q = 0; q < 2; q++) {
        typename Digits<L, BG>::word_t w_lo[8], w_hi[8];
        uint32_t ext[8];
        cmux_digits<F, L, BG, kNegAcc, kSignFree>(w_lo, w_hi, ext, al, ah, q ? acc1 : nullptr, xch, a_lo, flip, off, t);
        // rows two at a time where the transform keeps its pass twiddles in LDS (tools/ab/pbs_ab.hip -DAB_LTW instantiates that) -- at two wavefronts per SIMD
        // the pairs gain nothing here (experiments/README.md round 4): production instantiates pbs_kernel on the register-twiddle transforms
        if constexpr (F::kLtw && F::kForward2 && L % 2 == 0) cmux_rows2<F, L, BG>(w_lo, w_hi, ext, q, o_re, o_im, xch, fft, bkrow, Bg_bit, t);
        else cmux_rows<F, L, BG, false, kSignFree>(w_lo, w_hi, ext, q, o_re, o_im, xch, fft, bkrow, Bg_bit, t);
        if constexpr (BYC) {
          // (the slot addresses are made inside the step: hoisted out of the loop over the key they would hold 32 registers and spill, like cmux_digits' rotated addresses)
          int here = 0;
          asm volatile("" : "+s"(here));
          d2 *__restrict__ mine = reinterpret_cast<d2 *>(parked.park) + (size_t)blockIdx.x * (16 * T) + here + t;
          if (q == 0) {   // S_0 is parked; S_1 starts from zero
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
              for (int m = 0; m < 8; m++) {
                mine[(c * 8 + m) * T] = d2{o_re[c][m], o_im[c][m]};
                o_re[c][m] = 0.0;
                o_im[c][m] = 0.0;
              }
          } else {        // S_0 + S_1
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
              for (int m = 0; m < 8; m++) {
                const d2 s0 = mine[(c * 8 + m) * T];
                o_re[c][m] = s0.x + o_re[c][m];
                o_im[c][m] = s0.y + o_im[c][m];
              }
          }
        }
      }
    }
    fft.inverse2(o_re[0], o_im[0], o_re[1], o_im[1], xch, t);
    if constexpr (kNegAcc) {
#pragma unroll
      for (int m = 0; m < 8; m++) {
        al[m] = add_pairs(neg_rounded(o_re[0][m], scale), al[m]);
        ah[m] = add_pairs(neg_rounded(o_im[0][m], scale), ah[m]);
      }
#pragma unroll
      for (int m = 0; m < 8; m++) {
        // (ds_add_u64, nothing returned: no read to wait for at the end of the step, and the next step's reads of acc1 stand behind it in the wavefront's DS order)
        (void)__hip_atomic_fetch_add(&acc1[m * T + t], neg_rounded(o_re[1][m], scale), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        (void)__hip_atomic_fetch_add(&acc1[M + m * T + t], neg_rounded(o_im[1][m], scale), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
    } else {
#pragma unroll
      for (int m = 0; m < 8; m++) {
        al[m] = add_rounded<kReduce>(al[m], o_re[0][m], scale);
        ah[m] = add_rounded<kReduce>(ah[m], o_im[0][m], scale);
      }
#pragma unroll
      for (int m = 0; m < 8; m++) {
        acc1[m * T + t] = add_rounded<kReduce>(acc1[m * T + t], o_re[1][m], scale);
        acc1[M + m * T + t] = add_rounded<kReduce>(acc1[M + m * T + t], o_im[1][m], scale);
      }
    }
    F::sync();
  }

  if (!live) return;   // (behind the last barrier)
  int te = t;
  if constexpr (G > 1) {   // (the lane index anew, so that the addresses of the stores below are made here and not held over the step loop)
    unsigned ones = ~0u;
    asm volatile("" : "+s"(ones));
    te = (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
  }
  if (p.extract) {
    // src/trlwe.c:540-552 at idx = 0: a[0] = acc_a[0], a[j] = -acc_a[N - j]; b = acc_b[0]
    uint64_t *st = reinterpret_cast<uint64_t *>(xch);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      st[m * T + te] = al[m];
      st[M + m * T + te] = ah[m];
    }
    F::sync();
    uint64_t *dst = p.out + b * (size_t)(N + 1);
    // (kNegAcc: the resident words are already -acc_a; only a[0] and b are negated back)
    if constexpr (kNegAcc) {
      for (int j = te; j < N; j += T) dst[j] = (j == 0) ? (0 - st[0]) : st[N - j];
      if (te == 0) dst[N] = 0 - acc1[0];
    } else {
      for (int j = te; j < N; j += T) dst[j] = extract0_coeff(st, j, N);
      if (te == 0) dst[N] = acc1[0];
    }
  } else {
    uint64_t *dst = p.out + b * (size_t)(2 * N);
#pragma unroll
    for (int m = 0; m < 8; m++) {
      dst[m * T + te] = kNegAcc ? 0 - al[m] : al[m];
      dst[M + m * T + te] = kNegAcc ? 0 - ah[m] : ah[m];
      dst[N + m * T + te] = kNegAcc ? 0 - acc1[m * T + te] : acc1[m * T + te];
      dst[N + M + m * T + te] = kNegAcc ? 0 - acc1[M + m * T + te] : acc1[M + m * T + te];
    }
  }
