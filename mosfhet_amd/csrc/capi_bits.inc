// capi_bits.inc -- an n-bit -> m-bit function on inputs given as LWE-encrypted bits, LWE-encrypted bits out: circuit bootstrap + vertical packing of CGGI, the loop
// the reference's leveled application runs per input (applications/leveled_lut/main.c: circuit_bootstrap_3 src/bootstrap.c:346-366, trgsw_to_DFT src/trgsw.c:345-349,
// eval_LUT vertical_packing.c:36-52, tlwe_keyswitch src/tlwe.c:289-320) as ONE call over a batch.  Own code: nothing of the reference is compiled in.
//
// The selectors are an internal, bounded workspace: the circuit bootstrap writes them in the DFT domain directly (trlwe_fft_keyswitch_kernel mode 3,
// bootstrap_kernels.h), one chunk of whole inputs at a time, into the calling thread's pool (slot POOL_BITS); the leveled LUT reads them from there.

// mosfhet_hip_circuit_bootstrap_3_dft_batch: circuit_bootstrap_3 followed by trgsw_to_DFT (src/bootstrap.c:346-366, src/trgsw.c:345-349) without the torus-domain
// TRGSW in between.  Same checks, same bootstrap launch, same choice between one packing switch for all levels and one per level as circuit_bootstrap_3_batch.
extern "C" int mosfhet_hip_circuit_bootstrap_3_dft_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, double *d_out_dft,
                                                         const uint64_t *d_in, int count, void *stream) {
  return circuit_bootstrap_3_run("circuit_bootstrap_3_dft", ctx, bsk, kska, kskb, nullptr, reinterpret_cast<d2 *>(d_out_dft), d_in, count, stream, nullptr);
}

// Selector workspace bound: the selectors [chunk][size][2l][2][N/2] complex of one chunk of inputs stay within it (one input always runs).  Results of a key with a
// set product order do not depend on it.  2 GiB: 8192 bits at lvl2's gadget, and the circuit bootstrap keeps its full-batch kernels from 1024 bits on.
constexpr long long BITS_WORKSPACE_DEFAULT = 2ll << 30;
static std::atomic<long long> g_bits_workspace{BITS_WORKSPACE_DEFAULT};
constexpr long long BITS_MAX_LAUNCH = 1ll << 20;   // bits per circuit-bootstrap launch at most, whatever the bound (grids and staging sizes stay far inside int)

extern "C" int mosfhet_hip_set_lut_bits_workspace(long long bytes) {
  if (bytes < 0) return fail(MOSFHET_HIP_EINVAL, "set_lut_bits_workspace: bytes = %lld (0 restores the default)", bytes);
  g_bits_workspace = bytes ? bytes : BITS_WORKSPACE_DEFAULT;
  return MOSFHET_HIP_OK;
}

struct BitsPlan { int chunk, chunks, cb_bits; long long sel_bytes; LutTablesPlan lut; };

// The one place that decides the shape of a lut_bits call: for the launcher and for mosfhet_hip_lut_bits_plan.
static int bits_plan(const char *who, int N, int l, int size, int tables, int count, int cus, BitsPlan *r) {
  LutTablesPlan whole;
  int rc = lut_tables_plan(who, N, l, size, tables, count, cus, &whole);   // the argument checks of the LUT call
  if (rc) return rc;
  const long long per_input = (long long)size * 2 * l * 2 * (N / 2) * (long long)sizeof(d2);
  long long fit = g_bits_workspace.load(std::memory_order_relaxed) / per_input;
  if (fit > BITS_MAX_LAUNCH / size) fit = BITS_MAX_LAUNCH / size;
  r->chunk = fit < 1 ? 1 : (fit < count ? (int)fit : count);
  r->chunks = (count + r->chunk - 1) / r->chunk;
  r->cb_bits = r->chunk * size;
  r->sel_bytes = (long long)r->chunk * per_input;
  return lut_tables_plan(who, N, l, size, tables, r->chunk, cus, &r->lut);
}

extern "C" int mosfhet_hip_lut_bits_plan(int N, int l, int size, int tables, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "lut_bits_plan: null plan");
  BitsPlan r;
  const int rc = bits_plan("lut_bits_plan", N, l, size, tables, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.chunk; plan[1] = r.chunks; plan[2] = r.sel_bytes; plan[3] = r.cb_bits;
  plan[4] = r.lut.levels; plan[5] = r.lut.nodes; plan[6] = r.lut.chunk; plan[7] = r.lut.pass; plan[8] = r.lut.bytes; plan[9] = r.lut.group;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_lut_bits_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out,
                                          uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int count, void *stream) {
  // (null handles and scalar ranges come before any handle is dereferenced and before any HIP call)
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "lut_bits: null ctx");
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "lut_bits: null bsk");
  if (!kska) return fail(MOSFHET_HIP_EINVAL, "lut_bits: null kska");
  if (!kskb) return fail(MOSFHET_HIP_EINVAL, "lut_bits: null kskb");
  if (size < 1 || size > 11 + MOSFHET_HIP_LUT_MAX_LEVELS)
    return fail(MOSFHET_HIP_EINVAL, "lut_bits: size = %d (1 .. log2 N + %d selector bits, N <= 2048)", size, MOSFHET_HIP_LUT_MAX_LEVELS);
  if (tables < 1 || tables > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "lut_bits: tables = %d (1 .. %d)", tables, MOSFHET_HIP_LUT_MAX_TABLES);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "lut_bits: count = %d", count);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_luts || !d_in) return fail(MOSFHET_HIP_EINVAL, "lut_bits: null buffer");
  TUNED_ONLY(bsk, "lut_bits");
  const int N = bsk->N, n = bsk->n, l = bsk->l, Bg_bit = bsk->Bg_bit;
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "lut_bits: bsk: ring degree N = %d not supported here (1024, 2048)", N);
  if (Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "lut_bits: bsk: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", l, Bg_bit);
  BitsPlan plan;
  int rc = bits_plan("lut_bits", N, l, size, tables, count, 256, &plan);
  if (rc) return rc;
  if (kska->entries != 2 || kska->N != N) return fail(MOSFHET_HIP_EINVAL, "lut_bits: kska must be the 2-entry private key-switch set for N");
  if (kskb->row != 2 * N || kskb->b_word != N || kskb->n_in != N) return fail(MOSFHET_HIP_EINVAL, "lut_bits: kskb must be a packing key N -> TRLWE(N)");
  if (N % (2 * l)) return fail(MOSFHET_HIP_EINVAL, "lut_bits: N not divisible by 2l");
  if (ksk_out) {
    if (ksk_out->b_word != ksk_out->n_out) return fail(MOSFHET_HIP_EINVAL, "lut_bits: ksk_out is a packing (LWE -> TRLWE) key, not an LWE -> LWE key");
    if (ksk_out->n_in != N || ksk_out->n_out != n)
      return fail(MOSFHET_HIP_EINVAL, "lut_bits: ksk_out switches %d -> %d, the outputs need N = %d -> bsk's n = %d", ksk_out->n_in, ksk_out->n_out, N, n);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t sel_words = (size_t)(plan.sel_bytes / (long long)sizeof(uint64_t)), lut_words = ksk_out ? (size_t)plan.chunk * tables * ((size_t)N + 1) : 0;
  uint64_t *ws = nullptr;
  if ((rc = pool_get(ctx->device, POOL_BITS, sel_words + lut_words, &ws))) return rc;
  d2 *sel = reinterpret_cast<d2 *>(ws);
  uint64_t *lut_out = ws + sel_words;
  const size_t out_row = ksk_out ? (size_t)n + 1 : (size_t)N + 1;
  for (int first = 0; first < count; first += plan.chunk) {
    const int inputs = count - first < plan.chunk ? count - first : plan.chunk;
    if ((rc = circuit_bootstrap_3_run("lut_bits", ctx, bsk, kska, kskb, nullptr, sel, d_in + (size_t)first * size * ((size_t)n + 1), inputs * size, stream, nullptr))) return rc;
    uint64_t *dst = d_out + (size_t)first * tables * out_row;
    if ((rc = mosfhet_hip_leveled_lut_tables_batch(ctx, ksk_out ? lut_out : dst, reinterpret_cast<const double *>(sel), d_luts, size, N, l, Bg_bit, tables, inputs, stream)))
      return rc;
    if (ksk_out && (rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, ksk_out, dst, lut_out, inputs * tables, stream))) return rc;
  }
  return MOSFHET_HIP_OK;
}

// ---------------------------------------------------------------- several outputs packed into one table ----------------------------------------------------------------
// mosfhet_hip_lut_bits_packed_batch: the same round with mosfhet_hip_leveled_lut_packed_batch as its middle: `tables` tables of m = 2^pack_log output bits per entry,
// tables * m output bits per input.  The selector workspace is that of lut_bits (`size` selectors per input); the staging in front of the output key switch is
// [chunk][tables * m][N + 1].

struct BitsPackedPlan { int chunk, chunks, cb_bits; long long sel_bytes; LutPackedPlan lut; };

// The one place that decides the shape of a lut_bits_packed call: for the launcher and for mosfhet_hip_lut_bits_packed_plan.
static int bits_packed_plan(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, BitsPackedPlan *r) {
  LutPackedPlan whole;
  int rc = lut_packed_plan(who, N, l, size, tables, pack_log, count, cus, &whole);   // the argument checks of the LUT call
  if (rc) return rc;
  // the chunks are lut_bits': they depend on `size` selectors per input alone.  (bits_plan's own LUT plan is the unpacked one of `size`, whose tree is never
  // deeper than the packed one that just passed; it is not used.)
  BitsPlan cut;
  if ((rc = bits_plan(who, N, l, size, tables, count, cus, &cut))) return rc;
  r->chunk = cut.chunk; r->chunks = cut.chunks; r->cb_bits = cut.cb_bits; r->sel_bytes = cut.sel_bytes;
  return lut_packed_plan(who, N, l, size, tables, pack_log, r->chunk, cus, &r->lut);
}

extern "C" int mosfhet_hip_lut_bits_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed_plan: null plan");
  BitsPackedPlan r;
  const int rc = bits_packed_plan("lut_bits_packed_plan", N, l, size, tables, pack_log, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.chunk; plan[1] = r.chunks; plan[2] = r.sel_bytes; plan[3] = r.cb_bits;
  plan[4] = r.lut.t.levels; plan[5] = r.lut.t.nodes; plan[6] = r.lut.t.chunk; plan[7] = r.lut.t.pass; plan[8] = r.lut.t.bytes; plan[9] = r.lut.t.group;
  plan[10] = r.lut.steps; plan[11] = r.lut.outputs;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_lut_bits_packed_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out,
                                                 uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int pack_log, int count, void *stream) {
  // (null handles and scalar ranges come before any handle is dereferenced and before any HIP call)
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: null ctx");
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: null bsk");
  if (!kska) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: null kska");
  if (!kskb) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: null kskb");
  if (pack_log < 0 || pack_log > 10) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: pack_log = %d (0 .. log2 N - 1, N <= 2048)", pack_log);
  if (size < 1 || size + pack_log > 11 + MOSFHET_HIP_LUT_MAX_LEVELS)
    return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: size = %d with pack_log = %d (size >= 1, size + pack_log <= log2 N + %d, N <= 2048)", size, pack_log, MOSFHET_HIP_LUT_MAX_LEVELS);
  if (tables < 1 || tables > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: tables = %d (1 .. %d)", tables, MOSFHET_HIP_LUT_MAX_TABLES);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: count = %d", count);
  if (pack_log == 0) return mosfhet_hip_lut_bits_batch(ctx, bsk, kska, kskb, ksk_out, d_out, d_luts, d_in, size, tables, count, stream);   // one output per entry: that call
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_luts || !d_in) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: null buffer");
  TUNED_ONLY(bsk, "lut_bits_packed");
  const int N = bsk->N, n = bsk->n, l = bsk->l, Bg_bit = bsk->Bg_bit;
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: bsk: ring degree N = %d not supported here (1024, 2048)", N);
  if (Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: bsk: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", l, Bg_bit);
  BitsPackedPlan plan;
  int rc = bits_packed_plan("lut_bits_packed", N, l, size, tables, pack_log, count, 256, &plan);
  if (rc) return rc;
  if (kska->entries != 2 || kska->N != N) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: kska must be the 2-entry private key-switch set for N");
  if (kskb->row != 2 * N || kskb->b_word != N || kskb->n_in != N) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: kskb must be a packing key N -> TRLWE(N)");
  if (N % (2 * l)) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: N not divisible by 2l");
  if (ksk_out) {
    if (ksk_out->b_word != ksk_out->n_out) return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: ksk_out is a packing (LWE -> TRLWE) key, not an LWE -> LWE key");
    if (ksk_out->n_in != N || ksk_out->n_out != n)
      return fail(MOSFHET_HIP_EINVAL, "lut_bits_packed: ksk_out switches %d -> %d, the outputs need N = %d -> bsk's n = %d", ksk_out->n_in, ksk_out->n_out, N, n);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const int outputs = plan.lut.outputs;   // tables * m output bits per input
  const size_t sel_words = (size_t)(plan.sel_bytes / (long long)sizeof(uint64_t)), lut_words = ksk_out ? (size_t)plan.chunk * outputs * ((size_t)N + 1) : 0;
  uint64_t *ws = nullptr;
  if ((rc = pool_get(ctx->device, POOL_BITS, sel_words + lut_words, &ws))) return rc;
  d2 *sel = reinterpret_cast<d2 *>(ws);
  uint64_t *lut_out = ws + sel_words;
  const size_t out_row = ksk_out ? (size_t)n + 1 : (size_t)N + 1;
  for (int first = 0; first < count; first += plan.chunk) {
    const int inputs = count - first < plan.chunk ? count - first : plan.chunk;
    if ((rc = circuit_bootstrap_3_run("lut_bits_packed", ctx, bsk, kska, kskb, nullptr, sel, d_in + (size_t)first * size * ((size_t)n + 1), inputs * size, stream, nullptr))) return rc;
    uint64_t *dst = d_out + (size_t)first * outputs * out_row;
    if ((rc = mosfhet_hip_leveled_lut_packed_batch(ctx, ksk_out ? lut_out : dst, reinterpret_cast<const double *>(sel), d_luts, size, N, l, Bg_bit, tables, pack_log, inputs,
                                                   stream)))
      return rc;
    if (ksk_out && (rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, ksk_out, dst, lut_out, inputs * outputs, stream))) return rc;
  }
  return MOSFHET_HIP_OK;
}
