// capi_bits.inc -- an n-bit -> m-bit function on inputs given as LWE-encrypted bits, LWE-encrypted bits out: circuit bootstrap + vertical packing of CGGI, the loop
// the reference's leveled application runs per input (applications/leveled_lut/main.c: circuit_bootstrap_3 src/bootstrap.c:346-366, trgsw_to_DFT src/trgsw.c:345-349,
// eval_LUT vertical_packing.c:36-52, tlwe_keyswitch src/tlwe.c:289-320) as ONE call over a batch.  Own code: nothing of the reference is compiled in.
//
// Two entry points, one path (bits_plan, lut_bits_run): mosfhet_hip_lut_bits_batch (`tables` one-bit tables) is mosfhet_hip_lut_bits_packed_batch (`tables` tables
// of m = 2^pack_log output bits per entry, tables * m output bits per input) at pack_log = 0.
//
// The selectors are an internal, bounded workspace: the circuit bootstrap writes them in the DFT domain directly (trlwe_fft_keyswitch_kernel mode 3,
// bootstrap_kernels.h), one chunk of whole inputs at a time, into the calling thread's pool (slot POOL_BITS); the leveled LUT (leveled_lut_run, capi_lut.inc) reads
// them from there.  Behind them in the same slot, when there is an output key: the staging [chunk][tables * m][N + 1] in front of the output key switch.

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

struct BitsPlan { int chunk, chunks, cb_bits; long long sel_bytes; LutPlan lut; };

// The one place that decides the shape of a call: for the launcher and for the two mosfhet_hip_lut_bits*_plan functions.
static int bits_plan(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, BitsPlan *r) {
  int rc = lut_plan(who, N, l, size, tables, pack_log, count, cus, &r->lut);   // the argument checks of the LUT call, on the whole batch
  if (rc) return rc;
  const long long per_input = (long long)size * 2 * l * 2 * (N / 2) * (long long)sizeof(d2);   // the chunks depend on `size` selectors per input alone
  long long fit = g_bits_workspace.load(std::memory_order_relaxed) / per_input;
  if (fit > BITS_MAX_LAUNCH / size) fit = BITS_MAX_LAUNCH / size;
  r->chunk = fit < 1 ? 1 : (fit < count ? (int)fit : count);
  r->chunks = (count + r->chunk - 1) / r->chunk;
  r->cb_bits = r->chunk * size;
  r->sel_bytes = (long long)r->chunk * per_input;
  return lut_plan(who, N, l, size, tables, pack_log, r->chunk, cus, &r->lut);
}

// plan[0 .. 4) the chunks, then the LUT plan of one chunk: 6 fields for one-bit tables, 8 for packed tables
static int bits_plan_fields(const char *who, int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan, int lut_fields) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "%s: null plan", who);
  BitsPlan r;
  const int rc = bits_plan(who, N, l, size, tables, pack_log, count, cus, &r);
  if (rc) return rc;
  plan[0] = r.chunk; plan[1] = r.chunks; plan[2] = r.sel_bytes; plan[3] = r.cb_bits;
  plan[4] = r.lut.levels; plan[5] = r.lut.nodes; plan[6] = r.lut.chunk; plan[7] = r.lut.pass; plan[8] = r.lut.bytes; plan[9] = r.lut.group;
  if (lut_fields == 8) { plan[10] = r.lut.steps; plan[11] = r.lut.outputs; }
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_lut_bits_plan(int N, int l, int size, int tables, int count, int cus, long long *plan) {
  return bits_plan_fields("lut_bits_plan", N, l, size, tables, 0, count, cus, plan, 6);
}

extern "C" int mosfhet_hip_lut_bits_packed_plan(int N, int l, int size, int tables, int pack_log, int count, int cus, long long *plan) {
  return bits_plan_fields("lut_bits_packed_plan", N, l, size, tables, pack_log, count, cus, plan, 8);
}

// The body of both calls.  Null handles and scalar ranges come before any handle is dereferenced and before any HIP call.
static int lut_bits_run(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out,
                        uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int pack_log, int count, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!bsk) return fail(MOSFHET_HIP_EINVAL, "%s: null bsk", who);
  if (!kska) return fail(MOSFHET_HIP_EINVAL, "%s: null kska", who);
  if (!kskb) return fail(MOSFHET_HIP_EINVAL, "%s: null kskb", who);
  if (pack_log < 0 || pack_log > 10) return fail(MOSFHET_HIP_EINVAL, "%s: pack_log = %d (0 .. log2 N - 1, N <= 2048)", who, pack_log);
  if (size < 1 || size + pack_log > 11 + MOSFHET_HIP_LUT_MAX_LEVELS)
    return fail(MOSFHET_HIP_EINVAL, "%s: size = %d with pack_log = %d (size >= 1, size + pack_log <= log2 N + %d, N <= 2048)", who, size, pack_log, MOSFHET_HIP_LUT_MAX_LEVELS);
  if (tables < 1 || tables > MOSFHET_HIP_LUT_MAX_TABLES) return fail(MOSFHET_HIP_EINVAL, "%s: tables = %d (1 .. %d)", who, tables, MOSFHET_HIP_LUT_MAX_TABLES);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_luts || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  TUNED_ONLY(bsk, who);
  const int N = bsk->N, n = bsk->n, l = bsk->l, Bg_bit = bsk->Bg_bit;
  if (N != 1024 && N != 2048) return fail(MOSFHET_HIP_EINVAL, "%s: bsk: ring degree N = %d not supported here (1024, 2048)", who, N);
  if (Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bsk: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  BitsPlan plan;
  int rc = bits_plan(who, N, l, size, tables, pack_log, count, 256, &plan);
  if (rc) return rc;
  if (kska->entries != 2 || kska->N != N) return fail(MOSFHET_HIP_EINVAL, "%s: kska must be the 2-entry private key-switch set for N", who);
  if (kskb->row != 2 * N || kskb->b_word != N || kskb->n_in != N) return fail(MOSFHET_HIP_EINVAL, "%s: kskb must be a packing key N -> TRLWE(N)", who);
  if (N % (2 * l)) return fail(MOSFHET_HIP_EINVAL, "%s: N not divisible by 2l", who);
  if (ksk_out) {
    if (ksk_out->b_word != ksk_out->n_out) return fail(MOSFHET_HIP_EINVAL, "%s: ksk_out is a packing (LWE -> TRLWE) key, not an LWE -> LWE key", who);
    if (ksk_out->n_in != N || ksk_out->n_out != n)
      return fail(MOSFHET_HIP_EINVAL, "%s: ksk_out switches %d -> %d, the outputs need N = %d -> bsk's n = %d", who, ksk_out->n_in, ksk_out->n_out, N, n);
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
    if ((rc = circuit_bootstrap_3_run(who, ctx, bsk, kska, kskb, nullptr, sel, d_in + (size_t)first * size * ((size_t)n + 1), inputs * size, stream, nullptr))) return rc;
    uint64_t *dst = d_out + (size_t)first * outputs * out_row;
    if ((rc = leveled_lut_run(who, ctx, ksk_out ? lut_out : dst, reinterpret_cast<const double *>(sel), d_luts, size, N, l, Bg_bit, tables, pack_log, false, inputs, stream)))
      return rc;
    if (ksk_out && (rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, ksk_out, dst, lut_out, inputs * outputs, stream))) return rc;
  }
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_lut_bits_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out,
                                          uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int count, void *stream) {
  return lut_bits_run("lut_bits", ctx, bsk, kska, kskb, ksk_out, d_out, d_luts, d_in, size, tables, 0, count, stream);
}

extern "C" int mosfhet_hip_lut_bits_packed_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_bsk_t bsk, mosfhet_hip_gak_t kska, mosfhet_hip_ksk_t kskb, mosfhet_hip_ksk_t ksk_out,
                                                 uint64_t *d_out, const uint64_t *d_luts, const uint64_t *d_in, int size, int tables, int pack_log, int count, void *stream) {
  return lut_bits_run("lut_bits_packed", ctx, bsk, kska, kskb, ksk_out, d_out, d_luts, d_in, size, tables, pack_log, count, stream);
}
