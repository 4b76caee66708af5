// capi_unpack.inc -- packed TRLWE samples opened into batches of LWE samples on the device: the inverse layout of capi_pack.inc.  Own code: nothing of the reference is
// compiled in.  Kernels: unpack_kernels.h.
//
//   d_in [outputs][2][N], outputs = ceil(total / per); sample o per + j is the reference's trlwe_extract_tlwe(in[o], first + j stride) (src/trlwe.c:540-552, k = 1), word
//   for word; the calls without a geometry are (first 0, stride 1) of the same bodies
//
//   mosfhet_hip_trlwe_unpack_batch                                the [total][N + 1] batch
//   mosfhet_hip_trlwe_unpack_keyswitch_batch                      mosfhet_hip_tlwe_keyswitch_batch of that batch without writing it: the table key switch re-orients its input anyway
//                                                                 (ciphertexts along the fast index), and for extracted samples that orientation is the packed mask polynomial
//                                                                 read at an offset -- the pre-pass of every form reads the packed words directly (KsSource, keyswitch_kernels.h)
//   mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch       ... followed by the body of mosfhet_hip_keyswitch_functional_bootstrap_batch
//   mosfhet_hip_*_strided_*                                       the same three and the plan with (first, stride)
//
// One place decides the shape of a call (unpack_plan: for the launchers and for mosfhet_hip_trlwe_unpack_plan); the form of the switch is ks_form, the decision of
// launch_tlwe_keyswitch itself.  Up to 16 samples the switch walks no table and re-orients nothing: the samples are unpacked into the calling thread's pool (slot
// POOL_UNPACK) and take the existing path.  Everything is pure integer work, exact mod 2^64: no word depends on the form, on total, on the piece boundaries or on
// mosfhet_hip_set_ks_words.
constexpr int UNPACK_MAX_ROWS = 64, UNPACK_MIN_ROWS = 8;   // samples per workgroup of the row-major form: the staged polynomial is 1/64 .. 1/8 of the bytes written

struct UnpackPlan { int outputs, form, pieces, rows; long long prepass_wgs, prepass_bytes, saved_bytes, pool_bytes; };

static bool unpack_ring_ok(int N) { return N >= 256 && N <= 4096 && !(N & (N - 1)); }

// the geometry of a call on a ring N (per >= 1 already checked): 0 <= first < N, 1 <= stride, first + (per - 1) stride <= N - 1 in 64 bits -- indices do not wrap
static int unpack_geometry(const char *who, int N, int per, int first, int stride) {
  if (first < 0 || first >= N) return fail(MOSFHET_HIP_EINVAL, "%s: first = %d (0 .. N - 1 = %d)", who, first, N - 1);
  if (stride < 1) return fail(MOSFHET_HIP_EINVAL, "%s: stride = %d (at least 1)", who, stride);
  const long long last = (long long)first + ((long long)per - 1) * (long long)stride;
  if (last > N - 1)
    return fail(MOSFHET_HIP_EINVAL, "%s: stride = %d with per = %d and first = %d: the last coefficient first + (per - 1) stride = %lld is past N - 1 = %d (indices do not wrap)",
                who, stride, per, first, last, N - 1);
  return MOSFHET_HIP_OK;
}

// rows per workgroup of the row-major form: as many as leave at least four workgroups per CU, within UNPACK_MIN_ROWS .. UNPACK_MAX_ROWS
static int unpack_rows(int outputs, int per, int cus) {
  int rows = UNPACK_MAX_ROWS;
  while (rows > UNPACK_MIN_ROWS && (long long)outputs * ((per + rows - 1) / rows) < 4ll * cus) rows /= 2;
  return rows;
}

// n_out = 0: part 1 alone (t, base_bit and compressed are not read)
static int unpack_plan(const char *who, int N, int n_out, int t, int base_bit, int compressed, int total, int per, int first, int stride, int cus, UnpackPlan *r) {
  if (!unpack_ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (a power of two in 256 .. 4096)", who, N);
  if (n_out < 0) return fail(MOSFHET_HIP_EINVAL, "%s: n_out = %d", who, n_out);
  if (n_out > 0 && (t < 1 || t > 63)) return fail(MOSFHET_HIP_EINVAL, "%s: t = %d (1 .. 63)", who, t);
  if (n_out > 0 && (base_bit < 1 || base_bit > 8 || t * base_bit > 63)) return fail(MOSFHET_HIP_EINVAL, "%s: base_bit = %d (1 .. 8, t base_bit < 64)", who, base_bit);
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  if (per < 1 || per > N) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N = %d)", who, per, N);
  if (int rc = unpack_geometry(who, N, per, first, stride)) return rc;
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  // byte counts: refuse what does not fit a signed 64-bit field
  const unsigned __int128 limit = (unsigned __int128)0x7fffffffffffffffLL;
  const unsigned __int128 batch = (unsigned __int128)total * (unsigned __int128)(N + 1) * 8, switched = (unsigned __int128)total * ((unsigned __int128)n_out + 1) * 8;
  if (batch > limit || switched > limit)
    return fail(MOSFHET_HIP_EINVAL, "%s: total = %d samples x (N + 1 = %d or n_out + 1 = %lld) words x 8 bytes do not fit a 64-bit byte count", who, total, N + 1, (long long)n_out + 1);
  r->outputs = (int)(((long long)total + per - 1) / per);
  r->rows = unpack_rows(r->outputs, per, cus);
  const long long row_major_wgs = (long long)r->outputs * ((per + r->rows - 1) / r->rows);
  r->form = KS_FORM_SMALL; r->pieces = total ? 1 : 0;
  r->prepass_wgs = total ? row_major_wgs : 0; r->prepass_bytes = (long long)batch; r->saved_bytes = 0; r->pool_bytes = n_out ? (long long)batch : 0;
  if (!n_out || !total) return MOSFHET_HIP_OK;
  r->form = ks_form(total, N, n_out + 1, t, base_bit, compressed != 0, compressed ? n_out : 0);
  if (r->form == KS_FORM_SMALL) return MOSFHET_HIP_OK;
  r->saved_bytes = (long long)batch; r->pool_bytes = 0;
  if (r->form == KS_FORM_WORDS) {
    r->pieces = (int)(((long long)total + KSW_PIECE - 1) / KSW_PIECE);
    r->prepass_wgs = 0; r->prepass_bytes = 0;
    for (long long first = 0; first < total; first += KSW_PIECE) {
      const int n = (int)(total - first < KSW_PIECE ? total - first : KSW_PIECE);
      const KsWordsPlan p = ks_words_plan(n, N, n_out + 1, t, base_bit, cus, compressed != 0);
      r->prepass_wgs += (long long)p.ctwaves * ((N + 63) / 64);
      r->prepass_bytes += (long long)p.entry_bytes + (long long)n * 8;   // the digit entries and the b words
    }
    return MOSFHET_HIP_OK;
  }
  r->prepass_wgs = (((long long)total + UNPACK_THREADS - 1) / UNPACK_THREADS) * ((N + 1 + UNPACK_COL_WORDS - 1) / UNPACK_COL_WORDS);   // inT [N + 1][Bp], the words of live columns
  return MOSFHET_HIP_OK;
}

// plan = { outputs, form of the switch (0 small via unpack, 1 word-lane, 2 tiles of 256, 3 tiles of 512), pieces, workgroups of the source pre-pass, bytes the pre-pass
//          writes, bytes of the [total][N + 1] batch the fused form does not write, pool bytes used, rows per workgroup of the row-major form }
// No field depends on the geometry: it is checked and nothing else.
static int unpack_plan_out(const char *who, int N, int n_out, int t, int base_bit, int compressed, int total, int per, int first, int stride, int cus, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "%s: null plan", who);
  UnpackPlan r;
  const int rc = unpack_plan(who, N, n_out, t, base_bit, compressed, total, per, first, stride, cus, &r);
  if (rc) return rc;
  plan[0] = r.outputs; plan[1] = r.form; plan[2] = r.pieces; plan[3] = r.prepass_wgs; plan[4] = r.prepass_bytes; plan[5] = r.saved_bytes; plan[6] = r.pool_bytes; plan[7] = r.rows;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_trlwe_unpack_plan(int N, int n_out, int t, int base_bit, int compressed, int total, int per, int cus, long long plan[8]) {
  return unpack_plan_out("trlwe_unpack_plan", N, n_out, t, base_bit, compressed, total, per, 0, 1, cus, plan);
}

extern "C" int mosfhet_hip_trlwe_unpack_strided_plan(int N, int n_out, int t, int base_bit, int compressed, int total, int per, int first, int stride, int cus,
                                                     long long plan[8]) {
  return unpack_plan_out("trlwe_unpack_strided_plan", N, n_out, t, base_bit, compressed, total, per, first, stride, cus, plan);
}

// the row-major form: one workgroup per (input, block of `rows` samples)
static int launch_trlwe_unpack(uint64_t *out, const uint64_t *in, int N, int total, int per, int first, int stride, int rows, hipStream_t s) {
  const int outputs = (int)(((long long)total + per - 1) / per);
  hipLaunchKernelGGL(trlwe_unpack_kernel, dim3((unsigned)((long long)outputs * ((per + rows - 1) / rows))), dim3(UNPACK_THREADS), (size_t)N * sizeof(uint64_t), s, out, in, N, per, 0,
                     first, stride, total, (size_t)N + 1, (size_t)1, rows);
  return launched();
}

// Null handles and scalar ranges come before any handle is read and before any HIP call.
static int trlwe_unpack_body(const char *who, mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in, int N, int total, int per, int first, int stride, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  UnpackPlan plan;
  int rc = unpack_plan(who, N, 0, 0, 0, 0, total, per, first, stride, 256, &plan);   // the ring, total, per <= N, the geometry, the size limit
  if (rc) return rc;
  if (total == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (ranges_overlap(d_out, (size_t)total * ((size_t)N + 1) * sizeof(uint64_t), d_in, (size_t)plan.outputs * 2 * N * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_trlwe_unpack(d_out, d_in, N, total, per, first, stride, unpack_rows(plan.outputs, per, ksw_device_cus()), pick(ctx, stream));
}

extern "C" int mosfhet_hip_trlwe_unpack_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in, int N, int total, int per, void *stream) {
  return trlwe_unpack_body("trlwe_unpack", ctx, d_out, d_in, N, total, per, 0, 1, stream);
}

extern "C" int mosfhet_hip_trlwe_unpack_strided_batch(mosfhet_hip_ctx_t ctx, uint64_t *d_out, const uint64_t *d_in, int N, int total, int per, int first, int stride,
                                                      void *stream) {
  return trlwe_unpack_body("trlwe_unpack_strided", ctx, d_out, d_in, N, total, per, first, stride, stream);
}

// the scalar checks of parts 2 and 3 that need no handle: the ring comes from the key, so the ranges are held to the largest ring here and to the key's in unpack_plan
static int unpack_scalars(const char *who, int total, int per, int first, int stride) {
  if (per < 1 || per > 4096) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N)", who, per);
  if (int rc = unpack_geometry(who, 4096, per, first, stride)) return rc;
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  return MOSFHET_HIP_OK;
}

// the checks of parts 2 and 3 on the key and the buffers (total > 0)
static int unpack_keyswitch_check(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, const uint64_t *d_out, const uint64_t *d_in, size_t out_row, int total, int per,
                                  int first, int stride, UnpackPlan *plan) {
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (ksk->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: ksk belongs to another context (device %d)", who, ksk->device);
  if (ksk->b_word != ksk->n_out) return fail(MOSFHET_HIP_EINVAL, "%s: this key is a packing (LWE -> TRLWE) key: an LWE -> LWE key from the extracted key is needed", who);
  if (!unpack_ring_ok(ksk->n_in)) return fail(MOSFHET_HIP_EINVAL, "%s: the key switches from n_in = %d words: not the extracted key of a ring this call opens (N a power of two in 256 .. 4096)", who, ksk->n_in);
  HIP_TRY(hipSetDevice(ctx->device));
  const int rc = unpack_plan(who, ksk->n_in, ksk->n_out, ksk->t, ksk->base_bit, ksk->compressed, total, per, first, stride, ksw_device_cus(), plan);   // per <= N = n_in, the geometry, the size limits
  if (rc) return rc;
  if (ranges_overlap(d_out, (size_t)total * out_row * sizeof(uint64_t), d_in, (size_t)plan->outputs * 2 * ksk->n_in * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  return MOSFHET_HIP_OK;
}

// switched [total][n_out + 1] <- the key switch of the samples of d_in
static int unpack_keyswitch_run(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, const UnpackPlan &plan, uint64_t *switched, const uint64_t *d_in, int total, int per, int first,
                                int stride, hipStream_t s) {
  const int N = ksk->n_in;
  if (plan.form == KS_FORM_SMALL) {
    uint64_t *rows = nullptr;
    const int rc = pool_get(ctx->device, POOL_UNPACK, (size_t)total * ((size_t)N + 1), &rows);
    if (rc) return rc;
    if (int r2 = launch_trlwe_unpack(rows, d_in, N, total, per, first, stride, plan.rows, s)) return r2;
    HIP_TRY(launch_tlwe_keyswitch(ksk->d_ksk, switched, (size_t)ksk->row, rows, (size_t)N + 1, total, N, ksk->row, ksk->b_word, ksk->t, ksk->base_bit, tl_ws(ctx->device), s,
                                  ksk->compressed, ksk->seed));
    return MOSFHET_HIP_OK;
  }
  HIP_TRY(launch_tlwe_keyswitch(ksk->d_ksk, switched, (size_t)ksk->row, KsSource::trlwe(d_in, N, per, 0, first, stride), total, N, ksk->row, ksk->b_word, ksk->t, ksk->base_bit,
                                tl_ws(ctx->device), s, ksk->compressed, ksk->seed));
  return MOSFHET_HIP_OK;
}

static int trlwe_unpack_keyswitch_body(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out, const uint64_t *d_in, int total, int per, int first,
                                       int stride, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!ksk) return fail(MOSFHET_HIP_EINVAL, "%s: null ksk", who);
  int rc = unpack_scalars(who, total, per, first, stride);
  if (rc) return rc;
  if (total == 0) return MOSFHET_HIP_OK;
  UnpackPlan plan;
  rc = unpack_keyswitch_check(who, ctx, ksk, d_out, d_in, (size_t)ksk->n_out + 1, total, per, first, stride, &plan);
  if (rc) return rc;
  return unpack_keyswitch_run(ctx, ksk, plan, d_out, d_in, total, per, first, stride, pick(ctx, stream));
}

extern "C" int mosfhet_hip_trlwe_unpack_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out, const uint64_t *d_in, int total, int per, void *stream) {
  return trlwe_unpack_keyswitch_body("trlwe_unpack_keyswitch", ctx, ksk, d_out, d_in, total, per, 0, 1, stream);
}

extern "C" int mosfhet_hip_trlwe_unpack_strided_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, uint64_t *d_out, const uint64_t *d_in, int total, int per,
                                                                int first, int stride, void *stream) {
  return trlwe_unpack_keyswitch_body("trlwe_unpack_strided_keyswitch", ctx, ksk, d_out, d_in, total, per, first, stride, stream);
}

// part 2 into the bootstrap key's scratch, then the body of mosfhet_hip_keyswitch_functional_bootstrap_batch: the same scratch, the same one-stream-per-host-thread rule
static int unpack_keyswitch_bootstrap_body(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tv,
                                           int tv_count, const uint64_t *d_in, int total, int per, int first, int stride, int torus_base, int extract, void *stream) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!ksk || !bsk) return fail(MOSFHET_HIP_EINVAL, "%s: null key", who);
  if (int rs = unpack_scalars(who, total, per, first, stride)) return rs;
  if (int rk = ks_bootstrap_keys_match(who, ksk, bsk)) return rk;
  if (bsk->k != 1) return fail(MOSFHET_HIP_EINVAL, "%s: packed inputs have one mask polynomial (k = 1), the bootstrap key has k = %d", who, bsk->k);
  if (total == 0) return MOSFHET_HIP_OK;
  UnpackPlan plan;
  int rc = unpack_keyswitch_check(who, ctx, ksk, d_out, d_in, extract ? (size_t)bsk->N + 1 : (size_t)2 * bsk->N, total, per, first, stride, &plan);
  if (rc) return rc;
  uint64_t *tmp = nullptr;
  if ((rc = ext_scratch(bsk, 1, (size_t)total * (bsk->n + 1), &tmp))) return rc;
  if ((rc = unpack_keyswitch_run(ctx, ksk, plan, tmp, d_in, total, per, first, stride, pick(ctx, stream)))) return rc;
  return extract ? mosfhet_hip_functional_bootstrap_batch(ctx, bsk, d_out, d_tv, tv_count, tmp, total, torus_base, stream)
                 : mosfhet_hip_functional_bootstrap_wo_extract_batch(ctx, bsk, d_out, d_tv, tv_count, tmp, total, torus_base, stream);
}

extern "C" int mosfhet_hip_unpack_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out, const uint64_t *d_tv,
                                                                       int tv_count, const uint64_t *d_in, int total, int per, int torus_base, int extract, void *stream) {
  return unpack_keyswitch_bootstrap_body("unpack_keyswitch_bootstrap", ctx, ksk, bsk, d_out, d_tv, tv_count, d_in, total, per, 0, 1, torus_base, extract, stream);
}

extern "C" int mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_ksk_t ksk, mosfhet_hip_bsk_t bsk, uint64_t *d_out,
                                                                               const uint64_t *d_tv, int tv_count, const uint64_t *d_in, int total, int per, int first,
                                                                               int stride, int torus_base, int extract, void *stream) {
  return unpack_keyswitch_bootstrap_body("unpack_strided_keyswitch_bootstrap", ctx, ksk, bsk, d_out, d_tv, tv_count, d_in, total, per, first, stride, torus_base, extract, stream);
}
