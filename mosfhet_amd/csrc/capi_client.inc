// capi_client.inc -- the client half on the device: samples encrypted and opened under a secret-key handle (include/mosfhet_hip.h has the definition and the randomness
// contract).  Own code: nothing of the reference is compiled in.  Device code: client_kernels.h, as run-time kinds of two generator kernels (no kernel of its own).
//   mosfhet_hip_client_key_create / _destroy / _info   the secret keys as a handle: checked and packed on the host at creation (no device needed) -- the nonzero
//                                                      coefficients of the TRLWE key as (value << 16) | position, then the LWE key, one int per coefficient -- and copied
//                                                      to a device the first time a call runs there (table_image, capi_automaton.inc)
//   mosfhet_hip_tlwe_encrypt_batch, _trlwe_, _trgsw_   one ChaCha20 nonce per call (noise_key_for_call, kinds 6 - 8), launches in chunks of at most 2^20 rows; refused
//                                                      on a capturing stream before anything is launched.  TRGSW rows go to d_out_torus, or chunk by chunk through the
//                                                      calling thread's pool (slot POOL_CLIENT), and torus_to_dft_kernel transforms them as mosfhet_hip_bsk_generate does
//   mosfhet_hip_tlwe_phase_batch, _trlwe_              one launch, no pool, no nonce: capturable once the key image is on the device
//   mosfhet_hip_trgsw_encrypt_plan                     the shape of a TRGSW call as a pure function, shared with the launcher (client_trgsw_plan)

struct mosfhet_hip_client_key {
  int N = 0, n = 0, cnt_rlwe = 0, binary_rlwe = 1, cnt_lwe = 0, binary_lwe = 1;
  std::vector<int> table;                   // [cnt_rlwe] (value << 16) | position, then [n] LWE key coefficients
  std::mutex lock;
  std::map<int, int *> images;              // device -> the table's copy there, made on first use
  ~mosfhet_hip_client_key() {
    for (auto &e : images)
      if (hipSetDevice(e.first) == hipSuccess) (void)hipFree(e.second);
  }
};

enum { NOISE_CLIENT_TLWE = 6, NOISE_CLIENT_TRLWE = 7, NOISE_CLIENT_TRGSW = 8 };
static const size_t CLIENT_CHUNK_ROWS = (size_t)1 << 20;          // rows of one launch, as the generators' chunks
static const long long CLIENT_POOL_BYTES = 1ll << 30;             // bound of the pooled torus rows of a DFT-only TRGSW call

static bool client_fits16(uint64_t w) { const int64_t v = (int64_t)w; return v >= -32768 && v <= 32767; }

extern "C" int mosfhet_hip_client_key_create(mosfhet_hip_client_key_t *out, const uint64_t *h_s_rlwe, int N, const uint64_t *h_s_lwe, int n) {
  const char *who = "client_key_create";
  if (!out) return fail(MOSFHET_HIP_EINVAL, "%s: null out", who);
  if (!h_s_rlwe && !h_s_lwe) return fail(MOSFHET_HIP_EINVAL, "%s: null h_s_rlwe and null h_s_lwe (at least one key)", who);
  if (h_s_rlwe && (N < 256 || N > 4096 || (N & (N - 1)))) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d (a power of two in 256 .. 4096)", who, N);
  if (h_s_lwe && (n < 1 || n > 65536)) return fail(MOSFHET_HIP_EINVAL, "%s: n = %d (1 .. 65536: the ChaCha20 counter keeps 16 bits for the coefficient)", who, n);
  std::unique_ptr<mosfhet_hip_client_key> k(new mosfhet_hip_client_key());
  if (h_s_rlwe) {
    k->N = N;
    for (int x = 0; x < N; x++) {
      if (!client_fits16(h_s_rlwe[x])) return fail(MOSFHET_HIP_EINVAL, "%s: h_s_rlwe[%d] does not fit 16 bits", who, x);
      const int v = (int)(int64_t)h_s_rlwe[x];
      if (!v) continue;
      k->binary_rlwe &= v == 1;
      k->table.push_back((int)((unsigned)v << 16) | x);
    }
    k->cnt_rlwe = (int)k->table.size();
  }
  if (h_s_lwe) {
    k->n = n;
    for (int x = 0; x < n; x++) {
      if (!client_fits16(h_s_lwe[x])) return fail(MOSFHET_HIP_EINVAL, "%s: h_s_lwe[%d] does not fit 16 bits", who, x);
      const int v = (int)(int64_t)h_s_lwe[x];
      k->cnt_lwe += v != 0;
      k->binary_lwe &= v == 0 || v == 1;
      k->table.push_back(v);
    }
  }
  k->table.push_back(0);   // (never read: an image is never empty)
  *out = k.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_client_key_destroy(mosfhet_hip_client_key_t key) {
  delete key;
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_client_key_info(mosfhet_hip_client_key_t key, int64_t info[6]) {
  if (!key || !info) return fail(MOSFHET_HIP_EINVAL, "client_key_info: null %s", key ? "info" : "key");
  info[0] = key->N; info[1] = key->n; info[2] = key->cnt_rlwe; info[3] = key->binary_rlwe; info[4] = key->cnt_lwe; info[5] = key->binary_lwe;
  return MOSFHET_HIP_OK;
}

struct ClientTrgswPlan { long long launches, widest, bytes, chunks, chunk; };

// The one place that decides the shape of a TRGSW call: for the launcher and for mosfhet_hip_trgsw_encrypt_plan.  mode 0: DFT only (the torus rows pass through the pool,
// chunk by chunk under CLIENT_POOL_BYTES), 1: torus and DFT, 2: torus only.
static int client_trgsw_plan(const char *who, int N, int l, int count, int mode, ClientTrgswPlan *r) {
  if (N < 256 || N > 4096 || (N & (N - 1))) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d (a power of two in 256 .. 4096)", who, N);
  if (mode != 2 && !ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d has no TRGSW_DFT form (d_out_dft: 1024, 2048, 4096)", who, N);
  if (l < 1 || l > 6) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (mode < 0 || mode > 2) return fail(MOSFHET_HIP_EINVAL, "%s: with_torus_out = %d (0: DFT only, 1: torus and DFT, 2: torus only)", who, mode);
  const long long rows = (long long)count * 2 * l, row_bytes = 2ll * N * (long long)sizeof(uint64_t);
  long long chunk = (long long)CLIENT_CHUNK_ROWS;
  if (mode == 0 && CLIENT_POOL_BYTES / row_bytes < chunk) chunk = CLIENT_POOL_BYTES / row_bytes;
  if (rows < chunk) chunk = rows;
  r->chunk = chunk;
  r->chunks = rows ? (rows + chunk - 1) / chunk : 0;
  r->launches = r->chunks * (mode == 2 ? 1 : 2);
  r->widest = mode == 2 ? chunk : 2 * chunk;      // the transform runs one workgroup per polynomial, two per row
  r->bytes = mode == 0 ? chunk * row_bytes : 0;
  return MOSFHET_HIP_OK;
}

// info = { launches, workgroups of the widest launch, workspace bytes, chunks }
extern "C" int mosfhet_hip_trgsw_encrypt_plan(int N, int l, int count, int with_torus_out, int64_t info[4]) {
  if (!info) return fail(MOSFHET_HIP_EINVAL, "trgsw_encrypt_plan: null info");
  ClientTrgswPlan r;
  const int rc = client_trgsw_plan("trgsw_encrypt_plan", N, l, count, with_torus_out, &r);
  if (rc) return rc;
  info[0] = r.launches; info[1] = r.widest; info[2] = r.bytes; info[3] = r.chunks;
  return MOSFHET_HIP_OK;
}

// A replay of a captured encryption would reuse its nonce: the same masks and noise under a new message.
static int client_refuse_capture(const char *who, hipStream_t s) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(s, &status));
  if (status != hipStreamCaptureStatusNone)
    return fail(MOSFHET_HIP_EINVAL, "%s: the stream is in capture: an encryption cannot be captured (a replay would reuse its nonce: same masks and noise)", who);
  return MOSFHET_HIP_OK;
}

static int client_image(mosfhet_hip_client_key_t key, int device, const int **out) { return table_image(key->lock, key->images, key->table, device, out); }

// The client kinds of the two generator kernels that host them (keygen_kernels.h: ClientParams).  Ring kinds: one workgroup of 256 threads per row, the sign-extended
// mask in 16 N bytes of dynamic LDS -- 64 KiB at N = 4096, which a launch may use only with the attribute set (on the current device's copy of the kernel).
static int client_launch_ring(const ClientParams &p, unsigned grid, const NoiseKey &nkey, hipStream_t s) {
  const size_t lds = (size_t)16 * p.N;
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(trlwe_poly_keygen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds + 64));
  hipLaunchKernelGGL(trlwe_poly_keygen_kernel, dim3(grid), dim3(256), lds, s, (uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)nullptr, 0, 0, 0, 0.0,
                     (uint64_t)0, nkey, p);
  return MOSFHET_HIP_OK;
}

// LWE kinds: one wavefront per sample
static void client_launch_lwe(const ClientParams &p, unsigned grid, const NoiseKey &nkey, hipStream_t s) {
  hipLaunchKernelGGL(tlwe_ksk_keygen_kernel, dim3(grid), dim3(64), 0, s, (uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)nullptr, 0, 0, 0, 0.0, (uint64_t)0,
                     (size_t)0, 0, nkey, p);
}

// rows [first, first + n_rows) of one call under `nkey`, chunk by chunk; p.out / p.rows_first say where row numbers land
static int client_launch_rows(ClientParams p, size_t first, size_t n_rows, const NoiseKey &nkey, hipStream_t s) {
  for (size_t at = first; at < first + n_rows; at += CLIENT_CHUNK_ROWS) {
    const size_t chunk = first + n_rows - at < CLIENT_CHUNK_ROWS ? first + n_rows - at : CLIENT_CHUNK_ROWS;
    p.first_row = at;
    const int rc = client_launch_ring(p, (unsigned)chunk, nkey, s);
    if (rc) return rc;
  }
  return launched();
}

extern "C" int mosfhet_hip_tlwe_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out, const uint64_t *d_msg, double sigma, int count,
                                              void *stream) {
  const char *who = "tlwe_encrypt";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!key) return fail(MOSFHET_HIP_EINVAL, "%s: null key", who);
  if (!key->n) return fail(MOSFHET_HIP_EINVAL, "%s: the key handle has no LWE key (h_s_lwe)", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (!(sigma >= 0.0)) return fail(MOSFHET_HIP_EINVAL, "%s: sigma = %g", who, sigma);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out", who);
  if (!d_msg) return fail(MOSFHET_HIP_EINVAL, "%s: null d_msg", who);
  const int n = key->n;
  if (ranges_overlap(d_out, (size_t)count * ((size_t)n + 1) * sizeof(uint64_t), d_msg, (size_t)count * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_msg", who);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  int rc = client_refuse_capture(who, s);
  if (rc) return rc;
  const int *image = nullptr;
  if ((rc = client_image(key, ctx->device, &image))) return rc;
  const NoiseKey nkey = noise_key_for_call(NOISE_CLIENT_TLWE);
  ClientParams p = {};
  p.kind = 3; p.out = d_out; p.in = d_msg; p.key = image + key->cnt_rlwe; p.N = n; p.sigma = sigma;
  for (size_t at = 0; at < (size_t)count; at += CLIENT_CHUNK_ROWS) {
    const size_t chunk = (size_t)count - at < CLIENT_CHUNK_ROWS ? (size_t)count - at : CLIENT_CHUNK_ROWS;
    p.first_row = at;
    client_launch_lwe(p, (unsigned)chunk, nkey, s);
  }
  return launched();
}

extern "C" int mosfhet_hip_trlwe_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out, const uint64_t *d_msg, double sigma, int count,
                                               void *stream) {
  const char *who = "trlwe_encrypt";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!key) return fail(MOSFHET_HIP_EINVAL, "%s: null key", who);
  if (!key->N) return fail(MOSFHET_HIP_EINVAL, "%s: the key handle has no TRLWE key (h_s_rlwe)", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (!(sigma >= 0.0)) return fail(MOSFHET_HIP_EINVAL, "%s: sigma = %g", who, sigma);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out", who);
  const int N = key->N;
  if (d_msg && ranges_overlap(d_out, (size_t)count * 2 * N * sizeof(uint64_t), d_msg, (size_t)count * N * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_msg", who);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  int rc = client_refuse_capture(who, s);
  if (rc) return rc;
  const int *image = nullptr;
  if ((rc = client_image(key, ctx->device, &image))) return rc;
  ClientParams p = {};
  p.kind = 1; p.out = d_out; p.in = d_msg; p.key = image; p.cnt = key->cnt_rlwe; p.binary = key->binary_rlwe; p.N = N; p.sigma = sigma;
  return client_launch_rows(p, 0, (size_t)count, noise_key_for_call(NOISE_CLIENT_TRLWE), s);
}

extern "C" int mosfhet_hip_trgsw_encrypt_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, double *d_out_dft, uint64_t *d_out_torus, const int32_t *d_m,
                                               const int32_t *d_exp, int l, int Bg_bit, double sigma, int count, void *stream) {
  const char *who = "trgsw_encrypt";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!key) return fail(MOSFHET_HIP_EINVAL, "%s: null key", who);
  if (!key->N) return fail(MOSFHET_HIP_EINVAL, "%s: the key handle has no TRLWE key (h_s_rlwe)", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (l < 1 || Bg_bit < 1 || Bg_bit > 31 || l * Bg_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: bad gadget l=%d Bg_bit=%d (Bg_bit <= 31, l*Bg_bit < 64)", who, l, Bg_bit);
  if (!(sigma >= 0.0)) return fail(MOSFHET_HIP_EINVAL, "%s: sigma = %g", who, sigma);
  if (!d_out_dft && !d_out_torus) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out_dft and null d_out_torus (at least one output)", who);
  const int N = key->N;
  ClientTrgswPlan plan;
  int rc = client_trgsw_plan(who, N, l, count, d_out_dft ? (d_out_torus ? 1 : 0) : 2, &plan);
  if (rc || count == 0) return rc;
  if (!d_m) return fail(MOSFHET_HIP_EINVAL, "%s: null d_m", who);
  const size_t n_rows = (size_t)count * 2 * l, out_bytes = n_rows * 2 * N * sizeof(uint64_t), list_bytes = (size_t)count * sizeof(int32_t);
  if (d_out_dft && d_out_torus && ranges_overlap(d_out_dft, out_bytes, d_out_torus, out_bytes)) return fail(MOSFHET_HIP_EINVAL, "%s: d_out_dft overlaps d_out_torus", who);
  for (const void *o : {(const void *)d_out_dft, (const void *)d_out_torus}) {
    if (!o) continue;
    const char *name = o == (const void *)d_out_dft ? "d_out_dft" : "d_out_torus";
    if (ranges_overlap(o, out_bytes, d_m, list_bytes)) return fail(MOSFHET_HIP_EINVAL, "%s: %s overlaps d_m", who, name);
    if (d_exp && ranges_overlap(o, out_bytes, d_exp, list_bytes)) return fail(MOSFHET_HIP_EINVAL, "%s: %s overlaps d_exp", who, name);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  if ((rc = client_refuse_capture(who, s))) return rc;
  const int *image = nullptr;
  if ((rc = client_image(key, ctx->device, &image))) return rc;
  uint64_t *pool = nullptr;
  if (plan.bytes && (rc = pool_get(ctx->device, POOL_CLIENT, (size_t)(plan.bytes / (long long)sizeof(uint64_t)), &pool))) return rc;
  ClientParams p = {};
  p.kind = 1; p.m = d_m; p.exp = d_exp; p.key = image; p.cnt = key->cnt_rlwe; p.binary = key->binary_rlwe; p.N = N; p.l = l; p.Bg_bit = Bg_bit; p.sigma = sigma;
  const NoiseKey nkey = noise_key_for_call(NOISE_CLIENT_TRGSW);
  for (size_t at = 0; at < n_rows; at += (size_t)plan.chunk) {
    const size_t chunk = n_rows - at < (size_t)plan.chunk ? n_rows - at : (size_t)plan.chunk;
    if (d_out_torus) { p.out = d_out_torus; p.rows_first = 0; }
    else { p.out = pool; p.rows_first = at; }
    if ((rc = client_launch_rows(p, at, chunk, nkey, s))) return rc;
    if (d_out_dft) {
      const uint64_t *src = d_out_torus ? d_out_torus + at * 2 * N : pool;
      double *dst = d_out_dft + at * 2 * N;
      RING_DISPATCH(ctx, N, hipLaunchKernelGGL(torus_to_dft_kernel<F>, dim3((unsigned)(chunk * 2)), dim3(F::THREADS), 0, s, (const void *)src, (void *)dst, TW, 0));
    }
  }
  return launched();
}

// Argument checks of both phase calls, before any HIP call.
static int client_phase_check(const char *who, mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, int have, const char *which, const void *d_out, size_t out_words,
                              const void *d_in, size_t in_words, int msg_bits, int count) {
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!key) return fail(MOSFHET_HIP_EINVAL, "%s: null key", who);
  if (!have) return fail(MOSFHET_HIP_EINVAL, "%s: the key handle has no %s", who, which);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (msg_bits < 0 || msg_bits > 63) return fail(MOSFHET_HIP_EINVAL, "%s: msg_bits = %d (0: the phases, 1 .. 63: messages of that many bits)", who, msg_bits);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out) return fail(MOSFHET_HIP_EINVAL, "%s: null d_out", who);
  if (!d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null d_in", who);
  if (ranges_overlap(d_out, (size_t)count * out_words * sizeof(uint64_t), d_in, (size_t)count * in_words * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_tlwe_phase_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out, const uint64_t *d_in, int msg_bits, int count,
                                            void *stream) {
  const char *who = "tlwe_phase";
  int rc = client_phase_check(who, ctx, key, key ? key->n : 0, "LWE key (h_s_lwe)", d_out, 1, d_in, key ? (size_t)key->n + 1 : 1, msg_bits, count);
  if (rc || count == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int *image = nullptr;
  if ((rc = client_image(key, ctx->device, &image))) return rc;
  ClientParams p = {};
  p.kind = 4; p.out = d_out; p.in = d_in; p.key = image + key->cnt_rlwe; p.N = key->n; p.msg_bits = msg_bits;
  client_launch_lwe(p, (unsigned)count, NoiseKey{}, pick(ctx, stream));
  return launched();
}

extern "C" int mosfhet_hip_trlwe_phase_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_client_key_t key, uint64_t *d_out, const uint64_t *d_in, int msg_bits, int count,
                                             void *stream) {
  const char *who = "trlwe_phase";
  const int N = key ? key->N : 0;
  int rc = client_phase_check(who, ctx, key, N, "TRLWE key (h_s_rlwe)", d_out, (size_t)N, d_in, (size_t)2 * N, msg_bits, count);
  if (rc || count == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int *image = nullptr;
  if ((rc = client_image(key, ctx->device, &image))) return rc;
  ClientParams p = {};
  p.kind = 2; p.out = d_out; p.in = d_in; p.key = image; p.cnt = key->cnt_rlwe; p.binary = key->binary_rlwe; p.N = N; p.msg_bits = msg_bits;
  if ((rc = client_launch_ring(p, (unsigned)count, NoiseKey{}, pick(ctx, stream)))) return rc;
  return launched();
}
