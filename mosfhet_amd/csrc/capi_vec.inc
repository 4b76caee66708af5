// capi_vec.inc -- digit-parallel forms of the radix-integer callers of the reference's applications/multi-ciphertext-arith (SURVEY 8(f).4): the same gate
// sequences as ufhe_extend_integer / ufhe_sl_add_integer / ufhe_sl_addto_integer / ufhe_sub_integer / ufhe_mul_integer (src/integer.c:62-215), ufhe_cmp_integer
// (:217-264), ufhe_relu_integer (src/ml.c:4-20), ufhe_encrypted_tlwe_lut (src/lut.c:6-20) and ufhe_lut_integer (:23-47), written over the *_batch entry points of
// this library for M INDEPENDENT integers at once: every step of a carry chain, every level of a LUT tree, every table of a multiplication step
// is ONE key switch + ONE packing switch + ONE bootstrap launch over all M (x groups) samples instead of M (x groups) single gates.  Own code: the
// reference application is the specification (which LUT, which extraction, which constant), nothing of it is compiled in.
//
// Layout: an array of M integers of d digits is DIGIT-MAJOR on the device, [d][M][N+1] torus words (digit plane i = the i-th radix-B digit of every integer, B =
// torus_base, encoded as digit / (2 B) under the extracted TRLWE key like ufhe_encrypt_integer, src/integer.c:34-40), so that a step's M samples are one
// contiguous batch.  Temporaries live in the calling thread's pool (slots POOL_VEC, POOL_VEC2; POOL_VEC3 for the cleartext LUT, POOL_VEC4 for the multiplication): no
// call allocates per call or synchronises, all of them queue on the given stream.  Limits (EINVAL beyond them): M <= 65535 (the extraction kernels index the batch by
// gridDim.z), units per launch <= INT_MAX.  The handle is read-only after creation.
struct mosfhet_hip_vec {
  mosfhet_hip_ctx_t ctx = nullptr;
  mosfhet_hip_bsk_t bsk = nullptr;     // borrowed: bootstrap key n -> N
  mosfhet_hip_ksk_t ksk = nullptr;     // borrowed: LWE key switch N -> n
  mosfhet_hip_ksk_t pksk = nullptr;    // borrowed: LUT-packing key (torus_base slots), may be null (then only add / sub)
  int torus_base = 0, log_torus_base = 0;
  uint64_t *d_luts = nullptr;          // [3][2][N]: ADDSUB_LUT (constant -1/(4B), src/ufhe.c:61-64), ReLU's top-digit LUT (src/ml.c:14-18), SIGNEXTEND_LUT (src/ufhe.c:66-71)
  ~mosfhet_hip_vec() {
    if (ctx) (void)hipSetDevice(ctx->device);
    if (d_luts) (void)hipFree(d_luts);
  }
};
typedef mosfhet_hip_vec *mosfhet_hip_vec_t;

// trivial samples (a = 0, b = value) for a batch [src/tlwe.c: tlwe_noiseless_trivial_sample]
__global__ void tlwe_trivial_kernel(uint64_t *__restrict__ out, size_t words, int row, uint64_t value) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) out[i] = (i % (size_t)row == (size_t)row - 1) ? value : 0;
}
// packing-switch inputs of ReLU (src/ml.c:6-10): unit (i, m), slot q = digit i of integer m for q < B/2, a trivial zero above; dst [units][B][row]
__global__ void relu_slots_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ in, size_t units, int B, int row) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = units * (size_t)B * row;
  if (i >= total) return;
  const size_t w = i % row, q = (i / row) % B, u = i / ((size_t)row * B);
  dst[i] = q < (size_t)B / 2 ? in[u * row + w] : 0;
}
// packing-switch inputs of one level of the encrypted-LUT tree (src/lut.c:12-15): unit (j, m), slot q = table entry j B + q of instance m; table [size][M][row]
__global__ void lut_level_slots_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ table, size_t groups, size_t M, int B, int row) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = groups * M * (size_t)B * row;
  if (i >= total) return;
  const size_t w = i % row, q = (i / row) % B, u = i / ((size_t)row * B), j = u / M, m = u % M;
  dst[i] = table[((j * B + q) * M + m) * row + w];
}

// packing-switch inputs of the comparison (src/integer.c:216-245): per integer m the B slots of its LUT.  mode 0: slot 0 = the running result c0[m], the others the
// trivial sample `one`; mode 1 (sign steps): slots below B / 2 = c0[m], the others -c0[m].  dst [M][B][row]
// ... and of the product tables (src/integer.c:183-196), modes 2 and 3: the B slots [0, c0[m] (mode 2) or 0 (mode 3), v_2[m], .., v_{B-1}[m]]; vals [B-2][M][row]
__global__ void cmp_slots_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ c0, const uint64_t *__restrict__ vals, size_t M, int B, int row, int mode, uint64_t one) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = M * (size_t)B * row;
  if (i >= total) return;
  const size_t w = i % row, q = (i / row) % B, m = i / ((size_t)row * B);
  if (mode >= 2) {
    dst[i] = q == 0 ? 0 : (q == 1 ? (mode == 2 ? c0[m * row + w] : 0) : vals[((q - 2) * M + m) * row + w]);
    return;
  }
  const uint64_t c = c0[m * row + w];
  if (mode == 0) dst[i] = q == 0 ? c : (w == (size_t)row - 1 ? one : 0);
  else dst[i] = q < (size_t)B / 2 ? c : (uint64_t)0 - c;
}

static uint64_t vec_double2torus(double d) { return (uint64_t)((int64_t)((d - (double)(int64_t)d) * 18446744073709551616.0)); }   // src/misc.c:13-15

extern "C" int mosfhet_hip_vec_create(mosfhet_hip_ctx_t ctx, mosfhet_hip_vec_t *out, mosfhet_hip_bsk_t bsk, mosfhet_hip_ksk_t ksk, mosfhet_hip_ksk_t pksk, int torus_base) {
  if (!ctx || !out || !bsk || !ksk) return fail(MOSFHET_HIP_EINVAL, "vec_create: bad argument");
  TUNED_ONLY(bsk, "vec_create");
  if (torus_base < 2 || (torus_base & (torus_base - 1)) || bsk->N % (2 * torus_base)) return fail(MOSFHET_HIP_EINVAL, "vec_create: torus_base %d must be a power of two dividing N / 2", torus_base);
  if (ksk->n_in != bsk->N || ksk->n_out != bsk->n || ksk->b_word != ksk->n_out) return fail(MOSFHET_HIP_EINVAL, "vec_create: ksk must be the LWE key switch N -> n of the bootstrap key");
  if (pksk && (pksk->b_word >= 0 || pksk->row != 2 * bsk->N || pksk->n_in != bsk->N * torus_base))
    return fail(MOSFHET_HIP_EINVAL, "vec_create: pksk must be the LUT-packing key of %d slots from the extracted key (N words) to TRLWE(N)", torus_base);
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mosfhet_hip_vec> v(new mosfhet_hip_vec());
  v->ctx = ctx; v->bsk = bsk; v->ksk = ksk; v->pksk = pksk; v->torus_base = torus_base; v->log_torus_base = ilog2(torus_base);
  const int N = bsk->N;
  HIP_TRY(hipMalloc((void **)&v->d_luts, (size_t)3 * 2 * N * sizeof(uint64_t)));
  // ADDSUB_LUT: every slot -1/(4B) (src/ufhe.c:61-64)
  hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, nullptr, v->d_luts, N, (const uint64_t *)nullptr, 1, vec_double2torus(-1. / (4 * torus_base)), vec_double2torus(-1. / (4 * torus_base)));
  // ReLU's LUT for the top digit (src/ml.c:14-18): slot j < B/2 keeps j, the negative half gives 0
  std::vector<uint64_t> slots(torus_base, 0);
  for (int j = 0; j < torus_base / 2; j++) slots[j] = vec_double2torus((double)j / (torus_base * 2));
  DevBuf d_slots;
  HIP_TRY(d_slots.alloc(slots.size() * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(d_slots.p, slots.data(), slots.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, nullptr, v->d_luts + (size_t)2 * N, N, d_slots.as<uint64_t>(), torus_base, (uint64_t)0, (uint64_t)0);
  HIP_TRY(hipStreamSynchronize(nullptr));
  // SIGNEXTEND_LUT (src/ufhe.c:66-71): 0 for the non-negative half, (B - 1) / (2 B) for the negative one
  for (int j = 0; j < torus_base; j++) slots[j] = j < torus_base / 2 ? 0 : vec_double2torus((double)(torus_base - 1) / (2 * torus_base));
  HIP_TRY(hipMemcpy(d_slots.p, slots.data(), slots.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(torus_packing_kernel, dim3((N + 255) / 256), dim3(256), 0, nullptr, v->d_luts + (size_t)4 * N, N, d_slots.as<uint64_t>(), torus_base, (uint64_t)0, (uint64_t)0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = v.release();
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_vec_destroy(mosfhet_hip_vec_t vec) {
  delete vec;
  return MOSFHET_HIP_OK;
}

// c = a + b (subtract = 0: ufhe_sl_add_integer with g = h = 0, src/integer.c:79-107) or c = a - b (subtract = 1: ufhe_sub_integer, :136-156) for M integers of d
// digits each (signed integers of equal width, or unsigned ones whose result keeps the operands' width: the chain runs over all d digits and the carry out of the
// last one is dropped, as the reference's loops do at c->d == a->d == b->d).  c must not alias a or b.  Per digit: one launch of each gate for all M integers.
extern "C" int mosfhet_hip_vec_addsub(mosfhet_hip_vec_t vec, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, int M, int d, int subtract, void *stream) {
  if (!vec || M < 0 || d < 1) return fail(MOSFHET_HIP_EINVAL, "vec_addsub: bad argument");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_c || !d_a || !d_b || d_c == d_a || d_c == d_b) return fail(MOSFHET_HIP_EINVAL, "vec_addsub: null or aliased buffer");
  if (M > 65535) return fail(MOSFHET_HIP_EINVAL, "vec_addsub: M = %d (at most 65535 integers per call)", M);
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, B = vec->torus_base, row = N + 1;
  const size_t plane = (size_t)M * row;
  uint64_t *rot = nullptr;                                     // [M][2][N]: the rotated ADDSUB_LUT of the step
  int rc = pool_get(ctx->device, POOL_VEC, (size_t)M * 2 * N, &rot);
  if (rc) return rc;
  const unsigned g_plane = (unsigned)((plane + 255) / 256), g_m = (unsigned)((M + 255) / 256);
  // sign conventions of the two loops: add subtracts the B-scaled extraction and 1/4, carries +1/(4B) + extraction; sub mirrors every sign (src/integer.c:97-104, 146-152)
  const uint64_t quarter = vec_double2torus(subtract ? 0.25 : -0.25), carry0 = vec_double2torus((subtract ? -1. : 1.) / (4 * B));
  hipLaunchKernelGGL(tlwe_trivial_kernel, dim3(g_plane), dim3(256), 0, s, d_c, plane, row, (uint64_t)0);
  for (int i = 0; i < d; i++) {
    uint64_t *c_i = d_c + (size_t)i * plane;
    hipLaunchKernelGGL(words_add2_kernel, dim3(g_plane), dim3(256), 0, s, c_i, d_a + (size_t)i * plane, d_b + (size_t)i * plane, plane, subtract, 1);
    if ((rc = mosfhet_hip_keyswitch_functional_bootstrap_batch(ctx, vec->ksk, vec->bsk, rot, vec->d_luts, 1, c_i, M, B, 0, stream))) return rc;
    if ((rc = mosfhet_hip_trlwe_mv_extract_batch(ctx, c_i, rot, N, subtract ? 2 : 3, B, M, stream))) return rc;
    hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3(g_m), dim3(256), 0, s, c_i, M, (size_t)row, ((size_t)row) - 1, quarter);
    if (i != d - 1) {
      uint64_t *c_n = c_i + plane;
      hipLaunchKernelGGL(tlwe_trivial_kernel, dim3(g_plane), dim3(256), 0, s, c_n, plane, row, carry0);
      if ((rc = mosfhet_hip_trlwe_mv_extract_batch(ctx, c_n, rot, N, subtract ? 3 : 2, 1, M, stream))) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// out = in > 0 ? in : 0 for M signed integers of d digits (ufhe_relu_integer, src/ml.c:4-20): the top digit of every integer is key-switched once; the d - 1 lower
// digits of all M integers go through ONE packing switch (slots: the digit in the non-negative half, zero in the negative half) and ONE bootstrap launch, the top
// digit through one more.  out may alias in (the reference calls it in place, test/tests.c:186).
extern "C" int mosfhet_hip_vec_relu(mosfhet_hip_vec_t vec, uint64_t *d_out, const uint64_t *d_in, int M, int d, void *stream) {
  if (!vec || M < 0 || d < 1) return fail(MOSFHET_HIP_EINVAL, "vec_relu: bad argument");
  if (!vec->pksk) return fail(MOSFHET_HIP_EINVAL, "vec_relu: the handle has no LUT-packing key");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "vec_relu: null buffer");
  if (M > 65535 || (long long)(d - 1) * M > 0x7fffffffLL / (vec->torus_base > 0 ? vec->torus_base : 1)) return fail(MOSFHET_HIP_EINVAL, "vec_relu: batch too large (M <= 65535)");
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, n = vec->bsk->n, B = vec->torus_base, row = N + 1;
  const size_t plane = (size_t)M * row, units = (size_t)(d - 1) * M;
  // pool: selectors tiled d - 1 times + one more copy [d][M][n+1], packing inputs [units][B][row], packed test vectors [units][2][N]
  const size_t w_sel = (size_t)d * M * (n + 1), w_slots = units * B * row, w_tv = units * 2 * N;
  uint64_t *sel = nullptr;
  int rc = pool_get(ctx->device, POOL_VEC, w_sel + w_slots + w_tv, &sel);
  if (rc) return rc;
  uint64_t *slots = sel + w_sel, *tvs = slots + w_slots;
  if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel, d_in + (size_t)(d - 1) * plane, M, stream))) return rc;
  for (int i = 1; i < d - 1; i++) HIP_TRY(hipMemcpyAsync(sel + (size_t)i * M * (n + 1), sel, (size_t)M * (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  if (units) {
    hipLaunchKernelGGL(relu_slots_kernel, dim3((unsigned)((w_slots + 255) / 256)), dim3(256), 0, s, slots, d_in, units, B, row);
    if ((rc = mosfhet_hip_trlwe_lut_packing_keyswitch_batch(ctx, vec->pksk, B, tvs, slots, (int)units, stream))) return rc;
  }
  // the top digit first (it reads in[d-1] through sel only, and out may alias in), then the lower digits
  if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, vec->bsk, d_out + (size_t)(d - 1) * plane, vec->d_luts + (size_t)2 * N, 1, sel, M, B, stream))) return rc;
  if (units && (rc = mosfhet_hip_functional_bootstrap_batch(ctx, vec->bsk, d_out, tvs, (int)units, sel, (int)units, B, stream))) return rc;
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// table[0][m] = table[selector_m][m] for M independent encrypted tables of `size` entries each (ufhe_encrypted_tlwe_lut, src/lut.c:6-20): d_table [size][M][N+1] is
// consumed level by level (size -> size / B -> ... -> 1; entry 0 of every instance holds the result), d_sel [levels][M][N+1] holds the selector digits, least
// significant first, levels = log_B(size).  Per level: one key switch of the level's M selector digits, ONE packing switch over all size / B groups of all M
// instances, ONE bootstrap launch over the same units.
extern "C" int mosfhet_hip_vec_encrypted_lut(mosfhet_hip_vec_t vec, uint64_t *d_table, const uint64_t *d_sel, int size, int M, void *stream) {
  if (!vec || M < 0 || size < 1) return fail(MOSFHET_HIP_EINVAL, "vec_encrypted_lut: bad argument");
  if (!vec->pksk) return fail(MOSFHET_HIP_EINVAL, "vec_encrypted_lut: the handle has no LUT-packing key");
  const int B = vec->torus_base;
  int levels = 0;
  for (int sz = size; sz > 1; sz /= B, levels++)
    if (sz % B) return fail(MOSFHET_HIP_EINVAL, "vec_encrypted_lut: size %d is not a power of torus_base %d", size, B);
  if (M == 0 || levels == 0) return MOSFHET_HIP_OK;
  if (!d_table || !d_sel) return fail(MOSFHET_HIP_EINVAL, "vec_encrypted_lut: null buffer");
  if ((long long)(size / B) * M > 0x7fffffffLL / B) return fail(MOSFHET_HIP_EINVAL, "vec_encrypted_lut: too many units (size / torus_base x M)");
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, n = vec->bsk->n, row = N + 1;
  const size_t plane = (size_t)M * row, g0 = (size_t)size / B;
  const size_t w_sel = g0 * M * (n + 1), w_slots = g0 * M * B * row, w_tv = g0 * M * 2 * N;
  uint64_t *sel = nullptr;
  int rc = pool_get(ctx->device, POOL_VEC, w_sel + w_slots + w_tv, &sel);
  if (rc) return rc;
  uint64_t *slots = sel + w_sel, *tvs = slots + w_slots;
  int sz = size;
  for (int lev = 0; lev < levels; lev++, sz /= B) {
    const size_t groups = (size_t)sz / B, units = groups * M;
    if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel, d_sel + (size_t)lev * plane, M, stream))) return rc;
    for (size_t j = 1; j < groups; j++) HIP_TRY(hipMemcpyAsync(sel + j * M * (n + 1), sel, (size_t)M * (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(lut_level_slots_kernel, dim3((unsigned)((units * B * row + 255) / 256)), dim3(256), 0, s, slots, d_table, groups, (size_t)M, B, row);
    if ((rc = mosfhet_hip_trlwe_lut_packing_keyswitch_batch(ctx, vec->pksk, B, tvs, slots, (int)units, stream))) return rc;
    if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, vec->bsk, d_table, tvs, (int)units, sel, (int)units, B, stream))) return rc;   // entry j of instance m <- unit (j, m)
  }
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// out[m] = vec[selector_m][m] for M independent arrays of `size` encrypted integers of d digits each (ufhe_mux_integer_array, src/lut.c:49-64: one tree per output
// digit, all under the same selector).  d_tables [size][d][M][N+1] IS [size][d M][N+1]: the d trees of all M instances run as ONE tree over d M instances whose
// selector digits are the M selectors repeated d times, so every level is one packing switch and one bootstrap launch over size / B^level x d x M units.  d_tables is
// consumed; d_out [d][M][N+1] receives entry 0.
extern "C" int mosfhet_hip_vec_mux_array(mosfhet_hip_vec_t vec, uint64_t *d_out, uint64_t *d_tables, const uint64_t *d_sel, int size, int d, int M, void *stream) {
  if (!vec || M < 0 || size < 1 || d < 1) return fail(MOSFHET_HIP_EINVAL, "vec_mux_array: bad argument");
  const int B = vec->torus_base;
  int levels = 0;
  for (int sz = size; sz > 1; sz /= B, levels++)
    if (sz % B) return fail(MOSFHET_HIP_EINVAL, "vec_mux_array: size %d is not a power of torus_base %d", size, B);
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_tables || (levels && !d_sel)) return fail(MOSFHET_HIP_EINVAL, "vec_mux_array: null buffer");
  if ((long long)d * M > 0x7fffffffLL / size) return fail(MOSFHET_HIP_EINVAL, "vec_mux_array: too many units");
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const size_t plane = (size_t)M * (vec->bsk->N + 1);
  if (levels) {
    uint64_t *sel = nullptr;   // [levels][d][M][N+1]
    int rc = pool_get(ctx->device, POOL_VEC2, (size_t)levels * d * plane, &sel);
    if (rc) return rc;
    for (int lev = 0; lev < levels; lev++)
      for (int i = 0; i < d; i++)
        HIP_TRY(hipMemcpyAsync(sel + ((size_t)lev * d + i) * plane, d_sel + (size_t)lev * plane, plane * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if ((rc = mosfhet_hip_vec_encrypted_lut(vec, d_tables, sel, size, d * M, stream))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(d_out, d_tables, (size_t)d * plane * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  return MOSFHET_HIP_OK;
}

// c[m] = 0 if a[m] < b[m], 1 if equal, 2 if a[m] > b[m] (as digit / (2 B), ufhe_cmp_integer, src/integer.c:205-264) for M pairs of integers of d digits: the digits
// are compared from the least significant one up, every step ONE key switch of the M differences, ONE packing switch of the M running LUTs [c, 1, .., 1] and ONE
// bootstrap launch; signed operands take one more step each on their top digit.  d_c: [M][N+1] (the one digit that carries the result).
extern "C" int mosfhet_hip_vec_cmp(mosfhet_hip_vec_t vec, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, int M, int d, int a_signed, int b_signed, void *stream) {
  if (!vec || M < 0 || d < 1) return fail(MOSFHET_HIP_EINVAL, "vec_cmp: bad argument");
  if (!vec->pksk) return fail(MOSFHET_HIP_EINVAL, "vec_cmp: the handle has no LUT-packing key");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_c || !d_a || !d_b) return fail(MOSFHET_HIP_EINVAL, "vec_cmp: null buffer");
  if (d_c == d_a || d_c == d_b) return fail(MOSFHET_HIP_EINVAL, "vec_cmp: the result must not alias an operand");
  if (M > 65535) return fail(MOSFHET_HIP_EINVAL, "vec_cmp: M = %d (at most 65535 integers per call)", M);
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, n = vec->bsk->n, B = vec->torus_base, row = N + 1;
  const size_t plane = (size_t)M * row, w_sel = (size_t)M * (n + 1), w_slots = (size_t)M * B * row, w_tv = (size_t)M * 2 * N;
  uint64_t *diff = nullptr;
  int rc = pool_get(ctx->device, POOL_VEC, plane + w_sel + w_slots + w_tv, &diff);
  if (rc) return rc;
  uint64_t *sel = diff + plane, *slots = sel + w_sel, *tvs = slots + w_slots;
  const unsigned g_plane = (unsigned)((plane + 255) / 256), g_slots = (unsigned)((w_slots + 255) / 256);
  const uint64_t one = vec_double2torus(1. / (2 * B));
  hipLaunchKernelGGL(tlwe_trivial_kernel, dim3(g_plane), dim3(256), 0, s, d_c, plane, row, (uint64_t)0);
  auto step = [&](const uint64_t *selector_N, int mode) -> int {   // c <- LUT_c[selector]
    int r2;
    if ((r2 = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel, selector_N, M, stream))) return r2;
    hipLaunchKernelGGL(cmp_slots_kernel, dim3(g_slots), dim3(256), 0, s, slots, d_c, (const uint64_t *)nullptr, (size_t)M, B, row, mode, one);
    if ((r2 = mosfhet_hip_trlwe_lut_packing_keyswitch_batch(ctx, vec->pksk, B, tvs, slots, M, stream))) return r2;
    return mosfhet_hip_functional_bootstrap_batch(ctx, vec->bsk, d_c, tvs, M, sel, M, B, stream);
  };
  for (int i = 0; i < d; i++) {
    hipLaunchKernelGGL(words_add2_kernel, dim3(g_plane), dim3(256), 0, s, diff, d_a + (size_t)i * plane, d_b + (size_t)i * plane, plane, 1, 0);   // diff = a - b
    if ((rc = step(diff, 0))) return rc;
  }
  if (a_signed && (rc = step(d_a + (size_t)(d - 1) * plane, 1))) return rc;
  if (b_signed && (rc = step(d_b + (size_t)(d - 1) * plane, 1))) return rc;
  hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, d_c, M, (size_t)row, ((size_t)row) - 1, one);
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// out[m] = lut[selector_m] for a CLEARTEXT table of `size` integers (ufhe_lut_integer, src/lut.c:23-47) and M encrypted selectors: ONE multi-value rotation per
// selector (phase 1 on its lowest digit), per output digit and table group one phase-2 launch over all M (the group's B digits are cleartext), then the encrypted-LUT
// tree over the selector's remaining digits.  d_out [d_out][M][N+1], d_sel [levels][M][N+1] (levels = log_B size), h_lut [size] host words.
extern "C" int mosfhet_hip_vec_lut_cleartext(mosfhet_hip_vec_t vec, uint64_t *d_out, const uint64_t *d_sel, const uint64_t *h_lut, int size, int d_out_digits, int M, void *stream) {
  if (!vec || !h_lut || M < 0 || size < 1 || d_out_digits < 1) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: bad argument");
  if (!vec->pksk) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: the handle has no LUT-packing key");
  const int B = vec->torus_base, logB = vec->log_torus_base;
  if (size < B) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: the table needs at least torus_base entries");
  if ((long long)d_out_digits * logB > 64) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: %d digits of %d bits do not fit the 64-bit table entries", d_out_digits, logB);
  if ((long long)M * (size / B) > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: too many units");
  for (int sz = size; sz > 1; sz /= B)
    if (sz % B) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: size %d is not a power of torus_base %d", size, B);
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_sel) return fail(MOSFHET_HIP_EINVAL, "vec_lut_cleartext: null buffer");
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, n = vec->bsk->n, row = N + 1, groups = size / B;
  const size_t plane = (size_t)M * row, w_sel = (size_t)M * (n + 1), w_rot = (size_t)M * (B + 1) * 2 * N, w_tab = (size_t)groups * plane;
  // a pool slot of its own: the tree below (vec_encrypted_lut) uses the thread's POOL_VEC slot itself
  uint64_t *sel = nullptr;
  int rc = pool_get(ctx->device, POOL_VEC3, w_sel + w_rot + w_tab, &sel);
  if (rc) return rc;
  uint64_t *rot = sel + w_sel, *table = rot + w_rot;
  if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel, d_sel, M, stream))) return rc;
  if ((rc = mosfhet_hip_multivalue_bootstrap_phase1_batch(ctx, vec->bsk, rot, sel, M, B, stream))) return rc;
  std::vector<int> dec(B);
  for (int j = 0; j < d_out_digits; j++) {
    for (int i = 0; i < groups; i++) {
      for (int q = 0; q < B; q++) dec[q] = (int)((h_lut[(size_t)i * B + q] >> (j * logB)) & (uint64_t)(B - 1));
      if ((rc = mosfhet_hip_multivalue_bootstrap_phase2_batch(ctx, table + (size_t)i * plane, dec.data(), rot, N, B, logB, M, stream))) return rc;
    }
    if (groups > 1 && (rc = mosfhet_hip_vec_encrypted_lut(vec, table, d_sel + plane, groups, M, stream))) return rc;
    HIP_TRY(hipMemcpyAsync(d_out + (size_t)j * plane, table, plane * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// ---- shifted additions and the multiplication (ufhe_sl_add_integer, ufhe_sl_addto_integer, ufhe_extend_integer, ufhe_mul_integer: src/integer.c:64-77,79-134,166-203) ----
// one carry step on digit plane c_i (ufhe_sl_add_integer's loop body, src/integer.c:94-104): c_i <- c_i reduced mod B, its carry into c_next (set = 1: c_next starts
// from the trivial 1/(4B), sl_add; set = 0: 1/(4B) is added to what c_next holds, sl_addto).  rot: [M][2][N] scratch.
static int vec_carry_step(mosfhet_hip_vec_t vec, uint64_t *c_i, uint64_t *c_next, int set, uint64_t *rot, int M, void *stream) {
  mosfhet_hip_ctx_t ctx = vec->ctx;
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, B = vec->torus_base, row = N + 1;
  const size_t plane = (size_t)M * row;
  int rc;
  if ((rc = mosfhet_hip_keyswitch_functional_bootstrap_batch(ctx, vec->ksk, vec->bsk, rot, vec->d_luts, 1, c_i, M, B, 0, stream))) return rc;
  if ((rc = mosfhet_hip_trlwe_mv_extract_batch(ctx, c_i, rot, N, 3, B, M, stream))) return rc;
  hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, c_i, M, (size_t)row, ((size_t)row) - 1, vec_double2torus(-0.25));
  if (c_next) {
    if (set) hipLaunchKernelGGL(tlwe_trivial_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, c_next, plane, row, vec_double2torus(1. / (4 * B)));
    else hipLaunchKernelGGL(tlwe_add_to_word_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, c_next, M, (size_t)row, ((size_t)row) - 1, vec_double2torus(1. / (4 * B)));
    if ((rc = mosfhet_hip_trlwe_mv_extract_batch(ctx, c_next, rot, N, 2, 1, M, stream))) return rc;
  }
  return MOSFHET_HIP_OK;
}

// ufhe_extend_integer (src/integer.c:64-77): digits [d_ini, dc) of c <- 0 (unsigned) or the sign extension of digit d_ini - 1 (signed: one bootstrap, dc - d_ini extractions)
static int vec_extend(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, int d_ini, int is_signed, uint64_t *rot, int M, void *stream) {
  if (dc <= d_ini) return MOSFHET_HIP_OK;
  mosfhet_hip_ctx_t ctx = vec->ctx;
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, B = vec->torus_base, row = N + 1, more = dc - d_ini;
  const size_t plane = (size_t)M * row;
  if (!is_signed) {
    hipLaunchKernelGGL(tlwe_trivial_kernel, dim3((unsigned)((plane * more + 255) / 256)), dim3(256), 0, s, d_c + (size_t)d_ini * plane, plane * more, row, (uint64_t)0);
    return MOSFHET_HIP_OK;
  }
  int rc;
  if ((rc = mosfhet_hip_keyswitch_functional_bootstrap_batch(ctx, vec->ksk, vec->bsk, rot, vec->d_luts + (size_t)4 * N, 1, d_c + (size_t)(d_ini - 1) * plane, M, B, 0, stream))) return rc;
  uint64_t *ext = nullptr;   // [M][more][row], then plane by plane into the digit-major integer
  if ((rc = pool_get(ctx->device, POOL_VEC, (size_t)M * more * row, &ext))) return rc;
  if ((rc = mosfhet_hip_trlwe_mv_extract_batch(ctx, ext, rot, N, 0, more, M, stream))) return rc;
  for (int q = 0; q < more; q++)
    HIP_TRY(hipMemcpy2DAsync(d_c + (size_t)(d_ini + q) * plane, (size_t)row * 8, ext + (size_t)q * row, (size_t)more * row * 8, (size_t)row * 8, (size_t)M, hipMemcpyDeviceToDevice, s));
  return MOSFHET_HIP_OK;
}

// c = a B^g + b B^h (ufhe_sl_add_integer, src/integer.c:79-107) for M integers; a [da][M][row], b [db][M][row], c [dc][M][row] (no aliasing)
static int vec_sl_add(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, const uint64_t *d_a, int da, int g, const uint64_t *d_b, int db, int h, int is_signed, uint64_t *rot, int M, void *stream) {
  mosfhet_hip_ctx_t ctx = vec->ctx;
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, row = N + 1;
  const size_t plane = (size_t)M * row;
  const unsigned g_plane = (unsigned)((plane + 255) / 256);
  int size = da + g > db + h ? da + g : db + h;
  size = is_signed ? da : (size + 1 < dc ? size + 1 : dc);
  int rc;
  hipLaunchKernelGGL(tlwe_trivial_kernel, dim3(g_plane), dim3(256), 0, s, d_c, plane, row, (uint64_t)0);
  for (int i = 0; i < size; i++) {
    uint64_t *c_i = d_c + (size_t)i * plane, *c_n = i != size - 1 ? c_i + plane : nullptr;
    if (i - g >= 0 && i - g < da) hipLaunchKernelGGL(words_add2_kernel, dim3(g_plane), dim3(256), 0, s, c_i, d_a + (size_t)(i - g) * plane, (const uint64_t *)nullptr, plane, 0, 1);
    if (i - h >= 0 && i - h < db) hipLaunchKernelGGL(words_add2_kernel, dim3(g_plane), dim3(256), 0, s, c_i, d_b + (size_t)(i - h) * plane, (const uint64_t *)nullptr, plane, 0, 1);
    if (i - g < 0 || i - h < 0) {
      if (c_n) hipLaunchKernelGGL(tlwe_trivial_kernel, dim3(g_plane), dim3(256), 0, s, c_n, plane, row, (uint64_t)0);
      continue;
    }
    if ((rc = vec_carry_step(vec, c_i, c_n, 1, rot, M, stream))) return rc;
  }
  return vec_extend(vec, d_c, dc, size, is_signed, rot, M, stream);
}

// b += a B^g (ufhe_sl_addto_integer, src/integer.c:110-134)
static int vec_sl_addto(mosfhet_hip_vec_t vec, uint64_t *d_b, int db, const uint64_t *d_a, int da, int g, int is_signed, uint64_t *rot, int M, void *stream) {
  hipStream_t s = pick(vec->ctx, stream);
  const int row = vec->bsk->N + 1;
  const size_t plane = (size_t)M * row;
  const int size = is_signed ? da : (da + g + 1 < db ? da + g + 1 : db);
  int rc;
  for (int i = 0; i < size; i++) {
    uint64_t *b_i = d_b + (size_t)i * plane;
    if (i - g >= 0 && i - g < da) hipLaunchKernelGGL(words_add2_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, b_i, d_a + (size_t)(i - g) * plane, (const uint64_t *)nullptr, plane, 0, 1);
    if (i - g < 0) continue;
    if ((rc = vec_carry_step(vec, b_i, i != size - 1 ? b_i + plane : nullptr, 0, rot, M, stream))) return rc;
  }
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_vec_sl_add(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, const uint64_t *d_a, int da, int g, const uint64_t *d_b, int db, int h, int is_signed, int M,
                                      void *stream) {
  if (!vec || M < 0 || da < 1 || db < 1 || dc < 1 || g < 0 || h < 0) return fail(MOSFHET_HIP_EINVAL, "vec_sl_add: bad argument");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_c || !d_a || !d_b || d_c == d_a || d_c == d_b) return fail(MOSFHET_HIP_EINVAL, "vec_sl_add: null or aliased buffer");
  if (is_signed && da > dc) return fail(MOSFHET_HIP_EINVAL, "vec_sl_add: the result has fewer digits than the signed operand a");
  if (M > 65535) return fail(MOSFHET_HIP_EINVAL, "vec_sl_add: M = %d (at most 65535 integers per call)", M);
  HIP_TRY(hipSetDevice(vec->ctx->device));
  uint64_t *rot = nullptr;
  int rc = pool_get(vec->ctx->device, POOL_VEC2, (size_t)M * 2 * vec->bsk->N, &rot);
  if (rc) return rc;
  if ((rc = vec_sl_add(vec, d_c, dc, d_a, da, g, d_b, db, h, is_signed, rot, M, stream))) return rc;
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

extern "C" int mosfhet_hip_vec_extend(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, int d_ini, int is_signed, int M, void *stream) {
  if (!vec || M < 0 || dc < 1 || d_ini < (is_signed ? 1 : 0) || d_ini > dc) return fail(MOSFHET_HIP_EINVAL, "vec_extend: bad argument");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_c) return fail(MOSFHET_HIP_EINVAL, "vec_extend: null buffer");
  if (M > 65535) return fail(MOSFHET_HIP_EINVAL, "vec_extend: M = %d (at most 65535 integers per call)", M);
  HIP_TRY(hipSetDevice(vec->ctx->device));
  uint64_t *rot = nullptr;
  int rc = pool_get(vec->ctx->device, POOL_VEC2, (size_t)M * 2 * vec->bsk->N, &rot);
  if (rc) return rc;
  if ((rc = vec_extend(vec, d_c, dc, d_ini, is_signed, rot, M, stream))) return rc;
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}

// c = a * b (ufhe_mul_integer, src/integer.c:166-203) for M pairs: schoolbook over the digits of a; per digit one multi-value rotation of the M selectors, the two
// product tables (x j mod B, x j div B for j < B) packed per integer, two bootstrap launches over all db x M digits of b, one shifted addition and one shifted
// accumulation.  a [da][M][row], b [db][M][row], c [dc][M][row]; signed operands as in the reference (the product keeps a's width and is sign-extended to dc digits).
extern "C" int mosfhet_hip_vec_mul(mosfhet_hip_vec_t vec, uint64_t *d_c, int dc, const uint64_t *d_a, int da, const uint64_t *d_b, int db, int is_signed, int M, void *stream) {
  if (!vec || M < 0 || da < 1 || db < 1 || dc < 1) return fail(MOSFHET_HIP_EINVAL, "vec_mul: bad argument");
  if (!vec->pksk) return fail(MOSFHET_HIP_EINVAL, "vec_mul: the handle has no LUT-packing key");
  if (is_signed && (da > dc || db > dc)) return fail(MOSFHET_HIP_EINVAL, "vec_mul: the result has fewer digits than a signed operand");
  if (M == 0) return MOSFHET_HIP_OK;
  if (!d_c || !d_a || !d_b || d_c == d_a || d_c == d_b) return fail(MOSFHET_HIP_EINVAL, "vec_mul: null or aliased buffer");
  mosfhet_hip_ctx_t ctx = vec->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const int N = vec->bsk->N, n = vec->bsk->n, B = vec->torus_base, logB = vec->log_torus_base, row = N + 1;
  const size_t plane = (size_t)M * row;
  int size = da + db + 1 < dc ? da + db + 1 : dc;
  if (is_signed) size = da;
  const int dres = db + (is_signed ? 0 : 1);
  if ((long long)db * M > 0x7fffffffLL || M > 65535) return fail(MOSFHET_HIP_EINVAL, "vec_mul: batch too large (M <= 65535: the extraction kernels index the batch by gridDim.z)");
  // temporaries of this call (a pool slot of its own: the carry steps use POOL_VEC / POOL_VEC2)
  const size_t w_sel = (size_t)db * M * (n + 1), w_rot = (size_t)M * (B + 1) * 2 * N, w_vals = (size_t)(B - 2) * plane, w_slots = (size_t)M * B * row, w_tv = (size_t)2 * M * 2 * N,
               w_tvt = (size_t)db * M * 2 * N, w_int = (size_t)(2 * db + dres) * plane, w_cr = (size_t)M * 2 * N;
  uint64_t *sel = nullptr;
  int rc = pool_get(ctx->device, POOL_VEC4, w_sel + w_rot + w_vals + w_slots + w_tv + w_tvt + w_int + w_cr, &sel);
  if (rc) return rc;
  uint64_t *rot = sel + w_sel, *vals = rot + w_rot, *slots = vals + w_vals, *tv = slots + w_slots, *tvt = tv + w_tv, *prod = tvt + w_tvt,
           *carry = prod + (size_t)db * plane, *res = carry + (size_t)db * plane, *crot = res + (size_t)dres * plane;
  std::vector<int> mat(B);
  hipLaunchKernelGGL(tlwe_trivial_kernel, dim3((unsigned)((plane * dc + 255) / 256)), dim3(256), 0, s, d_c, plane * dc, row, (uint64_t)0);   // ufhe_cleartext_integer(c, 0)
  // the selectors of b's digits do not depend on the digit of a: one key switch of all db x M
  if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel, d_b, db * M, stream))) return rc;
  for (int i = 0; i < da; i++) {
    const uint64_t *a_i = d_a + (size_t)i * plane;
    uint64_t *sel_a = slots;   // (the packing inputs are built after the rotation: the space is free until then)
    if ((rc = mosfhet_hip_tlwe_keyswitch_batch(ctx, vec->ksk, sel_a, a_i, M, stream))) return rc;
    if ((rc = mosfhet_hip_multivalue_bootstrap_phase1_batch(ctx, vec->bsk, rot, sel_a, M, B, stream))) return rc;
    for (int which = 0; which < 2; which++) {   // 0: x j mod B (mulmod), 1: x j div B (mulquo)
      for (int j = 2; j < B; j++) {
        for (int q = 0; q < B; q++) mat[q] = which ? (j * q) / B : (j * q) % B;   // row j of the matrices of src/ufhe.c:84-93
        if ((rc = mosfhet_hip_multivalue_bootstrap_phase2_batch(ctx, vals + (size_t)(j - 2) * plane, mat.data(), rot, N, B, logB, M, stream))) return rc;
      }
      hipLaunchKernelGGL(cmp_slots_kernel, dim3((unsigned)((w_slots + 255) / 256)), dim3(256), 0, s, slots, a_i, vals, (size_t)M, B, row, which == 0 ? 2 : 3, (uint64_t)0);
      if ((rc = mosfhet_hip_trlwe_lut_packing_keyswitch_batch(ctx, vec->pksk, B, tv + (size_t)which * M * 2 * N, slots, M, stream))) return rc;
      // every digit of b against its integer's table: the M tables tiled db times, one launch
      for (int j = 0; j < db; j++)
        HIP_TRY(hipMemcpyAsync(tvt + (size_t)j * M * 2 * N, tv + (size_t)which * M * 2 * N, (size_t)M * 2 * N * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
      if ((rc = mosfhet_hip_functional_bootstrap_batch(ctx, vec->bsk, which ? carry : prod, tvt, db * M, sel, db * M, B, stream))) return rc;
    }
    if ((rc = vec_sl_add(vec, res, dres, prod, db, 0, carry, db, 1, is_signed, crot, M, stream))) return rc;
    if ((rc = vec_sl_addto(vec, d_c, dc, res, dres, i, is_signed, crot, M, stream))) return rc;
  }
  if (is_signed && (rc = vec_extend(vec, d_c, dc, size, 1, crot, M, stream))) return rc;
  HIP_TRY(hipGetLastError());
  return MOSFHET_HIP_OK;
}
