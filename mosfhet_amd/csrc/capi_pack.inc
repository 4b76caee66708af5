// capi_pack.inc -- batches of LWE samples packed into TRLWE samples on the device: the reference's trlwe_full_packing_keyswitch (src/keyswitch.c:195-227, key from
// trlwe_new_full_packing_KS_key) as ONE call over a batch.  Own code: nothing of the reference is compiled in.  Kernels: pack_kernels.h.
//
//   d_in [total][n_in + 1], d_out [outputs][2][N], outputs = ceil(total / per); output o packs samples o per .. min(total, (o + 1) per) - 1, sample j at coefficient j
//
// The key is a mosfhet_hip_gak_t with entries = n_in (mosfhet_hip_trlwe_ksk_create / _generate): entry i switches from the constant polynomial s_in[i].
// split = 1 gives the reference's summation (one accumulator pair over all n_in t products, one rounding); split = P > 1 cuts the entries into P consecutive
// parts of ceil(n_in / P), each with an accumulator pair and a rounding of its own, so that a handful of outputs still fills the chip.  The caller chooses P
// (mosfhet_hip_tlwe_pack_plan recommends one): the call never does, so no word depends on the batch size.
//
// One place decides the shape of a call (pack_plan: for the launcher and for mosfhet_hip_tlwe_pack_plan).  The transposed staging [outputs of a round][n_in][N] and
// the partial sums [outputs of a round][P][2][N] live in the calling thread's pool (slots POOL_PACK_COLS, POOL_PACK_PARTS): a call neither allocates per call nor
// synchronises, and is capturable on its one stream once a call of the same size has grown the pool.  The staging is bounded by
// mosfhet_hip_set_tlwe_pack_workspace; a larger batch runs in rounds of whole outputs, which changes no word.
constexpr long long PACK_WORKSPACE_DEFAULT = 256ll << 20;
static std::atomic<long long> g_pack_workspace{PACK_WORKSPACE_DEFAULT};
constexpr int PACK_MAX_SPLIT = 64;         // bounds the partial-sum staging
constexpr int PACK_MIN_PART = 8;           // entries per part the recommendation never goes below
constexpr int PACK_MAX_ROUND = 32768;      // outputs per round at most: the transposition and the sum index them by gridDim.y

extern "C" int mosfhet_hip_set_tlwe_pack_workspace(long long bytes) {
  if (bytes < 0) return fail(MOSFHET_HIP_EINVAL, "set_tlwe_pack_workspace: bytes = %lld (0 restores the default)", bytes);
  g_pack_workspace = bytes ? bytes : PACK_WORKSPACE_DEFAULT;
  return MOSFHET_HIP_OK;
}

struct PackPlan { int outputs, split, part_entries, round, rounds; long long teams, cols_bytes, key_bytes, parts_bytes; };

// teams resident on `cus` CUs at launch bound 1 (one wavefront per SIMD, four SIMDs per CU)
static long long pack_resident_teams(int N, int cus) { return (long long)cus * 4 / (N / 16 / 64); }

// The one place that decides the shape of a call.  split = 0: recommend one -- enough parts to fill the resident teams, never fewer than PACK_MIN_PART entries per
// part, never above min(n_in, PACK_MAX_SPLIT), and 1 as soon as the outputs alone fill the chip.
static int pack_plan(const char *who, int N, int n_in, int t, int total, int per, int split, int cus, long long workspace, PackPlan *r) {
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (n_in < 1) return fail(MOSFHET_HIP_EINVAL, "%s: n_in = %d", who, n_in);
  if (t < 1 || t > 63) return fail(MOSFHET_HIP_EINVAL, "%s: t = %d (1 .. 63)", who, t);
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  if (per < 1 || per > N) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N = %d)", who, per, N);
  const int max_split = n_in < PACK_MAX_SPLIT ? n_in : PACK_MAX_SPLIT;
  if (split < 0 || split > max_split) return fail(MOSFHET_HIP_EINVAL, "%s: split = %d (1 .. min(n_in, %d) = %d; 0 asks the plan for one)", who, split, PACK_MAX_SPLIT, max_split);
  if (cus < 1) return fail(MOSFHET_HIP_EINVAL, "%s: cus = %d", who, cus);
  if (workspace < 0) return fail(MOSFHET_HIP_EINVAL, "%s: workspace_bytes = %lld (0: the current setting)", who, workspace);
  if (workspace == 0) workspace = g_pack_workspace.load(std::memory_order_relaxed);
  r->outputs = (int)(((long long)total + per - 1) / per);
  if (split == 0) {
    const long long resident = pack_resident_teams(N, cus);
    long long want = r->outputs > 0 && r->outputs < resident ? (resident + r->outputs - 1) / r->outputs : 1;
    const long long most = n_in / PACK_MIN_PART > 1 ? n_in / PACK_MIN_PART : 1;
    if (want > most) want = most;
    if (want > max_split) want = max_split;
    split = (int)want;
  }
  r->split = split;
  r->part_entries = (n_in + split - 1) / split;
  // byte counts: refuse what does not fit a signed 64-bit field
  const unsigned __int128 limit = (unsigned __int128)0x7fffffffffffffffLL;
  const unsigned __int128 one = (unsigned __int128)n_in * (unsigned __int128)N * 8;        // transposed staging of one output
  const unsigned __int128 key = (unsigned __int128)r->part_entries * (unsigned __int128)t * (unsigned __int128)N * 16;
  if (one > limit || key > limit || one * (unsigned __int128)(r->outputs ? r->outputs : 1) > limit)
    return fail(MOSFHET_HIP_EINVAL, "%s: n_in = %d: %d outputs x n_in x N = %d words x 8 bytes (or the key rows of a part) do not fit a 64-bit byte count", who, n_in, r->outputs, N);
  if ((long long)one > workspace)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the transposed columns of one output (%lld): mosfhet_hip_set_tlwe_pack_workspace", who, workspace,
                (long long)one);
  long long fit = workspace / (long long)one;
  if (fit > PACK_MAX_ROUND) fit = PACK_MAX_ROUND;
  r->round = r->outputs < fit ? r->outputs : (int)fit;
  r->rounds = r->outputs ? (r->outputs + r->round - 1) / r->round : 0;
  r->teams = (long long)r->round * split;
  r->cols_bytes = (long long)r->round * (long long)one;
  r->key_bytes = (long long)key;
  r->parts_bytes = split > 1 ? r->teams * 2 * N * 8 : 0;
  return MOSFHET_HIP_OK;
}

// plan = { outputs, split used, entries per part, outputs per round, rounds, teams of the main launch, transposed-staging bytes per round, key bytes one team reads }
extern "C" int mosfhet_hip_tlwe_pack_plan(int N, int n_in, int t, int total, int per, int split, int cus, long long workspace_bytes, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "tlwe_pack_plan: null plan");
  PackPlan r;
  const int rc = pack_plan("tlwe_pack_plan", N, n_in, t, total, per, split, cus, workspace_bytes, &r);
  if (rc) return rc;
  plan[0] = r.outputs; plan[1] = r.split; plan[2] = r.part_entries; plan[3] = r.round; plan[4] = r.rounds; plan[5] = r.teams; plan[6] = r.cols_bytes; plan[7] = r.key_bytes;
  return MOSFHET_HIP_OK;
}

// one launch of each kernel per residency round of whole outputs
template <class F>
static int launch_tlwe_pack(const PackPlan &plan, PackParams p, const d2 *key, const d2 *tw, int t, int base_bit, int total, hipStream_t s) {
  const uint64_t *in = p.in;
  uint64_t *out = p.out;
  const size_t w = (size_t)p.n_in + 1;
  const unsigned tiles = (unsigned)(F::N / PACK_TILE) * (unsigned)((p.n_in + 1 + PACK_TILE - 1) / PACK_TILE);
  for (int o0 = 0; o0 < plan.outputs; o0 += plan.round) {
    p.outputs = plan.outputs - o0 < plan.round ? plan.outputs - o0 : plan.round;
    const long long first = (long long)o0 * p.per;
    p.samples = (int)(total - first < (long long)p.outputs * p.per ? total - first : (long long)p.outputs * p.per);
    p.in = in + (size_t)first * w;
    p.out = out + (size_t)o0 * 2 * F::N;
    hipLaunchKernelGGL(tlwe_pack_transpose_kernel, dim3(tiles, (unsigned)p.outputs), dim3(256), 0, s, p, F::N);
    hipLaunchKernelGGL(tlwe_pack_kernel<F>, dim3((unsigned)p.outputs * (unsigned)p.split), dim3(F::THREADS), 0, s, p, key, tw, t, base_bit);
    if (p.split > 1) hipLaunchKernelGGL(tlwe_pack_sum_kernel, dim3((unsigned)(2 * F::N / 256), (unsigned)p.outputs), dim3(256), 0, s, p, F::N);
  }
  return launched();
}

// Null handles and scalar ranges come before any handle is read and before any HIP call.
extern "C" int mosfhet_hip_tlwe_pack_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t pk, uint64_t *d_out, const uint64_t *d_in, int total, int per, int split, void *stream) {
  const char *who = "tlwe_pack";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!pk) return fail(MOSFHET_HIP_EINVAL, "%s: null pk", who);
  if (per < 1 || per > 4096) return fail(MOSFHET_HIP_EINVAL, "%s: per = %d (1 .. N)", who, per);
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  if (split < 1 || split > PACK_MAX_SPLIT) return fail(MOSFHET_HIP_EINVAL, "%s: split = %d (1 .. min(n_in, %d); mosfhet_hip_tlwe_pack_plan recommends one)", who, split, PACK_MAX_SPLIT);
  if (total == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (pk->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: pk belongs to another context (device %d): mosfhet_hip_gak_clone makes a copy for this one", who, pk->device);
  PackPlan plan;
  int rc = pack_plan(who, pk->N, pk->entries, pk->t, total, per, split, 256, 0, &plan);   // the ring, per <= N, split <= n_in, the size limits
  if (rc) return rc;
  if (ranges_overlap(d_out, (size_t)plan.outputs * 2 * pk->N * sizeof(uint64_t), d_in, (size_t)total * ((size_t)pk->entries + 1) * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  HIP_TRY(hipSetDevice(ctx->device));
  PackParams p = {};
  p.in = d_in; p.out = d_out; p.n_in = pk->entries; p.per = per; p.split = plan.split; p.part_entries = plan.part_entries;
  uint64_t *cols = nullptr, *parts = nullptr;
  if ((rc = pool_get(ctx->device, POOL_PACK_COLS, (size_t)(plan.cols_bytes / (long long)sizeof(uint64_t)), &cols))) return rc;
  if (plan.split > 1 && (rc = pool_get(ctx->device, POOL_PACK_PARTS, (size_t)(plan.parts_bytes / (long long)sizeof(uint64_t)), &parts))) return rc;
  p.cols = cols; p.parts = parts;
  hipStream_t s = pick(ctx, stream);
  RING_DISPATCH(ctx, pk->N, rc = launch_tlwe_pack<F>(plan, p, pk->d_ak, TW, pk->t, pk->base_bit, total, s));
  return rc;
}
