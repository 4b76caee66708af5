// capi_trace.inc -- the LWE -> TRLWE switch by the trace and the gadget -> TRGSW conversion on the device, over batches.  Own code: nothing of the reference is
// compiled in.  Kernels: trace_kernels.h.
//
//   mosfhet_hip_tlwe_trace_pack_batch             trlwe_packing1_keyswitch_CDKS21 (src/keyswitch.c:526-546): d_in [count][N + 1] -> d_out [count][2][N], entries
//                                                 entry0 .. entry0 + log2 N - 1 of the set (trlwe_new_packing1_KS_key_CDKS21's order: entry j switches from
//                                                 s(X^(N / 2^j + 1))); one launch, the accumulator never leaves the chip
//   mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch   trlwe_RLWE_priv_keyswitch (src/keyswitch.c:65-97): entries entry0 (from s_in v) and entry0 + 1 (from v); one launch
//   mosfhet_hip_trgsw_from_gadget_batch           trgsw_from_gadget (src/keyswitch.c:559-572): d_gadget [count][l][2][N] -> d_out_dft [count][2l][2][N/2] complex, the
//                                                 selector layout of the leveled-LUT calls; count * l teams, no torus-domain word written
//
// The keys are ordinary mosfhet_hip_gak_t sets (a trace key at N = 2048, t = 4 is 1.4 MiB): nothing to generate beyond mosfhet_hip_trlwe_ksk_create / _generate,
// nothing to hold per call.  The calls allocate nothing, never synchronise and are capturable from the first call.  One place checks the shape of a call
// (trace_plan: for the launchers and for mosfhet_hip_trace_plan).
struct TracePlan { int entries_read, threads; long long teams, forwards, inverses, key_bytes; };

static int trace_log2(int N) { int r = 0; while ((1 << r) < N) r++; return r; }

// entries: what the set holds; l is read for TRACE_KIND_GADGET only
static int trace_plan(const char *who, int kind, int N, int t, int base_bit, int entries, int entry0, int l, int count, TracePlan *r) {
  if (kind < TRACE_KIND_PACK || kind > TRACE_KIND_GADGET) return fail(MOSFHET_HIP_EINVAL, "%s: kind = %d (0 trace pack, 1 private key switch, 2 TRGSW from gadget)", who, kind);
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (t < 1 || base_bit < 1 || t * base_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: t = %d, base_bit = %d (both >= 1, t base_bit < 64)", who, t, base_bit);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (entry0 < 0) return fail(MOSFHET_HIP_EINVAL, "%s: entry0 = %d", who, entry0);
  if (kind == TRACE_KIND_GADGET && (l < 1 || l > 6)) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  const int steps = trace_log2(N), need = kind == TRACE_KIND_PACK ? steps : 2;
  if (entries < 1 || (long long)entry0 + need > entries)
    return fail(MOSFHET_HIP_EINVAL, "%s: the key set holds %d entries, entry0 = %d needs entry0 + %d = %lld%s", who, entries, entry0, need, (long long)entry0 + need,
                kind == TRACE_KIND_PACK ? " (log2 N switches of the trace)" : " (the keys of s_in v and of v)");
  const long long teams = (long long)count * (kind == TRACE_KIND_GADGET ? l : 1);
  if (teams > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d x l = %d teams do not fit one launch", who, count, l);
  r->entries_read = need; r->threads = N / 16; r->teams = teams;
  r->forwards = (long long)need * t + (kind == TRACE_KIND_GADGET ? 4 : 0);
  r->inverses = (long long)need * 2;
  r->key_bytes = (long long)need * t * N * 16;
  return MOSFHET_HIP_OK;
}

// plan = { key entries a team reads, teams of the launch, threads per team, forward transforms per team, inverse transforms per team, key bytes a team reads }
extern "C" int mosfhet_hip_trace_plan(int kind, int N, int t, int base_bit, int entries, int entry0, int l, int count, long long plan[6]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "trace_plan: null plan");
  TracePlan r;
  const int rc = trace_plan("trace_plan", kind, N, t, base_bit, entries, entry0, l, count, &r);
  if (rc) return rc;
  plan[0] = r.entries_read; plan[1] = r.teams; plan[2] = r.threads; plan[3] = r.forwards; plan[4] = r.inverses; plan[5] = r.key_bytes;
  return MOSFHET_HIP_OK;
}

// The checks every call shares.  Null handles and scalar ranges come before any handle is read and before any HIP call; *run = false: nothing to do (count == 0).
static int trace_check(const char *who, int kind, mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, const void *d_out, const void *d_in, int l, int count, bool *run) {
  *run = false;
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!tks) return fail(MOSFHET_HIP_EINVAL, "%s: null tks", who);
  if (count < 0) return fail(MOSFHET_HIP_EINVAL, "%s: count = %d", who, count);
  if (entry0 < 0) return fail(MOSFHET_HIP_EINVAL, "%s: entry0 = %d", who, entry0);
  if (kind == TRACE_KIND_GADGET && (l < 1 || l > 6)) return fail(MOSFHET_HIP_EINVAL, "%s: l = %d (1 .. 6)", who, l);
  if (count == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (tks->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: tks belongs to another context (device %d): mosfhet_hip_gak_clone makes a copy for this one", who, tks->device);
  TracePlan plan;
  const int rc = trace_plan(who, kind, tks->N, tks->t, tks->base_bit, tks->entries, entry0, l, count, &plan);
  if (rc) return rc;
  *run = true;
  return MOSFHET_HIP_OK;
}

// one launch of trace_conversions_kernel: `teams` workgroups of the ring's team
static int launch_trace(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int kind, int entry0, const uint64_t *in, uint64_t *out, d2 *sel, int l, unsigned teams, hipStream_t s) {
  TraceParams p = {};
  p.key = tks->d_ak + (size_t)entry0 * tks->t * 2 * (tks->N / 2);
  p.in = in; p.out = out; p.sel = sel; p.kind = kind; p.t = tks->t; p.base_bit = tks->base_bit; p.l = l;
  RING_DISPATCH(ctx, tks->N, p.tw = TW; hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3(teams), dim3(F::THREADS), 0, s, p));
  return launched();
}

extern "C" int mosfhet_hip_tlwe_trace_pack_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  const char *who = "tlwe_trace_pack";
  bool run;
  const int rc = trace_check(who, TRACE_KIND_PACK, ctx, tks, entry0, d_out, d_in, 0, count, &run);
  if (rc || !run) return rc;
  const int N = tks->N;
  if (ranges_overlap(d_out, (size_t)count * 2 * N * sizeof(uint64_t), d_in, (size_t)count * ((size_t)N + 1) * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_trace(ctx, tks, TRACE_KIND_PACK, entry0, d_in, d_out, nullptr, 1, (unsigned)count, pick(ctx, stream));
}

// ---- many samples per output: the packing tree of 2^log_per leaves, then the rest of the trace (TRACE_KIND_MANY, internal to TraceParams) ----
// Levels 1 .. L - 1 write their results to the calling thread's pool (slot POOL_TRACE_MANY): level 1 [round][n / 2][2][N] into region A, level 2 [round][n / 4][2][N]
// into region B behind it, level 3 into A again, ...; level L writes d_out and runs the tail.  The pool is bounded by mosfhet_hip_set_tlwe_pack_workspace; a larger
// batch runs in rounds of whole outputs, which changes no word.
struct TraceManyPlan { int outputs, launches, merges, tail, round, rounds; long long teams, pool_bytes, region_a_words; };

// The one place that decides the shape of a call (for the launcher and for mosfhet_hip_tlwe_trace_pack_many_plan).
static int trace_many_plan(const char *who, int N, int t, int base_bit, int entries, int entry0, int total, int log_per, long long workspace, TraceManyPlan *r) {
  if (!ring_ok(N)) return fail(MOSFHET_HIP_EINVAL, "%s: ring degree N = %d not supported here (1024, 2048, 4096)", who, N);
  if (t < 1 || base_bit < 1 || t * base_bit >= 64) return fail(MOSFHET_HIP_EINVAL, "%s: t = %d, base_bit = %d (both >= 1, t base_bit < 64)", who, t, base_bit);
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  if (entry0 < 0) return fail(MOSFHET_HIP_EINVAL, "%s: entry0 = %d", who, entry0);
  const int steps = trace_log2(N);
  if (log_per < 0 || log_per > steps) return fail(MOSFHET_HIP_EINVAL, "%s: log_per = %d (0 .. log2 N = %d)", who, log_per, steps);
  if (entries < 1 || (long long)entry0 + steps > entries)
    return fail(MOSFHET_HIP_EINVAL, "%s: the key set holds %d entries, entry0 = %d needs entry0 + %d = %lld (log2 N switches: the merges take the last log_per, the trace the rest)",
                who, entries, entry0, steps, (long long)entry0 + steps);
  if (workspace < 0) return fail(MOSFHET_HIP_EINVAL, "%s: workspace_bytes = %lld (0: the current setting)", who, workspace);
  if (workspace == 0) workspace = g_pack_workspace.load(std::memory_order_relaxed);
  const long long n = 1ll << log_per;
  r->outputs = (int)(((long long)total + n - 1) / n);
  r->launches = log_per ? log_per : 1;
  r->merges = (int)(n - 1);
  r->tail = steps - log_per;
  const long long trlwe = (long long)2 * N * 8;
  r->region_a_words = log_per >= 2 ? (n / 2) * 2 * N : 0;                         // per output
  const long long one = ((log_per >= 2 ? n / 2 : 0) + (log_per >= 3 ? n / 4 : 0)) * trlwe;   // pool bytes of one output
  if (one > workspace)
    return fail(MOSFHET_HIP_EINVAL, "%s: the workspace bound of %lld bytes does not hold the intermediate levels of one output (%lld): mosfhet_hip_set_tlwe_pack_workspace", who,
                workspace, one);
  const long long fit = one ? workspace / one : r->outputs;
  r->round = r->outputs < fit ? r->outputs : (int)fit;
  r->rounds = r->outputs ? (r->outputs + r->round - 1) / r->round : 0;
  r->teams = log_per ? (long long)r->round * (n / 2) : r->round;
  if (r->teams > 0x7fffffffLL) return fail(MOSFHET_HIP_EINVAL, "%s: %d outputs x %lld merges of level 1 do not fit one launch", who, r->round, n / 2);
  r->pool_bytes = (long long)r->round * one;
  return MOSFHET_HIP_OK;
}

// plan = { outputs, launches per round, teams of the first launch of a round, merge steps per output, tail steps, outputs per round, rounds, pool bytes per round }
extern "C" int mosfhet_hip_tlwe_trace_pack_many_plan(int N, int t, int base_bit, int entries, int entry0, int total, int log_per, long long workspace_bytes, long long plan[8]) {
  if (!plan) return fail(MOSFHET_HIP_EINVAL, "tlwe_trace_pack_many_plan: null plan");
  TraceManyPlan r;
  const int rc = trace_many_plan("tlwe_trace_pack_many_plan", N, t, base_bit, entries, entry0, total, log_per, workspace_bytes, &r);
  if (rc) return rc;
  plan[0] = r.outputs; plan[1] = r.launches; plan[2] = r.teams; plan[3] = r.merges; plan[4] = r.tail; plan[5] = r.round; plan[6] = r.rounds; plan[7] = r.pool_bytes;
  return MOSFHET_HIP_OK;
}

// Null handles and scalar ranges come before any handle is read and before any HIP call.
extern "C" int mosfhet_hip_tlwe_trace_pack_many_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out, const uint64_t *d_in, int total, int log_per,
                                                      void *stream) {
  const char *who = "tlwe_trace_pack_many";
  if (!ctx) return fail(MOSFHET_HIP_EINVAL, "%s: null ctx", who);
  if (!tks) return fail(MOSFHET_HIP_EINVAL, "%s: null tks", who);
  if (total < 0) return fail(MOSFHET_HIP_EINVAL, "%s: total = %d", who, total);
  if (entry0 < 0) return fail(MOSFHET_HIP_EINVAL, "%s: entry0 = %d", who, entry0);
  if (log_per < 0 || log_per > 12) return fail(MOSFHET_HIP_EINVAL, "%s: log_per = %d (0 .. log2 N)", who, log_per);
  if (total == 0) return MOSFHET_HIP_OK;
  if (!d_out || !d_in) return fail(MOSFHET_HIP_EINVAL, "%s: null buffer", who);
  if (tks->ctx != ctx) return fail(MOSFHET_HIP_EINVAL, "%s: tks belongs to another context (device %d): mosfhet_hip_gak_clone makes a copy for this one", who, tks->device);
  TraceManyPlan plan;
  int rc = trace_many_plan(who, tks->N, tks->t, tks->base_bit, tks->entries, entry0, total, log_per, 0, &plan);
  if (rc) return rc;
  const int N = tks->N;
  if (ranges_overlap(d_out, (size_t)plan.outputs * 2 * N * sizeof(uint64_t), d_in, (size_t)total * ((size_t)N + 1) * sizeof(uint64_t)))
    return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in", who);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  if (log_per == 0) return launch_trace(ctx, tks, TRACE_KIND_PACK, entry0, d_in, d_out, nullptr, 1, (unsigned)total, s);
  uint64_t *pool = nullptr;
  if (plan.pool_bytes && (rc = pool_get(ctx->device, POOL_TRACE_MANY, (size_t)(plan.pool_bytes / (long long)sizeof(uint64_t)), &pool))) return rc;
  TraceParams p = {};
  p.key = tks->d_ak + (size_t)entry0 * tks->t * 2 * (N / 2);
  p.kind = TRACE_KIND_MANY; p.t = tks->t; p.base_bit = tks->base_bit; p.l = 1;
  for (int o0 = 0; o0 < plan.outputs; o0 += plan.round) {
    const int outputs = plan.outputs - o0 < plan.round ? plan.outputs - o0 : plan.round;
    const long long first = (long long)o0 << log_per;
    uint64_t *region[2] = {pool, pool + (size_t)plan.round * (size_t)plan.region_a_words};   // levels 1, 3, ... write A, levels 2, 4, ... B; both sized for plan.round outputs
    const uint64_t *src = d_in + (size_t)first * ((size_t)N + 1);
    for (int lvl = 1; lvl <= log_per; lvl++) {
      p.lvl = lvl; p.cnt_log = log_per - lvl; p.tail = lvl == log_per ? plan.tail : 0;
      p.total = (int)(total - first);
      p.in = src;
      p.out = lvl == log_per ? d_out + (size_t)o0 * 2 * N : region[(lvl - 1) & 1];
      const unsigned teams = (unsigned)outputs << p.cnt_log;
      RING_DISPATCH(ctx, N, p.tw = TW; hipLaunchKernelGGL(trace_conversions_kernel<F>, dim3(teams), dim3(F::THREADS), 0, s, p));
      src = p.out;
    }
  }
  return launched();
}

extern "C" int mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, uint64_t *d_out, const uint64_t *d_in, int count, void *stream) {
  const char *who = "trlwe_rlwe_priv_keyswitch";
  bool run;
  const int rc = trace_check(who, TRACE_KIND_PRIV, ctx, tks, entry0, d_out, d_in, 0, count, &run);
  if (rc || !run) return rc;
  const size_t bytes = (size_t)count * 2 * tks->N * sizeof(uint64_t);
  if (d_out != d_in && ranges_overlap(d_out, bytes, d_in, bytes)) return fail(MOSFHET_HIP_EINVAL, "%s: d_out overlaps d_in without being d_in (in place is fine, a shifted overlap is not)", who);
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_trace(ctx, tks, TRACE_KIND_PRIV, entry0, d_in, d_out, nullptr, 1, (unsigned)count, pick(ctx, stream));
}

extern "C" int mosfhet_hip_trgsw_from_gadget_batch(mosfhet_hip_ctx_t ctx, mosfhet_hip_gak_t tks, int entry0, double *d_out_dft, const uint64_t *d_gadget, int l, int count, void *stream) {
  const char *who = "trgsw_from_gadget";
  bool run;
  const int rc = trace_check(who, TRACE_KIND_GADGET, ctx, tks, entry0, d_out_dft, d_gadget, l, count, &run);
  if (rc || !run) return rc;
  const size_t in_bytes = (size_t)count * l * 2 * tks->N * sizeof(uint64_t);
  if (ranges_overlap(d_out_dft, 2 * in_bytes, d_gadget, in_bytes)) return fail(MOSFHET_HIP_EINVAL, "%s: d_out_dft overlaps d_gadget", who);
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_trace(ctx, tks, TRACE_KIND_GADGET, entry0, d_gadget, nullptr, (d2 *)d_out_dft, l, (unsigned)count * (unsigned)l, pick(ctx, stream));
}
