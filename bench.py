#!/usr/bin/env python3
"""bench.py -- programmable bootstraps / second on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch: `--batch` (default 4096) independent
programmable_bootstrap calls at SET_1 (n=585, N=1024, k=1, l=2, Bg=2^8: BASELINE.json configs[1]) on each
GPU, inputs and the bootstrap key already resident in HBM.  With --gpus N > 1 (launched by
torch.distributed.run, one rank per GPU) every rank bootstraps its own batch against its own replica of the
key -- no collective on the data path (weak scaling); the only collectives are the barrier and the
max-over-ranks of the timed region.

A plain run sets up, warms up, times --steps steps and prints ONE JSON line (rank 0) with the contract fields (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds of one timed step, ...) and nothing else.  --dump-outputs DIR writes the outputs of the last
timed step to DIR/programmable_bootstrap_out.npy (float64 torus values; the inputs are seeded, identical from run to run).

With --full the line also carries the other legs, each run after the timed region (the CPU baseline and the decrypt check of the first step's
outputs, max_phase_error_log2, before it):
  roofline     : the dominant kernel (pbs_kernel) against the roof that binds it, FP64 vector issue: SURVEY.md 8(d)'s FLOP model
                 (171,008 FLOP per CMUX step x n steps x B) over the kernel's average launch duration, measured live with hipEvents on
                 the launch stream, against the 78.6 TFLOP/s FP64 vector peak.  SURVEY 8(d)'s byte model (bootstrap key streamed once
                 per ciphertext) is kept as `hbm_algorithmic`, labelled: it is NOT a bound, the key is shared by the batch through L2;
                 `traffic` = PMC-measured memory-side bytes per launch, only when profiles/latest_traffic.json was taken from THIS build;
  roofline_external_product : the kernel BASELINE.json's target names (trgsw_mul_trlwe_DFT + trlwe_from_DFT over a large batch against one
                 key entry, 32 KiB of ciphertext I/O per unit) against HBM bandwidth, timed live the same way; a sample of its outputs is checked
                 by phase (BK_i = TRGSW(s_i): phase(BK_i (.) c) = s_i phase(c), within the reference's 2^54);
  roofline_external_product_lvl2 : the same at N = 2048, l = 4 (64 KiB per unit, 256 KiB key entry);
  configs_3_4  : BASELINE.json configs[3] and [4] (N = 1: on this GPU; N > 1: each batch of 1024 SPLIT over the ranks, strong scaling, max over ranks): 1024 x circuit_bootstrap_3, full-domain functional bootstrap, multi-value bootstrap
                 (8 LUTs) and Galois-automorphism bootstrap at N = 2048, each checked by phase, each with the FP64 share of its blind rotations, the circuit
                 bootstrap's packing switches against the 64-bit-add issue rate that bounds them, and ONE GPU's share of the batch when it is split over 8 (128 inputs);
  lvl2_bootstraps : BASELINE.json configs[2] for the record (4096 programmable bootstraps at N = 2048, l = 4 on this GPU: rate, FP64-model fraction,
                 outputs checked by phase); not part of `value`; small_batches: 1 and 128 bootstraps on two CUs each (pbs_split_kernel) against one CU each;
  gate         : SURVEY 8(f).1 -- 4096 x (tlwe_keyswitch + functional_bootstrap) at SET_1, one call, checked by phase;
  vector_callers : SURVEY 8(f).4 -- 256 radix-4 integers through add + ReLU + 16-entry encrypted look-up at the reference application's parameter set, decrypted and compared;
  value_regime : how `value` was launched (steps alternate over --streams HIP streams) next to roofline.kernel_ms (the launch alone, timed right
                 after the timed region) and roofline.kernel_ms_in_stream_regime (an event pair around every launch of the same alternating schedule);
  sustained    : the same step back to back for >= 2.5 s (N = 1);
  single_bootstrap_ms : one programmable bootstrap alone (latency kernel), hipEvents on the launch stream;
  replicas     : N > 1 only -- every rank holds the same key (same seed), different ciphertexts, and its outputs decrypt;
  cpu_baseline : the reference's own programmable_bootstrap (oracle/_ref, built from /root/reference) timed on
                 this box's host cores on a bounded sample (N=1 only), plus config 1 (one FFNT pure-C bootstrap).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEED = 0x4D4F5346
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s
FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X FP64 vector peak: 256 CUs x 4 SIMDs x 16 FMA lanes x 2 FLOP x 2.4 GHz (one v_fma_f64 per 4 cycles per SIMD,
                                # tools/ubench: 4.2 cycles measured; the FP64 MFMA runs on the same units at the same rate)


def algorithmic_bytes_per_bootstrap(P):
    """bootstrap key streamed once per ciphertext + LWE in + test vector + LWE out."""
    k, N, n, l = P["k"], P["N"], P["n"], P["l"]
    return n * (k + 1) ** 2 * l * N * 8 + (n + 1) * 8 + (k + 1) * N * 8 + (k * N + 1) * 8


def flops_per_cmux(P):
    """5 M log2 M per M-point complex FFT ((k+1) l forward + (k+1) inverse) + 8 per complex multiply-add."""
    k, N, l = P["k"], P["N"], P["l"]
    M = N // 2
    fft = 5 * M * (M.bit_length() - 1)
    return ((k + 1) * l + (k + 1)) * fft + 8 * (k + 1) ** 2 * l * M


def flops_per_ga_step(P):
    """One step of the Galois-automorphism blind rotation (src/bootstrap_ga.c:39-60): an external product + trlwe_eval_automorphism's key switch of component a
    (src/keyswitch.c:162-193: l digit polynomials forward, k + 1 inverse transforms, l (k + 1) complex multiply-adds per point), priced like flops_per_cmux."""
    k, N, l = P["k"], P["N"], P["l"]
    M = N // 2
    fft = 5 * M * (M.bit_length() - 1)
    return flops_per_cmux(P) + (l + (k + 1)) * fft + 8 * l * (k + 1) * M


def lvl2_keys(eng, ma, host):
    """Key material of the TFHEpp lvl2 set (N = 2048, l = 4, n = 632) for the configs[2..4] legs: secrets on the host, the bootstrap key generated on the device."""
    P2 = dict(ma.PARAMS_LVL2)
    host.seed(SEED + 2)
    lk2 = host.LweKey(P2["n"], P2["lwe_sigma"])
    rk2 = host.RlweKey(P2["N"], 1, P2["rlwe_sigma"])
    bsk2 = eng.generate_bootstrap_key(rk2.s[0], lk2.s, P2["l"], P2["Bg_bit"], P2["rlwe_sigma"], seed=SEED)
    return P2, lk2, rk2, bsk2


def timed_ms(torch, fn, reps=3, groups=2):
    """average duration of `reps` back-to-back calls of fn (launches on torch's current stream, which the engine launches on), hipEvents on that stream; best of `groups`"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = None
    for _ in range(groups):
        ev[0].record(torch.cuda.current_stream())
        for _ in range(reps):
            fn()
        ev[1].record(torch.cuda.current_stream())
        ev[1].synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        best = ms if best is None else min(best, ms)
    return best


def lvl2_bootstrap_leg(eng, ma, host, torch, keys, B2=4096):
    """BASELINE.json configs[2] beside the headline: B2 programmable bootstraps at the TFHEpp lvl2 set (N = 2048, l = 4, n = 632) on this GPU, key generated on
    the device, launches timed with events on the launch stream (one launch per residency round of 1024, the teams of a round re-aligned per XCD: DESIGN.md 4.1);
    every output checked by PHASE against its LUT slot (the reference's criterion, test/tests.c:1560 -- no oracle on the measured path)."""
    P2, lk2, rk2, bsk2 = keys
    lut = np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64)
    d_tv2 = ma.to_device(host.torus_packing(lut, 1, P2["N"])[None], eng.device)
    d_ct2 = ma.to_device(host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(B2)], lk2), eng.device)
    out2 = eng.programmable_bootstrap(bsk2, d_tv2, d_ct2, 3)
    torch.cuda.synchronize()
    ph = host.tlwe_phase(ma.to_numpy(out2), rk2.extracted_lwe_key().s)
    err = np.abs((ph - lut[np.arange(B2) % 4]).astype(np.int64).astype(np.float64)).max()
    ms = min(eng.time_programmable_bootstrap(bsk2, d_tv2, d_ct2, 3, 3, out=out2) for _ in range(3))
    tflops = flops_per_cmux(P2) * P2["n"] * B2 / (ms * 1e-3) / 1e12
    # small batches (what one GPU gets of configs[3] / [4] over 8): two CUs per bootstrap (pbs_split_kernel, the default up to CUs / 2) against one CU per bootstrap
    from mosfhet_amd import engine
    small = {}
    for nb in (1, 128):
        sub = out2[:nb]
        two = min(eng.time_programmable_bootstrap(bsk2, d_tv2, d_ct2[:nb], 3, 3, out=sub) for _ in range(2))
        try:
            stats = engine.split_last_launch()
        except engine.MosfhetHipError:       # (the kernel is switched off: MOSFHET_HIP_SPLIT_MAX=0)
            stats = (nb, 0, 0)
        ph_s = host.tlwe_phase(ma.to_numpy(sub), rk2.extracted_lwe_key().s)
        err_s = np.abs((ph_s - lut[np.arange(nb) % 4]).astype(np.int64).astype(np.float64)).max()
        engine.set_split_max_batch(0)
        one = min(eng.time_programmable_bootstrap(bsk2, d_tv2, d_ct2[:nb], 3, 3, out=sub) for _ in range(2))
        engine.set_split_max_batch(-1)
        small["batch_%d" % nb] = {"ms_two_cus_per_bootstrap": two, "ms_one_cu_per_bootstrap": one, "taken_by_a_pair_of_workgroups": stats[1], "taken_alone": stats[2],
                                  "max_phase_error_log2": float(np.log2(err_s + 1)), "decrypts": bool(err_s < 2.0 ** 58)}
    res = {"workload": "batch of %d programmable bootstraps, TFHEpp lvl2 n=632 N=2048 k=1 l=4 Bg=2^9 (BASELINE.json configs[2])" % B2,
           "bootstraps_per_s": B2 / (ms * 1e-3), "ms_per_batch": ms, "kernel": "mosfhet::pbs_kernel<mosfhet::Fft2048T<false, false>, 4, 9>",
           "launches_per_batch": (B2 + 1023) // 1024, "bound": "fp64_valu", "achieved": tflops, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
           "frac": tflops / FP64_VECTOR_PEAK_TFLOPS, "max_phase_error_log2": float(np.log2(err + 1)), "decrypts": bool(err < 2.0 ** 58),
           "small_batches": small}
    return res


U64_ADD_PEAK_TOPS = 1024 * 64 / 4 * 2.4e9 / 1e12   # table key switches (word-lane form): one v_lshl_add_u64 (64 lanes) per SIMD per 4 clocks, 1024 SIMDs, 2.4 GHz = 39.3 T adds/s


def composition_legs(eng, ma, host, torch, keys, batch=1024, share=8, rank=0, world=1, dist_device=None):
    """BASELINE.json configs[3] and [4] on this GPU, `batch` inputs each and -- beside it -- ONE GPU's share when the configs' batches are split over `share` GPUs:
      circuit_bootstrap_3 (src/bootstrap.c:346-366: one bootstrap, l extractions, packing + private key switch per level; packing key t = 6, bb = 4, private key t = 20,
      bb = 2), full_domain_functional_bootstrap (:519-538, precision 3), multivalue_bootstrap_CLOT21 (:222-230, torus_base 2, 8 LUTs) and functional_bootstrap_ga
      (src/bootstrap_ga.c:62-76).  All keys but the private key-switch pair are generated on the device.  Every leg is checked by PHASE (no oracle on the measured path);
      each carries the share of the chip's FP64 vector peak its blind rotations reach (SURVEY 8(d) FLOP model over the composition's whole time -- the key switches,
      extractions and copies count as time, not as work) and, for the circuit bootstrap, its packing switches alone against the 64-bit-add issue rate that bounds them.
    world > 1 (every rank calls this): the configs' own shape -- the batch of 1024 SPLIT over the GPUs (strong scaling): rank r bootstraps the contiguous slice
      shard_bounds(batch, r, world) against its own replica of the keys (same seeds), no collective on the data path; a leg's time is the max over ranks of a
      barrier-bracketed region (mosfhet_amd/shard.py), its rate batch / that time; every rank phase-checks its own slice and the worst error is reported."""
    from mosfhet_amd import shard, engine
    P2, lk2, rk2, bsk = keys
    N, l, Bg, n = P2["N"], P2["l"], P2["Bg_bit"], P2["n"]
    s, out_s = rk2.s[0], rk2.extracted_lwe_key().s
    flops_rot = flops_per_cmux(P2) * n
    res = {}

    def phase_err(got, want):
        return float(np.abs((got - want).astype(np.int64).astype(np.float64)).max())

    lo, hi = shard.shard_bounds(batch, rank, world)
    mine = hi - lo                       # this rank's inputs (all of them at world = 1)

    def entry(name, workload, ref, units, run, check, rotations, small_run, extra=None, split_applies=True):
        run()
        torch.cuda.synchronize()
        err = check()
        if world > 1:
            import torch.distributed as dist
            reps = 3
            ms = 1e3 * shard.timed_region(run, reps, sync=torch.cuda.synchronize, device=dist_device) / reps
            e = torch.tensor([float(np.log2(err + 1))], dtype=torch.float64, device=dist_device)
            dist.all_reduce(e, op=dist.ReduceOp.MAX)
            tflops = rotations * flops_rot * units / (ms * 1e-3) / 1e12
            res[name] = {"workload": workload + " -- split over %d GPUs, %d - %d inputs each" % (world, batch // world, -(-batch // world)), "reference": ref, "units": units,
                         "n_gpus": world, "scaling": "strong", "ms_per_batch": ms, "units_per_s": units / (ms * 1e-3), "max_phase_error_log2": float(e.item()),
                         "decrypts": bool(e.item() < 60.0),
                         "roofline": {"bound": "fp64_valu", "achieved": tflops, "peak": world * FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                                      "frac": tflops / (world * FP64_VECTOR_PEAK_TFLOPS), "blind_rotations_per_unit": rotations,
                                      "note": "blind-rotation FLOP (SURVEY 8(d)) of the whole batch over the max-over-ranks time, against the %d GPUs' peak" % world}}
            return
        ms = timed_ms(torch, run)
        small_run()
        torch.cuda.synchronize()
        err_small = check()                # the share's outputs (the first `small` of the buffer) come from the kernels a batch of that size takes: checked like the full batch
        try:
            split = engine.split_last_launch() if split_applies else None
        except engine.MosfhetHipError:
            split = None
        ms_small = timed_ms(torch, small_run)
        tflops = rotations * flops_rot * units / (ms * 1e-3) / 1e12
        res[name] = {"workload": workload, "reference": ref, "units": units, "ms_per_batch": ms, "units_per_s": units / (ms * 1e-3),
                     "max_phase_error_log2": float(np.log2(err + 1)), "decrypts": bool(err < 2.0 ** 60),
                     "roofline": {"bound": "fp64_valu", "achieved": tflops, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tflops / FP64_VECTOR_PEAK_TFLOPS,
                                  "blind_rotations_per_unit": rotations, "note": "blind-rotation FLOP (SURVEY 8(d)) over the WHOLE composition's time"},
                     "share_of_%d" % share: {"units": units // share, "ms_per_batch": ms_small, "units_per_s": (units // share) / (ms_small * 1e-3),
                                             "max_phase_error_log2": float(np.log2(err_small + 1)), "decrypts": bool(err_small < 2.0 ** 60),
                                             "single_gpu_time_ratio_full_over_share": ms / ms_small,
                                             "blind_rotation_kernel": ("mosfhet::pbs_split_kernel / pbs_ga_split_kernel (two CUs per bootstrap, one 16 KiB exchange per CMUX step -- two for the Galois form; sums per accumulator "
                                                                       "component: FFT-level different bits from the full batch's kernel, bit-identical to the oracle in that order)"
                                                                       if split else "the kernels of the full batch"),
                                             "last_split_launch": ({"bootstraps": split[0], "by_a_pair_of_workgroups": split[1], "alone": split[2]} if split else None),
                                             "note": "ONE GPU's share when the config's batch of %d is sharded over %d GPUs, timed on this GPU alone (no other rank involved)" % (units, share)}}
        if extra:
            res[name].update(extra)

    small = max(1, mine // share)
    # ---- configs[3]: circuit_bootstrap_3 ----
    kska = eng.load_trlwe_ks_keys(host.gen_priv_ks_key(rk2, rk2, 20, 2), 2)
    pk = eng.generate_table_key(0, s, s, 6, 4, P2["rlwe_sigma"], seed=99)   # 6 GB of rows, all of them in HBM (seed-compressed keys -- 3 GB, masks regenerated in the kernel -- switch 25 % slower)
    d_cb_in = ma.to_device(host.tlwe_samples([host.double2torus(0.25 * (b & 1)) for b in range(lo, hi)], lk2), eng.device)
    d_cb_out = eng.empty(mine, 2 * l, 2, N)
    pick = np.unique(np.concatenate([[0, 1, mine // 2, mine - 1], np.random.default_rng(3).integers(0, mine, 12)]))

    def chk_cb():   # row l + i of TRGSW(bit): phase = bit 2^(64 - (i+1) Bg) on X^0 (test/tests.c:999-1003); a sample of the outputs, every coefficient of their b rows
        rows = ma.to_numpy(d_cb_out[pick][:, l:]).reshape(-1, 2, N)
        ph = trlwe_phase(rows, s).reshape(len(pick), l, N)
        want = np.zeros_like(ph)
        for i in range(l):
            want[:, i, 0] = ((pick + lo) & 1).astype(np.uint64) << np.uint64(64 - (i + 1) * Bg)
        return phase_err(ph, want)
    # the packing switches of one batch alone (l switches of `batch` extracted samples), against the issue rate of their 64-bit adds
    d_ext = ma.to_device(np.random.default_rng(4).integers(0, 2 ** 64, size=(mine, N + 1), dtype=np.uint64), eng.device)
    d_pk_out = eng.empty(mine, 2, N)
    eng.trlwe_packing1_keyswitch(pk, d_ext, out=d_pk_out)
    pk_ms = timed_ms(torch, lambda: eng.trlwe_packing1_keyswitch(pk, d_ext, out=d_pk_out))
    pk_adds = mine * N * 6 * (2 * N)
    entry("circuit_bootstrap_3", "%d x circuit_bootstrap_3 at N=2048 l=4 n=632, packing key t=6 bb=4 (6 GB of rows), private key t=20 bb=2 "
          "(BASELINE.json configs[3])" % batch, "/root/reference/src/bootstrap.c:346-366", batch,
          lambda: eng.circuit_bootstrap_3(bsk, kska, pk, d_cb_in, out=d_cb_out), chk_cb, 1,
          lambda: eng.circuit_bootstrap_3(bsk, kska, pk, d_cb_in[:small], out=d_cb_out[:small]),
          {"packing_switch": {"bound": "valu_issue", "kernel": "mosfhet::table_ks_words_kernel<15, false> (TRLWE rows; output words on the lanes)", "kernel_ms": pk_ms,
                              "switches_per_launch": mine, "launches_per_batch": l, "adds_per_launch": pk_adds,
                              "achieved": pk_adds / (pk_ms * 1e-3) / 1e12, "peak": U64_ADD_PEAK_TOPS, "unit": "T adds/s", "frac": pk_adds / (pk_ms * 1e-3) / 1e12 / U64_ADD_PEAK_TOPS,
                              "note": "one 64-bit add per (ciphertext, input word, digit position, output word) = src/keyswitch.c:470-473's subtraction; peak = one v_lshl_add_u64 per "
                                      "SIMD and 4 clocks on 1024 SIMDs at 2.4 GHz.  The ciphertext-lane form it replaces (keyswitch_kernels.h) was bound by its per-lane LDS gather",
                              "share_of_batch_time": None}})
    if world == 1:
        res["circuit_bootstrap_3"]["packing_switch"]["share_of_batch_time"] = l * pk_ms / res["circuit_bootstrap_3"]["ms_per_batch"]
    pk.free()
    kska.free()
    del d_cb_out, d_pk_out

    # ---- configs[4]: full-domain functional bootstrap, multi-value bootstrap ----
    ksk = eng.generate_keyswitch_key(lk2.s, out_s, P2["t"], P2["base_bit"], P2["lwe_sigma"], seed=7)
    lut8 = np.array([host.double2torus(((3 * i + 1) % 8) / 8.0) for i in range(8)], dtype=np.uint64)
    d_tv8 = ma.to_device(host.torus_packing_many_lut(lut8, 1, N, 4, 2)[None], eng.device)
    d_in5 = ma.to_device(host.tlwe_samples([(b % 8) << 61 for b in range(lo, hi)], lk2), eng.device)
    d_o5 = eng.empty(mine, N + 1)
    entry("full_domain_functional_bootstrap", "%d x full_domain_functional_bootstrap, precision 3, N=2048 l=4 n=632, key switch t=%d bb=%d (BASELINE.json configs[4])" % (batch, P2["t"], P2["base_bit"]),
          "/root/reference/src/bootstrap.c:519-538", batch, lambda: eng.full_domain_functional_bootstrap(bsk, ksk, d_tv8, d_in5, 3, out=d_o5),
          lambda: phase_err(host.tlwe_phase(ma.to_numpy(d_o5), out_s), lut8[np.arange(lo, hi) % 8]), 2,
          lambda: eng.full_domain_functional_bootstrap(bsk, ksk, d_tv8, d_in5[:small], 3, out=d_o5[:small]))
    ksk.free()
    lut16 = np.array([host.double2torus(((5 * i + 3) % 16) / 16.0) for i in range(16)], dtype=np.uint64)
    d_tvm = ma.to_device(host.torus_packing(lut16, 1, N)[None], eng.device)
    d_inm = ma.to_device(host.tlwe_samples([host.double2torus((b % 2) / 4.0) for b in range(lo, hi)], lk2), eng.device)
    d_om = eng.empty(mine, 8, N + 1)

    def chk_mv():   # selector m / 4 (m = b % 2), torus_base 2, 8 LUTs: output i is slot 8 m + i of the packed vector (test/tests.c:931-963)
        ph = host.tlwe_phase(ma.to_numpy(d_om).reshape(-1, N + 1), out_s).reshape(mine, 8)
        want = lut16[(8 * (np.arange(lo, hi) % 2))[:, None] + np.arange(8)[None, :]]
        return phase_err(ph, want)
    entry("multivalue_bootstrap_CLOT21", "%d x multivalue_bootstrap_CLOT21, torus_base 2, 8 LUTs per blind rotation, N=2048 l=4 n=632 (BASELINE.json configs[4])" % batch,
          "/root/reference/src/bootstrap.c:222-230", batch, lambda: eng.multivalue_bootstrap_CLOT21(bsk, d_tvm, d_inm, 2, 8, out=d_om), chk_mv, 1,
          lambda: eng.multivalue_bootstrap_CLOT21(bsk, d_tvm, d_inm[:small], 2, 8, out=d_om[:small]))

    # ---- configs[4]: Galois-automorphism bootstrap (its own bootstrap key TRGSW(X^s_i) and the N automorphism keys, both generated on the device) ----
    bk_ga = eng.generate_bootstrap_key(s, lk2.s, l, Bg, P2["rlwe_sigma"], seed=SEED + 9, ga=True)
    gak = eng.generate_trlwe_ks_keys(s, host.automorphism_key_sources(s), l, Bg, P2["rlwe_sigma"], seed=SEED + 10)
    lut4 = np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64)
    d_tv4 = ma.to_device(host.torus_packing(lut4, 1, N)[None], eng.device)
    d_inga = ma.to_device(host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(lo, hi)], lk2), eng.device)
    d_oga = eng.empty(mine, N + 1)
    entry("functional_bootstrap_ga", "%d x functional_bootstrap_ga (Galois-automorphism blind rotation), N=2048 l=4 n=632, 2048 automorphism keys (256 MiB) "
          "(BASELINE.json configs[4])" % batch, "/root/reference/src/bootstrap_ga.c:62-76", batch,
          lambda: eng.functional_bootstrap_ga(bk_ga, gak, d_tv4, d_inga, 4, out=d_oga),
          lambda: phase_err(host.tlwe_phase(ma.to_numpy(d_oga), out_s), lut4[np.arange(lo, hi) % 4]), flops_per_ga_step(P2) / flops_per_cmux(P2),
          lambda: eng.functional_bootstrap_ga(bk_ga, gak, d_tv4, d_inga[:small], 4, out=d_oga[:small]),
          {"flop_model": "per step: the external product (SURVEY 8(d): %d FLOP) + the automorphism key switch on component a (l forward and k + 1 inverse transforms, "
                         "8 l (k + 1) M for the products: %d FLOP) = %.3f plain steps; src/bootstrap_ga.c:39-60, src/keyswitch.c:162-193" % (
                             flops_per_cmux(P2), flops_per_ga_step(P2) - flops_per_cmux(P2), flops_per_ga_step(P2) / flops_per_cmux(P2))})
    bk_ga.free()
    gak.free()
    return res


def ffnt_single_ms(P, bk, tv, ct):
    """BASELINE.json configs[0]: ONE programmable bootstrap through the reference's portable FFNT pure-C build (plumbing, no GPU)."""
    from oracle import reflib
    if not reflib.available("ffnt"):
        return None
    ref = reflib.get("ffnt")
    ref.init(P["N"])
    h = ref.bk_new(bk, P["k"], P["l"], P["Bg_bit"])
    ref.bench_programmable_bootstrap(tv, ct, h, 3, 1)
    ms = 1e3 * ref.bench_programmable_bootstrap(tv, ct, h, 3, 5) / 5
    ref.bk_free(h)
    return ms


def cpu_baseline(P, bk, tv, cts, target_seconds):
    """Time the reference's programmable_bootstrap on the host cores (checker infrastructure, oracle/)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import reflib
    threads = usable_cores()
    backend = "avx512" if reflib.available("avx512") else ("ffnt" if reflib.available("ffnt") else None)
    if backend is None:
        # no reference build shipped: fall back to timing the oracle port on one core
        from oracle import oracle as O
        bk_dft = O.bk_to_dft(bk, P["k"], P["l"])
        t0 = time.time()
        reps = 0
        while time.time() - t0 < target_seconds / 2:
            O.programmable_bootstrap(tv, cts[reps % len(cts)], bk_dft, P["l"], P["Bg_bit"], 3, 0, 0)
            reps += 1
        dt = time.time() - t0
        return dict(value=reps / dt, unit="bootstraps/s", cores=1, kind="port",
                    sample="%d programmable_bootstrap calls of the C oracle, 1 thread, %.1f s" % (reps, dt))
    ref = reflib.get(backend)
    ref.init(P["N"])
    h = ref.bk_new(bk, P["k"], P["l"], P["Bg_bit"])
    # every usable core loops over small chunks of calls until a common deadline: bounded wall time whatever
    # the core count (ctypes releases the GIL; the reference's FFT state is per thread, src/polynomial.c:338-349)
    t1 = ref.bench_programmable_bootstrap(tv, cts[0], h, 3, 2) / 2
    chunk = max(1, int(0.25 / max(t1, 1e-4)))
    counts = [0] * threads
    t0 = time.time()
    deadline = t0 + target_seconds

    def worker(i):
        while time.time() < deadline:
            ref.bench_programmable_bootstrap(tv, cts[i % len(cts)], h, 3, chunk)
            counts[i] += chunk

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(worker, range(threads)))
    dt = time.time() - t0
    ref.bk_free(h)
    total = sum(counts)
    return dict(value=total / dt, unit="bootstraps/s", cores=threads, kind="reference",
                sample="%d programmable_bootstrap calls of MOSFHET (%s build of /root/reference) over %d threads in "
                       "%.1f s wall; one call alone takes %.2f ms" % (total, backend, threads, dt, 1e3 * t1))


def trlwe_phase(ct, s):
    """b - a * s of TRLWE samples [B][2][N] under a binary key s (negacyclic product as a sum of signed rotations; checker for the external-product
    legs: BK_i = TRGSW(s_i), so phase(BK_i (.) c) = s_i * phase(c) + noise, test_trgsw_trlwe_mul's property, test/tests.c:400-436)"""
    a, b = ct[:, 0], ct[:, 1]
    N = a.shape[1]
    acc = np.zeros_like(a)
    for p_ in np.nonzero(s)[0]:
        rot = np.roll(a, int(p_), axis=1)
        rot[:, :p_] = np.uint64(0) - rot[:, :p_]
        acc += rot
    return b - acc


def external_product_leg(eng, ma, host, P, B_ep, measured_traffic, traffic_file, kernel_name, torch):
    """The external-product kernel on its own (BASELINE.json's HBM target): B_ep TRLWE samples against ONE key entry, inputs and outputs in HBM.
    Timed with events on the launch stream; a sample of the outputs is checked by phase (no oracle in the measured path)."""
    N_, l_ = P["N"], P["l"]
    host.seed(SEED + 77)
    lk4 = host.LweKey(4, P["lwe_sigma"])
    rk4 = host.RlweKey(N_, P["k"], P["rlwe_sigma"])
    bsk4 = eng.load_bootstrap_key(host.gen_bootstrap_key(rk4, lk4, l_, P["Bg_bit"]), P["k"], l_, P["Bg_bit"])
    g = torch.Generator(device="cpu").manual_seed(SEED)
    d_ep_in = torch.randint(-2 ** 63, 2 ** 63 - 1, (B_ep, 2, N_), dtype=torch.int64, generator=g).to(eng.device)
    d_ep_out = eng.empty(B_ep, 2, N_)
    key_index = int(np.nonzero(lk4.s)[0][0]) if lk4.s.any() else 0       # an entry that encrypts 1: the product has to reproduce the phase
    eng.external_product(bsk4, key_index, d_ep_in, out=d_ep_out)
    torch.cuda.synchronize()
    pick = np.unique(np.concatenate([[0, 1, B_ep // 2, B_ep - 1], np.random.default_rng(5).integers(0, B_ep, 12)]))
    want = trlwe_phase(ma.to_numpy(d_ep_in[pick]), rk4.s[0]) * lk4.s[key_index]
    got = trlwe_phase(ma.to_numpy(d_ep_out[pick]), rk4.s[0])
    ep_err = np.abs((got - want).astype(np.int64).astype(np.float64)).max()
    if not ep_err < 2.0 ** 54:          # the reference's tolerance for this product (test/tests.c:424)
        sys.exit("bench.py: external-product outputs are wrong (max phase error 2^%.1f)" % np.log2(ep_err + 1))
    for _ in range(100):    # this kernel's own steady state: the clock the chip holds depends on the load of the last tenths of a second
        eng.external_product(bsk4, key_index, d_ep_in, out=d_ep_out)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps, groups = 20, []
    for _ in range(5):      # five groups of 20 back-to-back launches; the MEDIAN group is reported (min and max beside it)
        ev[0].record(torch.cuda.current_stream())      # the engine launches on torch's current stream (mosfhet_amd/engine.py: _stream)
        for _ in range(reps):
            eng.external_product(bsk4, key_index, d_ep_in, out=d_ep_out)
        ev[1].record(torch.cuda.current_stream())
        ev[1].synchronize()
        groups.append(ev[0].elapsed_time(ev[1]) / reps)
    groups.sort()
    ep_ms = groups[len(groups) // 2]
    ep_bytes = B_ep * 2 * (2 * N_ * 8) + (2 * l_) * 2 * N_ * 8        # TRLWE in + TRLWE out per unit, the key entry once
    ep_gbs = ep_bytes / (ep_ms * 1e-3) / 1e9
    flops = flops_per_cmux(P) * B_ep
    bsk4.free()
    traffic = measured_traffic(traffic_file, B_ep)
    return {"bound": "hbm", "achieved": ep_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ep_gbs / HBM_PEAK_GBS, "traffic": traffic,
            "traffic_source": ("profiles/%s: rocprofv3 PMC passes of this very build (source hash matched), taken once and committed -- not measured in this run" % traffic_file
                               if traffic is not None else None),
            "kernel": kernel_name, "kernel_ms": ep_ms, "kernel_ms_min_max": [groups[0], groups[-1]], "units_per_launch": B_ep,
            "algorithmic_bytes_per_launch": ep_bytes, "external_products_per_s": B_ep / (ep_ms * 1e-3),
            "fp64_model_tflops": flops / (ep_ms * 1e-3) / 1e12, "fp64_frac": flops / (ep_ms * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
            "max_phase_error_log2": float(np.log2(ep_err + 1)),
            "workload": "%d x trgsw_mul_trlwe_DFT + trlwe_from_DFT at N=%d l=%d against one TRGSW_DFT (src/trgsw.c:385-423)" % (B_ep, N_, l_)}


def gate_leg(eng, ma, host, torch, P, lk, rk, bsk, B=4096):
    """The reference's canonical gate at SET_1: tlwe_keyswitch from the extracted key (dimension kN) back to n (src/tlwe.c:289-303), then
    functional_bootstrap (src/bootstrap.c:200-206) -- one call, two launches (mosfhet_hip_keyswitch_functional_bootstrap_batch); B inputs resident, outputs checked by phase."""
    out_key = rk.extracted_lwe_key()
    ksk = eng.generate_keyswitch_key(lk.s, out_key.s, P["t"], P["base_bit"], P["lwe_sigma"], seed=21)
    lut = np.array([host.double2torus(x) for x in (0.0625, 0.3125, -0.1875, 0.4375)], dtype=np.uint64)
    d_tv = ma.to_device(host.torus_packing(lut, P["k"], P["N"])[None], eng.device)
    d_in = ma.to_device(host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(B)], out_key), eng.device)
    d_out = eng.empty(B, P["k"] * P["N"] + 1)
    d_ks = eng.empty(B, P["n"] + 1)
    run = lambda: eng.keyswitch_functional_bootstrap(ksk, bsk, d_tv, d_in, 4, out=d_out)
    run()
    torch.cuda.synchronize()
    ph = host.tlwe_phase(ma.to_numpy(d_out), out_key.s)
    err = float(np.abs((ph - lut[np.arange(B) % 4]).astype(np.int64).astype(np.float64)).max())
    ms = timed_ms(torch, run, reps=5)
    ks_ms = timed_ms(torch, lambda: eng.tlwe_keyswitch(ksk, d_in, out=d_ks), reps=5)
    tflops = flops_per_cmux(P) * P["n"] * B / (ms * 1e-3) / 1e12
    ksk.free()
    return {"workload": "%d x (tlwe_keyswitch N=%d -> n=%d, t=%d base 2^%d; functional_bootstrap) at SET_1" % (B, P["N"], P["n"], P["t"], P["base_bit"]),
            "reference": "/root/reference/src/tlwe.c:289-303, src/bootstrap.c:200-206", "units": B, "ms_per_batch": ms, "gates_per_s": B / (ms * 1e-3),
            "keyswitch_ms": ks_ms, "keyswitch_share_of_time": ks_ms / ms, "max_phase_error_log2": float(np.log2(err + 1)), "decrypts": bool(err < 2.0 ** 60),
            "roofline": {"bound": "fp64_valu", "achieved": tflops, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tflops / FP64_VECTOR_PEAK_TFLOPS,
                         "note": "blind-rotation FLOP (SURVEY 8(d)) over the whole gate's time: the key switch counts as time, not as work"}}


def vector_callers_leg(eng, ma, host, torch, M=256):
    """the radix-integer callers of applications/multi-ciphertext-arith (src/integer.c:62-107, src/ml.c:4-20, src/lut.c:49-64) over M independent signed 8-bit
    integers at the application's own parameter set (src/ufhe.c:18-20: n = 630, N = 2048, l = 6, Bg = 2^7, key switch t = 6 base 2^2, radix 4), digit-parallel: one call each
    of add, ReLU and a 16-entry encrypted look-up (mosfhet_hip_vec_addsub / _relu / _mux_array).  Every result is decrypted and compared with the arithmetic."""
    n, N, l, Bg, t, bb, Bt, d = 630, 2048, 6, 7, 6, 2, 4, 4
    host.seed(SEED + 30)
    lk = host.LweKey(n, 3.0517578125e-05)
    rk = host.RlweKey(N, 1, 5.684341886080802e-14)
    ex = rk.extracted_lwe_key()
    bsk = eng.generate_bootstrap_key(rk.s[0], lk.s, l, Bg, 5.684341886080802e-14, seed=31)
    ksk = eng.generate_keyswitch_key(lk.s, ex.s, t, bb, 3.0517578125e-05, seed=32)
    pksk = eng.generate_lut_packing_key(rk.s[0], ex.s, t, bb, Bt, 5.684341886080802e-14, seed=33)
    vec = eng.vector_ops(bsk, ksk, pksk, Bt)
    rng = np.random.default_rng(0xD163)
    a, b, sel = rng.integers(-128, 128, M), rng.integers(-128, 128, M), rng.integers(0, 16, M)
    table = rng.integers(-128, 128, (M, 16))

    def encrypt(values, digits):   # ufhe_encrypt_integer (src/integer.c:34-40), digit-major [digits][M][N+1]
        v = np.asarray(values).astype(np.int64) & 0xff
        msgs = [host.double2torus(float((int(x) >> (2 * i)) & 3) / (2 * Bt)) for i in range(digits) for x in v]
        return ma.to_device(host.tlwe_samples(msgs, ex).reshape(digits, len(v), N + 1), eng.device)

    def decrypt(ct):               # ufhe_decrypt_integer (:50-59), signed 8 bit
        x = ma.to_numpy(ct)
        digits, m, _ = x.shape
        ph = host.tlwe_phase(x.reshape(-1, N + 1), ex.s).reshape(digits, m)
        dig = np.round(ph.astype(np.float64) / 2.0 ** 64 * (2 * Bt)).astype(np.int64) % Bt
        return (sum(dig[i] << (2 * i) for i in range(digits)) + 128) % 256 - 128

    da, db, dsel = encrypt(a, d), encrypt(b, d), encrypt(sel, 2)
    dtab = torch.stack([encrypt(table[:, j], d) for j in range(16)]).contiguous()
    wrap = lambda x: (np.asarray(x) + 128) % 256 - 128
    c_add, c_relu, c_lut = vec.addsub(da, db), vec.relu(da), vec.mux_array(dtab.clone(), dsel)
    torch.cuda.synchronize()
    ok = bool((decrypt(c_add) == wrap(a + b)).all() and (decrypt(c_relu) == np.where(a > 0, a, 0)).all() and (decrypt(c_lut) == table[np.arange(M), sel]).all())
    tabs = [dtab.clone() for _ in range(3)]      # (the look-up consumes its table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(3):
        vec.addsub(da, db)
        vec.relu(da)
        vec.mux_array(tabs[k], dsel)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / 3
    vec.free(); pksk.free(); ksk.free(); bsk.free()
    return {"workload": "%d signed 8-bit radix-4 integers through add + ReLU + 16-entry encrypted look-up, one call each (n=630 N=2048 l=6 Bg=2^7)" % M,
            "reference": "/root/reference/applications/multi-ciphertext-arith/src/integer.c:62-107, src/ml.c:4-20, src/lut.c:49-64", "units": M, "ms_per_call_sequence": ms,
            "integers_per_s": M / (ms * 1e-3), "decrypts_to_the_arithmetic": ok}


def usable_cores():
    """Cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


DUMP_NAME = "programmable_bootstrap_out"
DUMP_BUDGET_BYTES = 60 * 10 ** 6     # all ranks' files together (the limit is 64 MB)


def dump_outputs(out_dir, out, rank, world):
    """--dump-outputs: the LWE samples [B][kN + 1] the timed path returned in its last step, as float64 torus values in [-1/2, 1/2) (signed 64-bit word / 2^64:
    the top 53 bits of every word, the message and its noise included).  Rank r > 0 writes <name>_rank<r>.npy.  When all ranks' rows exceed the budget, a fixed
    seeded sample of rows is written, in order, and its row indices beside it (<name>_rows.npy)."""
    B, width = out.shape
    rows = min(B, DUMP_BUDGET_BYTES // (world * width * 8))
    pick = np.sort(np.random.default_rng(SEED).choice(B, rows, replace=False)) if rows < B else None
    words = out if pick is None else out[pick]
    suffix = "" if rank == 0 else "_rank%d" % rank
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, DUMP_NAME + suffix + ".npy"), words.view(np.int64).astype(np.float64) * 2.0 ** -64)
    if pick is not None:
        np.save(os.path.join(out_dir, DUMP_NAME + "_rows" + suffix + ".npy"), pick.astype(np.float64))


def launch_ranks(n_gpus):
    """One rank per GPU under torch.distributed.run on this node (127.0.0.1, a free port), started as a child process with this script's own arguments.
    The child's stdout / stderr are inherited, so rank 0's JSON line is this command's JSON line; returns the child's exit code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this pool's host driver
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096, help="bootstraps per GPU per step")
    ap.add_argument("--streams", type=int, default=2, help="HIP streams the steps alternate over (1 = strictly back to back)")
    ap.add_argument("--ep-batch", type=int, default=65536, help="TRLWE samples of the external-product roofline line")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="wall budget of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-lvl2", action="store_true", help="skip the configs[2] leg (4096 lvl2 bootstraps, ~2 s) and with it configs[3] / [4]")
    ap.add_argument("--no-callers", action="store_true", help="skip the gate leg (4096 x key switch + bootstrap at SET_1) and the vector_callers leg (256 radix integers: add + ReLU + LUT; ~6 s with its keys)")
    ap.add_argument("--no-configs34", action="store_true", help="skip the configs[3] / [4] legs (circuit bootstrap, FDFB, multi-value, Galois bootstrap: ~10 s; N > 1: the batches split over the ranks)")
    ap.add_argument("--full", action="store_true", help="besides the headline figure, run every other leg of the line (decrypt check, roofline, external-product, "
                                                       "lvl2 and configs[3] / [4] legs, gate, vector callers, latency, sustained rate, host buffers, replicas, CPU baseline); "
                                                       "the --no-* options above apply to it")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the bootstrap outputs of the last timed step to DIR/%s.npy" % DUMP_NAME)
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves, as a CHILD torch.distributed.run, before this process has imported torch or
        # touched a GPU (never exec: see the GPU pool's rule); relay the ranks' output -- rank 0's one JSON line -- and leave with the child's code
        sys.exit(launch_ranks(args.gpus))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py --gpus %d inside a launcher with WORLD_SIZE=%d: the two must agree" % (args.gpus, world))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: mosfhet_amd has no CPU path")
    # Test hooks for the N > 1 path on a box with fewer GPUs than ranks (tests/test_gpu_parity.py::test_bench_two_ranks_on_one_gpu): every rank on
    # device 0 and gloo for the barrier / max-reduction.  The driver never sets them: one rank per GPU over RCCL ("nccl").
    share_gpu = os.environ.get("MOSFHET_BENCH_SHARE_GPU", "0") == "1"
    backend = os.environ.get("MOSFHET_BENCH_BACKEND", "nccl")
    dev_index = 0 if share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    # MOSFHET_BENCH_FORCE_DIST=1 (test hook): make the process group at world size 1 too, so that the RCCL branch -- communicator on this rank's device, the
    # barriers and the max-reduction of the timed region on a device tensor -- executes on a 1-GPU box exactly as the driver's N > 1 launches run it
    force_dist = os.environ.get("MOSFHET_BENCH_FORCE_DIST", "0") == "1" and "RANK" in os.environ
    if world > 1 or force_dist:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)

    import mosfhet_amd as ma
    from mosfhet_amd import host, build, shard
    build.build()
    P = dict(ma.PARAMS_SET1)
    B = args.batch

    # ---- synthetic keys and ciphertexts; same seed on every rank = replicated key
    host.seed(SEED)
    lk = host.LweKey(P["n"], P["lwe_sigma"])
    rk = host.RlweKey(P["N"], P["k"], P["rlwe_sigma"])
    bk = host.gen_bootstrap_key(rk, lk, P["l"], P["Bg_bit"])
    eng = ma.Engine(dev_index)
    bsk = eng.load_bootstrap_key(bk, P["k"], P["l"], P["Bg_bit"])
    host.seed(SEED + 1 + rank)  # different ciphertexts per rank
    lut = np.array([host.double2torus(x) for x in (0.0625, 0.3125, -0.1875, 0.4375)], dtype=np.uint64)
    tv = host.torus_packing(lut, P["k"], P["N"])
    msgs = [host.double2torus((b % 4) / 8.0) for b in range(B)]
    cts = host.tlwe_samples(msgs, lk)
    # --full: the CPU leg runs FIRST (rank 0, N = 1): the GPU legs then form one contiguous block at the end of the run
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(P, bk, tv, cts[:64], args.cpu_seconds)
        cpu["ffnt_single_ms"] = ffnt_single_ms(P, bk, tv, cts[0])      # BASELINE.json configs[0]
    elif args.full and world > 1 and not args.no_cpu_baseline:
        # N > 1: the same sample, shorter, on rank 0 while the other ranks sleep in a socket wait (a gloo side group: an RCCL barrier would keep one host
        # core per rank spinning under the CPU measurement) -- so that a SCALE line carries its own cpu_baseline
        side = dist.new_group(backend="gloo") if backend == "nccl" else None
        dist.barrier(group=side)
        if rank == 0:
            cpu = cpu_baseline(P, bk, tv, cts[:64], min(args.cpu_seconds, 8.0))
            cpu["sample"] += " (rank 0 of %d, the other ranks idle)" % world
        dist.barrier(group=side)
    d_tv = ma.to_device(tv[None], eng.device)
    d_ct = ma.to_device(cts, eng.device)
    d_out = eng.empty(B, P["k"] * P["N"] + 1)
    # Consecutive steps are independent batches: they alternate over `--streams` HIP streams (own output buffer each, the inputs are read-only), so
    # the tail of one launch -- CUs that have run out of work while the slowest teams finish -- is filled by the head of the next.
    streams = [torch.cuda.Stream(device=eng.device) for _ in range(max(1, args.streams))]
    d_outs = [d_out] + [eng.empty(B, P["k"] * P["N"] + 1) for _ in streams[1:]]
    turn = [0]

    def step():
        i = turn[0] % len(streams)
        turn[0] += 1
        with torch.cuda.stream(streams[i]):
            eng.programmable_bootstrap(bsk, d_tv, d_ct, 3, 0, 0, out=d_outs[i])

    step()
    torch.cuda.synchronize()

    # --full: correctness of what is being timed: every output must decrypt to its LUT slot.  The reference asserts 2^58 on a
    # single sample (test/tests.c:1560); over thousands of SET_1 samples the noise tail (sigma ~ 2^55.5) brushes that
    # bound, so the batch criterion is: all within 2^60 (no wrong slot: slots are >= 2^61 apart) and >= 99.5 % within 2^58.
    err = None
    if args.full:
        ph = host.tlwe_phase(ma.to_numpy(d_out), rk.extracted_lwe_key().s)
        dist_t = np.abs((ph - lut[np.arange(B) % 4]).astype(np.int64).astype(np.float64))
        err = dist_t.max()
        if not (err < 2.0 ** 60 and (dist_t < 2.0 ** 58).mean() >= 0.995):
            sys.exit("bench.py: bootstrap outputs do not decrypt (max phase error 2^%.1f)" % np.log2(err + 1))

    # W untimed warm-up steps directly before the timed region (the host-side decrypt check above idles the GPU)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    # timed region: barrier + synchronize on both sides, MAX over ranks (mosfhet_amd/shard.py)
    elapsed = shard.timed_region(step, args.steps, sync=torch.cuda.synchronize, device=eng.device if backend == "nccl" else "cpu")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, ma.to_numpy(d_outs[(turn[0] - 1) % len(streams)]), rank, world)

    line = {
        "metric": "programmable bootstraps/sec (whole node), N=1024 k=1",
        "value": world * args.steps * B / elapsed,
        "unit": "bootstraps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "value_regime": "%d HIP stream(s): consecutive steps are independent batches and %s" % (
            len(streams), "overlap at launch boundaries" if len(streams) > 1 else "run strictly back to back"),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "process_group": (backend if (world > 1 or force_dist) else None),
        "config": {"workload": "batch of %d programmable bootstraps per GPU, SET_1 n=585 N=1024 k=1 l=2 Bg=2^8 "
                               "(BASELINE.json configs[1])" % B,
                   "batch_per_gpu": B, "streams": len(streams), "parallelism": "batch sharded over %d GPU(s), bootstrap key replicated, "
                                                      "no collective on the data path" % world},
        "full": args.full,
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1 or force_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    # The dominant kernel, timed in the state the timed region left the chip in (round 3 timed it after the host-buffer leg and read 9 % above the
    # step it is the whole of): (a) alone -- launches back to back on ONE stream between two hipEvents, the launch duration the roofline is priced on;
    # (b) in the regime `value` was measured in -- the same alternating launches with an event pair around EACH launch on its own stream: a launch's
    # span there overlaps its neighbours' head and tail, so span - period is the overlap per step and  ms_per_step = span - overlap  can be checked
    # on the line itself.
    kernel_ms = eng.time_programmable_bootstrap(bsk, d_tv, d_ct, 3, max(3, min(args.steps, 10)), out=d_out)
    n_reg = max(4, min(args.steps, 20))
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_reg)]
    torch.cuda.synchronize()
    for i in range(n_reg):
        j = i % len(streams)
        with torch.cuda.stream(streams[j]):
            evs[i][0].record(streams[j])
            eng.programmable_bootstrap(bsk, d_tv, d_ct, 3, 0, 0, out=d_outs[j])
            evs[i][1].record(streams[j])
    torch.cuda.synchronize()
    spans = [a.elapsed_time(b) for a, b in evs]
    period = evs[0][0].elapsed_time(evs[-1][1]) / n_reg
    stream_regime = {"launches": n_reg, "launch_span_ms_mean": float(np.mean(spans)), "launch_span_ms_min_max": [float(min(spans)), float(max(spans))],
                     "period_ms": period, "overlap_ms_per_step": float(np.mean(spans)) - period,
                     "note": "hipEvents around every launch on its own stream while the %d streams alternate: period = span - overlap" % len(streams)}

    # N > 1: what makes the ranks replicas of one job -- the SAME bootstrap key on every GPU (same seed), DIFFERENT ciphertexts per rank, every rank's
    # outputs decrypting -- gathered once, outside the timed region
    replicas = None
    if world > 1 or force_dist:
        import zlib
        mine = torch.tensor([zlib.crc32(bk.tobytes()), zlib.crc32(cts.tobytes()), int(np.log2(err + 1) * 1000), int(kernel_ms * 1e6), int(period * 1e6)], dtype=torch.int64,
                            device=eng.device if backend == "nccl" else "cpu")
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        every = torch.stack(every).cpu().numpy()
        replicas = {"keys_identical": bool((every[:, 0] == every[0, 0]).all()), "inputs_distinct": len(set(every[:, 1].tolist())) == world,
                    "max_phase_error_log2_per_rank": (every[:, 2] / 1000.0).tolist(),
                    "kernel_ms_per_rank": (every[:, 3] / 1e6).tolist(), "period_ms_in_stream_regime_per_rank": (every[:, 4] / 1e6).tolist(),
                    "route": "one process per GPU: every rank builds the key from the same seed and uploads its own replica (host -> its device); nothing crosses between GPUs",
                    "key_bytes_per_gpu": int(bk.nbytes), "devices": [torch.cuda.get_device_name(dev_index)] if world == 1 else None}
        if rank == 0 and not (replicas["keys_identical"] and replicas["inputs_distinct"]):
            sys.exit("bench.py: the ranks are not replicas of one job: %s" % replicas)

    # the same step with the ciphertexts handed over in HOST buffers (pinned): H2D of the inputs + kernel + D2H of the results.  Reported
    # beside `value` for reference only (the contract's `value` has the inputs resident in HBM).
    h_in = torch.from_numpy(cts.view(np.int64)).pin_memory()
    h_out = torch.empty(B, P["k"] * P["N"] + 1, dtype=torch.int64).pin_memory()

    d_ct_h = torch.empty_like(d_ct)

    def step_host():   # one stream: copy in, bootstrap, copy out
        with torch.cuda.stream(streams[0]):
            d_ct_h.copy_(h_in, non_blocking=True)
            eng.programmable_bootstrap(bsk, d_tv, d_ct_h, 3, 0, 0, out=d_out)
            h_out.copy_(d_out, non_blocking=True)

    step_host()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        step_host()
    torch.cuda.synchronize()
    host_rate = 3 * B / (time.perf_counter() - t0)

    flops_per_launch = flops_per_cmux(P) * P["n"] * B
    achieved_tflops = flops_per_launch / (kernel_ms * 1e-3) / 1e12
    bytes_per_launch = algorithmic_bytes_per_bootstrap(P) * B

    def measured_traffic(name, units):
        """memory-side bytes per launch from the committed rocprofv3 PMC passes (tools/profile_r02.sh: FETCH_SIZE and WRITE_SIZE in separate
        passes, gfx950 correction applied by tools/make_traffic_json.py) -- only if they were taken from the library that is running now and at
        this launch size; otherwise null"""
        tfile = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(tfile):
            return None
        with open(tfile) as f:
            t = json.load(f)
        try:
            with open(build.STAMP) as f:
                srchash = f.read().strip()
        except OSError:
            return None
        if t.get("srchash") != srchash or t.get("units_per_launch", units) != units:
            return None
        return t.get("traffic_bytes_per_launch")

    traffic = measured_traffic("latest_traffic.json", 4096) if B == 4096 else None

    # the external-product kernel on its own (BASELINE.json's HBM target), at SET_1 and at the TFHEpp lvl2 set (N = 2048, l = 4: four of BASELINE's five
    # configs): arithmetic intensity 5.2 FLOP/B at SET_1, 9.8 at lvl2 = the FP64 ridge, where the instruction-mix ceiling of the transforms (DESIGN.md
    # 4.1) caps the HBM fraction near 0.45
    ep = ep2 = None
    if rank == 0:
        ep = external_product_leg(eng, ma, host, P, args.ep_batch, measured_traffic, "latest_traffic_ep.json",
                                  "mosfhet::external_product_ldskey_kernel<2, 8, false>", torch)
        ep2 = external_product_leg(eng, ma, host, dict(ma.PARAMS_LVL2), max(64, args.ep_batch // 4), measured_traffic, "latest_traffic_ep_lvl2.json",
                                   "mosfhet::external_product_kernel<mosfhet::Fft2048T<false, true>, 4, 9, false, 0>", torch)

    lvl2 = configs34 = None
    if not args.no_lvl2 and (rank == 0 or (world > 1 and not args.no_configs34)):
        keys2 = lvl2_keys(eng, ma, host)      # same seeds on every rank: replicas of one key set
        if rank == 0:
            lvl2 = lvl2_bootstrap_leg(eng, ma, host, torch, keys2)
        if not args.no_configs34:
            # N = 1: the whole batches on this GPU (+ one GPU's share of 8); N > 1: the batches split over the ranks, every rank takes part (barrier + max over ranks)
            configs34 = composition_legs(eng, ma, host, torch, keys2, rank=rank, world=world, dist_device=(eng.device if backend == "nccl" else "cpu"))
        keys2[3].free()

    gate = vectors = None
    if rank == 0 and not args.no_callers:
        gate = gate_leg(eng, ma, host, torch, P, lk, rk, bsk)
        vectors = vector_callers_leg(eng, ma, host, torch)

    # one bootstrap alone (the latency kernel: one workgroup of 2l wavefronts for the ciphertext), same key, same timing method as roofline.kernel_ms
    latency_ms = eng.time_programmable_bootstrap(bsk, d_tv, d_ct[:1], 3, 5, out=d_out[:1]) if rank == 0 else None

    # sustained rate: the same step back to back for >= 2.5 s (the contract's timed region is K steps = a fraction of a second; this is the figure a
    # long-running caller sees, and it keeps the GPU visibly busy for a utilisation sampler)
    sustained = None
    if world == 1:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_sus = 0
        while time.perf_counter() - t0 < 2.5:
            for _ in range(8):
                step()
            n_sus += 8
            torch.cuda.synchronize()
        sustained = {"bootstraps_per_s": n_sus * B / (time.perf_counter() - t0), "steps": n_sus, "seconds": time.perf_counter() - t0}

    if rank == 0:
        line["value_regime"] += ("; roofline.kernel_ms is the launch alone (one stream, timed right after the timed region), roofline.kernel_ms_in_stream_regime "
                                 "the same launches as they ran for `value`: ms_per_step = launch span - overlap")
        line.update({
            "roofline": {"bound": "fp64_valu", "achieved": achieved_tflops, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved_tflops / FP64_VECTOR_PEAK_TFLOPS, "traffic": traffic,
                         "traffic_source": ("profiles/latest_traffic.json: rocprofv3 PMC passes of this very build (source hash matched), taken once and committed -- not measured in this run"
                                            if traffic is not None else None),
                         "kernel": "mosfhet::pbs_kernel<mosfhet::Fft1024, 2, 8>", "kernel_ms": kernel_ms,
                         "kernel_ms_vs_ms_per_step": kernel_ms / (1e3 * elapsed / args.steps),
                         "kernel_ms_in_stream_regime": stream_regime,
                         "flops_per_launch": flops_per_launch, "flops_per_cmux": flops_per_cmux(P),
                         "hbm_algorithmic": {"bytes_per_launch": bytes_per_launch, "gb_per_s": bytes_per_launch / (kernel_ms * 1e-3) / 1e9,
                                             "note": "SURVEY 8(d) byte model (bootstrap key streamed once per ciphertext): not a bound, the "
                                                     "key is shared by the batch through L2 (see `traffic` for measured memory-side bytes)"}},
            "roofline_external_product": ep,
            "roofline_external_product_lvl2": ep2,
            "lvl2_bootstraps": lvl2,
            "configs_3_4": configs34,
            "gate": gate,
            "vector_callers": vectors,
            "sustained": sustained,
            "single_bootstrap_ms": latency_ms,
            "replicas": replicas,
            "cpu_baseline": cpu,
            "max_phase_error_log2": float(np.log2(err + 1)),
            "host_buffer_rate_per_gpu": host_rate,
        })
        print(json.dumps(line), flush=True)
    if world > 1 or force_dist:
        dist.barrier()                  # (rank 0 runs a few legs of its own after the last collective: the ranks leave together)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
