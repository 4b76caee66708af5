"""The client half on the device: time per call of Engine.trgsw_encrypt, Engine.trlwe_phase and Engine.tlwe_phase (mosfhet_hip_trgsw_encrypt_batch, _trlwe_phase_batch,
_tlwe_phase_batch) against the yardstick an older library has -- so the yardstick can be taken on a library built from the parent commit (--lib), where the new calls
are skipped.

    python tools/gpu_perf_client_samples.py [--lib PATH] [--repeats 7] [--samples 4096]

(a) trgsw_encrypt at (N, l, Bg_bit) = (2048, 4, 9), count 632, DFT output only, against mosfhet_hip_bsk_generate at n = 632 with the same gadget and TRLWE key: the same
    number of TRGSW samples made and transformed (5056 rows, 10112 transforms).  The yardstick's handle is freed outside the timed region.
(b) trlwe_phase and tlwe_phase of --samples samples at both parameter sets (SET_1: n 585, N 1024; lvl2: n 632, N 2048; binary keys of the tool's own making), next to
    two bounds computed here: the time the call's HBM traffic alone takes at 6.3 TB/s (what a streaming copy reaches on this part) and, for trlwe_phase, the time its LDS
    reads alone take -- N x (set positions) reads of 8 bytes per sample, as the kernel issues them: ds_read2st64_b64 at 128 bytes per clock and CU, 256 CUs at 2.4 GHz.
(c) generate_trlwe_ks_keys and generate_keyswitch_key at lvl2, the generators whose kernels host the client kinds as run-time kinds: on either library.
hipEvent time around one whole call after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: yardstick only)")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--samples", type=int, default=4096)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
have_new = hasattr(engine.lib(), "mosfhet_hip_trgsw_encrypt_batch")
HBM, LDS = 6.3e12, 128.0 * 256 * 2.4e9          # bytes per second: streaming HBM traffic; ds_read2st64_b64 on every CU


def timed(label, shape, run, after=None, note=""):
    run()
    torch.cuda.synchronize()
    if after:
        after()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        if after:
            after()
    ms.sort()
    med = ms[len(ms) // 2]
    print("%-22s %s ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats)%s" % (label, shape, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med,
                                                                                                    len(ms), note), flush=True)
    return med


rng = np.random.default_rng(7)
eng.set_keygen_secret(bytes(range(32)))

# (a)
N, l, Bg, n, sigma = 2048, 4, 9, 632, 2.0 ** -44
s_rlwe, s_lwe = rng.integers(0, 2, size=N).astype(np.uint64), rng.integers(0, 2, size=n).astype(np.uint64)
shape = "N=%d l=%d Bg=2^%d samples=%d" % (N, l, Bg, n)
held = []


def generate():
    held.append(eng.generate_bootstrap_key(s_rlwe, s_lwe, l, Bg, sigma, 0x5EED))


def release():
    while held:
        held.pop().free()


timed("yardstick bsk_generate", shape, generate, release)
if have_new:
    key = engine.client_key_create(s_rlwe=s_rlwe)
    m = torch.from_numpy(s_lwe.astype(np.int32)).to(eng.device)
    plan = engine.trgsw_encrypt_plan(N, l, n)
    timed("new trgsw_encrypt", shape, lambda: eng.trgsw_encrypt(key, m, l, Bg, sigma), note="  plan %s" % plan)
    timed("new trgsw_encrypt both", shape, lambda: eng.trgsw_encrypt(key, m, l, Bg, sigma, torus=True))
    timed("new trgsw rows only", shape, lambda: eng.trgsw_encrypt(key, m, l, Bg, sigma, torus=True, dft=False))
    key.close()

# (c) the two generators whose kernels host the client kinds (trlwe_poly_keygen_kernel, tlwe_ksk_keygen_kernel): the same calls on either library
msgs = rng.integers(0, 2 ** 64, size=(64, N), dtype=np.uint64)
timed("generate_trlwe_ks_keys", "N=%d entries=64 t=8 base_bit=4" % N, lambda: held.append(eng.generate_trlwe_ks_keys(s_rlwe, msgs, 8, 4, sigma, 0x5EED)), release)
timed("generate_keyswitch_key", "n_out=%d n_in=%d t=8 base_bit=4" % (n, N), lambda: held.append(eng.generate_keyswitch_key(s_lwe, s_rlwe, 8, 4, 2.0 ** -15, 0x5EED)), release)

# (b)
if have_new:
    count = args.samples
    for name, P in (("SET_1", ma.PARAMS_SET1), ("lvl2", ma.PARAMS_LVL2)):
        N, n = P["N"], P["n"]
        s_rlwe, s_lwe = rng.integers(0, 2, size=N).astype(np.uint64), rng.integers(0, 2, size=n).astype(np.uint64)
        key = engine.client_key_create(s_rlwe, s_lwe)
        gen = torch.Generator(device=eng.device).manual_seed(1)
        trlwe = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
        tlwe = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, n + 1), dtype=torch.int64, device=eng.device, generator=gen)
        out_r, out_t = eng.empty(count, N), eng.empty(count)
        hbm_r, hbm_t = count * 3 * N * 8 / HBM * 1e3, count * (n + 2) * 8 / HBM * 1e3
        lds_r = count * N * key.rlwe_weight * 8 / LDS * 1e3
        timed("new trlwe_phase", "%s N=%d weight=%d samples=%d" % (name, N, key.rlwe_weight, count), lambda: eng.trlwe_phase(key, trlwe, 0, out=out_r),
              note="  bounds: HBM traffic %.4f ms, LDS reads %.4f ms" % (hbm_r, lds_r))
        timed("new tlwe_phase", "%s n=%d samples=%d" % (name, n, count), lambda: eng.tlwe_phase(key, tlwe, 0, out=out_t), note="  bound: HBM traffic %.4f ms" % hbm_t)
        key.close()
