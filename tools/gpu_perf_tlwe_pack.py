"""LWE batches packed into TRLWE samples: time per call of Engine.tlwe_pack (mosfhet_hip_tlwe_pack_batch) against what the library could do before.

    python tools/gpu_perf_tlwe_pack.py [--modes new,loop,boot] [--shapes set1,lvl2] [--lib PATH] [--repeats 7]

--shapes:
    set1     4096 SET_1 results: N 1024, n_in 1024, t 6, base_bit 4, per 1024 (4 outputs)
    lvl2     1024 lvl2 results:  N 2048, n_in 2048, t 4, base_bit 6, per 1024 (1 output)
--modes, one after the other in one process:
    new      the call at split = 1, at the plan's split and at the splits around it; the outputs of the plan's split are decrypted (real keys: the packing key from
             mosfhet_hip_trlwe_ksk_generate, messages on multiples of 1/8) and the worst phase error is printed
    loop     yardstick (a), the same packing from entry points of the parent commit on device buffers: n_in calls of trlwe_keyswitch (entry i on the column
             polynomial a_i, prepared outside the timed region) and n_in adds -- so it can be taken on a library built from the parent: --lib names it
    boot     yardstick (b), the launch that produces the samples: that many functional bootstraps at the shape's parameter set (random key words)
hipEvent time around one whole call (`loop`: around the whole loop) after a warm-up of the same shape; median, minimum, maximum and spread (max - min) / median over
the repeats.  For the method of DESIGN 4.12.5 run the yardstick and the new library in two processes that alternate.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine, host

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="new,loop,boot")
ap.add_argument("--shapes", default="set1,lvl2")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes loop,boot)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
SHAPES = dict(set1=dict(P=ma.PARAMS_SET1, t=6, bb=4, per=1024, total=4096), lvl2=dict(P=ma.PARAMS_LVL2, t=4, bb=6, per=1024, total=1024))


def timed(what, run, extra=""):
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = ms[len(ms) // 2]
    print("%-58s ms: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra), flush=True)
    return med


modes = args.modes.split(",")
for name in args.shapes.split(","):
    S = SHAPES[name]
    P, t, bb, per, total = dict(S["P"]), S["t"], S["bb"], S["per"], S["total"]
    N = n_in = P["N"]
    outputs = -(-total // per)
    host.seed(0x9E2F + N)
    rk = host.RlweKey(N, 1, P["rlwe_sigma"])
    lwe = rk.extracted_lwe_key()
    msgs = (rng.integers(0, 8, size=total).astype(np.uint64)) << np.uint64(61)
    cts = ma.to_device(host.tlwe_samples(msgs, lwe), eng.device)
    src = np.zeros((n_in, N), dtype=np.uint64)
    src[:, 0] = lwe.s
    pk = eng.generate_trlwe_ks_keys(rk.s[0], src, t, bb, P["rlwe_sigma"], 0x7E57)
    print("%s: %d samples of n_in = %d into %d TRLWE of N = %d, t = %d, base_bit = %d; key %.0f MiB" % (name, total, n_in, outputs, N, t, bb, n_in * t * 2 * N * 8 / 2 ** 20), flush=True)
    if "new" in modes:
        plan = engine.tlwe_pack_plan(N, n_in, t, total, per, cus=torch.cuda.get_device_properties(eng.device).multi_processor_count)
        print("%s plan: %s" % (name, plan), flush=True)
        out = eng.empty(outputs, 2, N)
        best = None
        for split in sorted({1, 8, 16, 32, 64, plan["split"]}):
            med = timed("%s new   tlwe_pack split %d%s" % (name, split, " (the plan's)" if split == plan["split"] else ""), lambda: eng.tlwe_pack(pk, cts, per, split, out=out))
            best = (med, split) if best is None or med < best[0] else best
        print("%s fastest split measured: %d (%.4f ms)" % (name, best[1], best[0]), flush=True)
        got = ma.to_numpy(eng.tlwe_pack(pk, cts, per, plan["split"], out=out))
        s = np.ascontiguousarray(rk.s[0])
        from oracle import oracle as O
        worst = 0.0
        for o in range(outputs):
            expect = np.zeros(N, dtype=np.uint64)
            expect[:min(per, total - o * per)] = msgs[o * per:(o + 1) * per]
            worst = max(worst, float(O.torus_dist(O.trlwe_phase(got[o], s), expect).max()))
        print("%s decrypted at the plan's split: worst phase error 2^%.1f (half a slot of 1/8: 2^60)" % (name, np.log2(max(worst, 1.0))), flush=True)
        assert worst < 2.0 ** 60
    if "loop" in modes:
        cols = torch.zeros(n_in, outputs, 2, N, dtype=torch.int64, device=eng.device)      # entry i's inputs: (a_i(X), 0) per output
        padded = torch.zeros(outputs * per, n_in + 1, dtype=torch.int64, device=eng.device)
        padded[:total] = cts
        cols[:, :, 0, :per] = padded[:, :n_in].view(outputs, per, n_in).permute(2, 0, 1)
        acc, part = eng.empty(outputs, 2, N), eng.empty(outputs, 2, N)

        def loop():
            acc.zero_()
            acc[:, 1, :per] = padded[:, n_in].view(outputs, per)
            for i in range(n_in):
                eng.trlwe_keyswitch(pk, i, cols[i], out=part)
                acc.add_(part)
        timed("%s loop  %d x (trlwe_keyswitch + add)" % (name, n_in), loop)
        del cols, padded
    if "boot" in modes:
        n, l, Bg = P["n"], P["l"], P["Bg_bit"]
        bsk = eng.load_bootstrap_key(rng.integers(0, 2 ** 64, size=(n, 2 * l, 2, N), dtype=np.uint64), 1, l, Bg)
        gen = torch.Generator(device=eng.device).manual_seed(1)
        rand = lambda *shape: torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device=eng.device, generator=gen)
        tv, ins, res = rand(1, 2, N), rand(total, n + 1), eng.empty(total, N + 1)
        timed("%s boot  functional_bootstrap x %d" % (name, total), lambda: eng.functional_bootstrap(bsk, tv, ins, 4, out=res))
        bsk.free()
        del tv, ins, res
    pk.free()
    del cts
