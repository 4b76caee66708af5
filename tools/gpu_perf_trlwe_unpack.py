"""Packed TRLWE samples opened into LWE batches: time per call of Engine.trlwe_unpack and Engine.trlwe_unpack_keyswitch (mosfhet_hip_trlwe_unpack_batch,
mosfhet_hip_trlwe_unpack_keyswitch_batch) against what the library could do before.

    python tools/gpu_perf_trlwe_unpack.py [--modes new,old] [--shapes set1,lvl2] [--lib PATH] [--repeats 7]

--shapes:
    set1     4096 values at SET_1: N 1024, 4 inputs, per 1024, the LWE key of bench.py's gate leg (N -> 585, t 5, base_bit 2)
    lvl2     1024 values at N 2048, 1 input, per 1024, the lvl2 LWE key (N -> 632, t 8, base_bit 4)
--modes, one after the other in one process:
    new      part 1 (trlwe_unpack) beside a hipMemsetAsync of the same bytes (the write-only floor); part 2 (trlwe_unpack_keyswitch) beside the composition on this
             build (trlwe_unpack, then tlwe_keyswitch); the fused words are compared with the composition's
    old      the yardsticks from entry points of the parent commit, so that they can be taken on a library built from the parent (--lib names it): `per` calls of
             trlwe_extract_tlwe over the inputs plus the gather into batch order, and tlwe_keyswitch of an already unpacked batch (the cost the pre-pass of part 2
             cannot go below)
hipEvent time around one whole call (the yardstick: around the whole loop and the gather) after a warm-up of the same shape; median, minimum, maximum and spread
(max - min) / median over the repeats.  For the method of DESIGN 4.12.5 run the parent's library and this one in two processes that alternate.
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
ap.add_argument("--modes", default="new,old")
ap.add_argument("--shapes", default="set1,lvl2")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes old)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
SHAPES = dict(set1=dict(P=ma.PARAMS_SET1, per=1024, total=4096), lvl2=dict(P=ma.PARAMS_LVL2, per=1024, total=1024))


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
    print("%-62s ms: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra), flush=True)
    return med


modes = args.modes.split(",")
for name in args.shapes.split(","):
    S = SHAPES[name]
    P, per, total = dict(S["P"]), S["per"], S["total"]
    N, n, t, bb = P["N"], P["n"], P["t"], P["base_bit"]
    outputs = -(-total // per)
    s_in, s_out = rng.integers(0, 2, size=N).astype(np.uint64), rng.integers(0, 2, size=n).astype(np.uint64)
    ksk = eng.generate_keyswitch_key(s_out, s_in, t, bb, P["lwe_sigma"], seed=0x7E57)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    packed = torch.randint(-2 ** 63, 2 ** 63 - 1, (outputs, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
    batch, switched = eng.empty(total, N + 1), eng.empty(total, n + 1)
    print("%s: %d values in %d TRLWE of N = %d, per = %d; switch to n = %d, t = %d, base_bit = %d; key %.0f MiB; the batch %.1f MB" % (
        name, total, outputs, N, per, n, t, bb, ksk.nbytes / 2 ** 20, total * (N + 1) * 8 / 1e6), flush=True)
    if "new" in modes:
        cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
        print("%s plan of part 1: %s" % (name, engine.trlwe_unpack_plan(N, total=total, per=per, cus=cus)), flush=True)
        print("%s plan of part 2: %s" % (name, engine.trlwe_unpack_plan(N, n, t, bb, total, per, cus=cus)), flush=True)
        one = timed("%s new   trlwe_unpack" % name, lambda: eng.trlwe_unpack(packed, total, per, out=batch))
        floor = timed("%s new   memset of the batch's bytes" % name, lambda: batch.zero_())
        print("%s part 1 is %.2f x the write-only floor" % (name, one / floor), flush=True)
        fused = timed("%s new   trlwe_unpack_keyswitch" % name, lambda: eng.trlwe_unpack_keyswitch(ksk, packed, total, per, out=switched))
        got = switched.clone()

        def composition():
            eng.trlwe_unpack(packed, total, per, out=batch)
            eng.tlwe_keyswitch(ksk, batch, out=switched)
        comp = timed("%s new   trlwe_unpack, then tlwe_keyswitch" % name, composition)
        assert bool((got == switched).all()), "the fused words differ from the composition's"
        print("%s part 2 is %.3f x the composition (same words)" % (name, fused / comp), flush=True)
    if "old" in modes:
        tmp = eng.empty(per, outputs, N + 1)

        def yardstick():
            for j in range(per):
                eng.trlwe_extract_tlwe(packed, j, out=tmp[j])
            batch.view(outputs, per, N + 1)[:, :total // outputs].copy_(tmp.permute(1, 0, 2)[:, :total // outputs])
        timed("%s old   %d x trlwe_extract_tlwe + gather" % (name, per), yardstick)
        timed("%s old   tlwe_keyswitch of an unpacked batch" % name, lambda: eng.tlwe_keyswitch(ksk, batch, out=switched))
        del tmp
    ksk.free()
    del packed, batch, switched
