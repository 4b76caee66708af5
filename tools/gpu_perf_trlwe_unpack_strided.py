"""Packed TRLWE samples opened at an offset and a stride: time per call of Engine.trlwe_unpack_strided_keyswitch (mosfhet_hip_trlwe_unpack_strided_keyswitch_batch;
DESIGN 4.20) against the fastest way to the same words on the parent build, against the unstrided fused call, and the calls that must not have moved.

    python tools/gpu_perf_trlwe_unpack_strided.py [--modes strided,yardstick,level] [--shapes set1,lvl2] [--lib PATH] [--repeats 7]

--shapes (those of tools/gpu_perf_trlwe_unpack.py, opened 64 per input at first 0, stride N / 64):
    set1     4096 values at SET_1: N 1024, 64 inputs, the LWE key of bench.py's gate leg (N -> 585, t 5, base_bit 2)
    lvl2     1024 values at N 2048, 16 inputs, the lvl2 LWE key (N -> 632, t 8, base_bit 4)
--modes, one after the other in one process:
    strided    this build only.  The strided fused call beside the unstrided fused call at the same (total, per), in the word-lane form and -- with set_ks_words(0) --
               in the tiles; the strided unpack beside the unstrided one; the fused words are compared with trlwe_unpack_strided followed by tlwe_keyswitch.
    yardstick  entry points of the parent commit only, so that it can be taken on a library built from the parent (--lib names it): trlwe_unpack with
               per' = first + (per - 1) stride + 1, a device gather of the wanted rows into a contiguous batch, tlwe_keyswitch -- the fastest way to the same words there.
    level      entry points of the parent commit only, for both builds: trlwe_unpack, trlwe_unpack_keyswitch and unpack_keyswitch_functional_bootstrap at the shape
               (per 64), and the table key switch on 4096 plain rows (tools/gpu_perf_ks.py's shapes).
hipEvent time around one whole call after a warm-up of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.  For the method of
DESIGN 4.19.1 run the parent's library and this one in processes that alternate.
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
ap.add_argument("--modes", default="strided,yardstick,level")
ap.add_argument("--shapes", default="set1,lvl2")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes yardstick,level)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
SHAPES = dict(set1=dict(P=ma.PARAMS_SET1, total=4096), lvl2=dict(P=ma.PARAMS_LVL2, total=1024))
PER, PLAIN_ROWS = 64, 4096
build = "parent" if args.lib else "this"


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
    print("%-78s ms: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra), flush=True)
    return med


modes = args.modes.split(",")
for name in args.shapes.split(","):
    S = SHAPES[name]
    P, total, per = dict(S["P"]), S["total"], PER
    N, n, t, bb = P["N"], P["n"], P["t"], P["base_bit"]
    first, stride = 0, N // per
    outputs = -(-total // per)
    s_in, s_out = rng.integers(0, 2, size=N).astype(np.uint64), rng.integers(0, 2, size=n).astype(np.uint64)
    ksk = eng.generate_keyswitch_key(s_out, s_in, t, bb, P["lwe_sigma"], seed=0x7E57)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    packed = torch.randint(-2 ** 63, 2 ** 63 - 1, (outputs, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
    batch, switched = eng.empty(total, N + 1), eng.empty(total, n + 1)
    tag = "%s %s" % (name, build)
    print("%s: %d values in %d TRLWE of N = %d, per = %d, first = %d, stride = %d; switch to n = %d, t = %d, base_bit = %d; key %.0f MiB" % (
        tag, total, outputs, N, per, first, stride, n, t, bb, ksk.nbytes / 2 ** 20), flush=True)
    if "strided" in modes:
        cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
        a = timed("%s trlwe_unpack_strided" % tag, lambda: eng.trlwe_unpack_strided(packed, total, per, first, stride, out=batch))
        b = timed("%s trlwe_unpack (same total, per)" % tag, lambda: eng.trlwe_unpack(packed, total, per, out=batch))
        print("%s the strided unpack is %.3f x the unstrided one" % (tag, a / b), flush=True)
        eng.trlwe_unpack_strided(packed, total, per, first, stride, out=batch)
        want = eng.tlwe_keyswitch(ksk, batch).clone()
        for setting in (-1, 0):
            try:
                engine.set_ks_words(setting)
                form = engine.trlwe_unpack_strided_plan(N, n, t, bb, total, per, first, stride, cus=cus)["form"]
                a = timed("%s %-9s trlwe_unpack_strided_keyswitch" % (tag, form), lambda: eng.trlwe_unpack_strided_keyswitch(ksk, packed, total, per, first, stride, out=switched))
                assert bool((switched == want).all()), "the strided fused words differ from the composition's"
                b = timed("%s %-9s trlwe_unpack_keyswitch (same total, per)" % (tag, form), lambda: eng.trlwe_unpack_keyswitch(ksk, packed, total, per, out=switched))
                a2 = timed("%s %-9s trlwe_unpack_strided_keyswitch, again (after the unstrided call)" % (tag, form),
                           lambda: eng.trlwe_unpack_strided_keyswitch(ksk, packed, total, per, first, stride, out=switched))
                print("%s %s: the strided fused call is %.3f x the unstrided fused call (timed before it), %.3f x (timed after it)" % (tag, form, a / b, a2 / b), flush=True)
            finally:
                engine.set_ks_words(-1)
    if "yardstick" in modes:
        wide_per = first + (per - 1) * stride + 1
        wide = eng.empty(outputs * wide_per, N + 1)

        def yardstick():
            eng.trlwe_unpack(packed, outputs * wide_per, wide_per, out=wide)
            batch.view(outputs, per, N + 1).copy_(wide.view(outputs, wide_per, N + 1)[:, first::stride])
            eng.tlwe_keyswitch(ksk, batch, out=switched)
        timed("%s yardstick: trlwe_unpack per' = %d (%.0f MB), gather, tlwe_keyswitch" % (tag, wide_per, wide.numel() * 8 / 1e6), yardstick)
        timed("%s yardstick, first step alone: trlwe_unpack per' = %d" % (tag, wide_per), lambda: eng.trlwe_unpack(packed, outputs * wide_per, wide_per, out=wide))
        if "strided" in modes:
            assert bool((switched == want).all()), "the yardstick's words differ from the strided call's"
        del wide
    if "level" in modes:
        timed("%s level trlwe_unpack" % tag, lambda: eng.trlwe_unpack(packed, total, per, out=batch))
        timed("%s level trlwe_unpack_keyswitch" % tag, lambda: eng.trlwe_unpack_keyswitch(ksk, packed, total, per, out=switched))
        s_ring = s_in
        bsk = eng.generate_bootstrap_key(s_ring, s_out, P["l"], P["Bg_bit"], P["rlwe_sigma"], 0xB5C)
        tv = torch.randint(-2 ** 63, 2 ** 63 - 1, (1, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
        boot = eng.empty(total, N + 1)
        timed("%s level unpack_keyswitch_functional_bootstrap" % tag, lambda: eng.unpack_keyswitch_functional_bootstrap(ksk, bsk, tv, packed, total, per, 4, out=boot))
        bsk.free()
        plain = torch.randint(-2 ** 63, 2 ** 63 - 1, (PLAIN_ROWS, N + 1), dtype=torch.int64, device=eng.device, generator=gen)
        plain_out = eng.empty(PLAIN_ROWS, n + 1)
        timed("%s level tlwe_keyswitch of %d plain rows" % (tag, PLAIN_ROWS), lambda: eng.tlwe_keyswitch(ksk, plain, out=plain_out))
        del plain, plain_out, boot, tv
    ksk.free()
    del packed, batch, switched
