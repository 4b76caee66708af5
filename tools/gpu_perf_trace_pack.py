"""The trace switch and the gadget -> TRGSW conversion: time per call of Engine.tlwe_trace_pack and Engine.trgsw_from_gadget (mosfhet_hip_tlwe_trace_pack_batch,
mosfhet_hip_trgsw_from_gadget_batch) against the fastest way to the same words before.

    python tools/gpu_perf_trace_pack.py [--modes new,old,table] [--shapes lvl2,set1,one] [--lib PATH] [--repeats 7]

--shapes (key t 4, base_bit 9 everywhere; the key rows are random words: the time does not depend on them):
    lvl2     1024 samples at N 2048          set1     4096 samples at N 1024          one      1 sample at N 2048
--modes, one after the other in one process:
    new      the fused calls; their words are compared with the composition's on this build
    old      the yardsticks, from entry points of the parent commit so that they can be taken on a library built from the parent (--lib names it).  Yardstick 1: the
             embedding (three tensor operations), then log2 N rounds of trlwe_eval_automorphism_entry (gen N / 2^j + 1, entry j) and a word-wise add.  For the gadget
             conversion (l 2 at N 1024, l 4 at N 2048, `count` = samples / 16 inputs): two trlwe_keyswitch calls over all count * l rows at once, the subtraction,
             and torus_to_dft of the 2 l rows -- already batched over the rows, which the host loop of the drop-in layer is not
    table    yardstick 2, context only: trlwe_packing1_keyswitch of the same count with a device-made table key (t 12, base_bit 2: 2.4 GB at N 2048) -- another key,
             and its result is not scaled by N
hipEvent time around one whole call or composition after a warm-up of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.
For the method of DESIGN 4.12.5 run the parent's library and this one in two processes that alternate.
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
ap.add_argument("--shapes", default="lvl2,set1,one")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes old)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
T, BB = 4, 9
SHAPES = dict(lvl2=dict(N=2048, count=1024, l=4), set1=dict(N=1024, count=4096, l=2), one=dict(N=2048, count=1, l=4))


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
    print("%-66s ms: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra), flush=True)
    return med


modes = args.modes.split(",")
for name in args.shapes.split(","):
    S = SHAPES[name]
    N, count, l = S["N"], S["count"], S["l"]
    steps = N.bit_length() - 1
    rows = rng.integers(0, 2 ** 64, size=(steps + 2, T, 2, N), dtype=np.uint64)
    tks = eng.load_trlwe_ks_keys(rows, BB)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    cts = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, N + 1), dtype=torch.int64, device=eng.device, generator=gen)
    inputs = max(1, count // 16)
    gadget = torch.randint(-2 ** 63, 2 ** 63 - 1, (inputs, l, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
    acc, tmp = eng.empty(count, 2, N), eng.empty(count, 2, N)
    print("%s: %d samples at N = %d, key t = %d, base_bit = %d, %d trace entries of %.2f MiB in all; gadget conversion of %d inputs, l = %d" % (
        name, count, N, T, BB, steps, steps * T * 2 * N * 8 / 2 ** 20, inputs, l), flush=True)

    def composition():
        acc[:, 0, 0] = cts[:, 0]
        acc[:, 0, 1:] = -cts[:, 1:N].flip(1)
        acc[:, 1] = 0
        acc[:, 1, 0] = cts[:, N]
        for j in range(steps):
            eng.trlwe_eval_automorphism_entry(tks, j, acc, (N >> j) + 1, out=tmp)
            acc.add_(tmp)

    src, as_, bs_ = torch.zeros(inputs * l, 2, N, dtype=torch.int64, device=eng.device), eng.empty(inputs * l, 2, N), eng.empty(inputs * l, 2, N)
    words = eng.empty(inputs, 2 * l, 2, N)

    def gadget_composition():
        g = gadget.view(inputs * l, 2, N)
        src[:, 0] = g[:, 0]
        eng.trlwe_keyswitch(tks, steps, src, out=as_)
        src[:, 0] = g[:, 1]
        eng.trlwe_keyswitch(tks, steps + 1, src, out=bs_)
        words[:, :l] = (as_ - bs_).view(inputs, l, 2, N)
        words[:, l:] = gadget
        return eng.torus_to_dft(words.view(-1, N))

    if "new" in modes:
        out = eng.empty(count, 2, N)
        fused = timed("%s new   tlwe_trace_pack" % name, lambda: eng.tlwe_trace_pack(tks, cts, 0, out=out))
        comp = timed("%s new   embedding + %d x (eval_automorphism_entry + add)" % (name, steps), composition)
        assert bool((out == acc).all()), "the fused words differ from the composition's"
        print("%s the trace is %.3f x the composition (same words): %.2f us per sample" % (name, fused / comp, 1e3 * fused / count), flush=True)
        sel = torch.empty(inputs, 2 * l, 2, N, dtype=torch.float64, device=eng.device)
        gf = timed("%s new   trgsw_from_gadget" % name, lambda: eng.trgsw_from_gadget(tks, gadget, steps, out=sel))
        gc = timed("%s new   2 x trlwe_keyswitch + subtract + torus_to_dft" % name, gadget_composition)
        assert bool(torch.equal(sel.view(-1, N), gadget_composition())), "the selectors differ from the composition's"
        print("%s the gadget conversion is %.3f x the composition (same doubles)" % (name, gf / gc), flush=True)
    if "old" in modes:
        timed("%s old   embedding + %d x (eval_automorphism_entry + add)" % (name, steps), composition)
        timed("%s old   2 x trlwe_keyswitch + subtract + torus_to_dft" % name, gadget_composition)
    if "table" in modes:
        s = rng.integers(0, 2, size=N).astype(np.uint64)
        table = eng.generate_table_key(0, s, s, 12, 2, 2.0 ** -44, 0x7AB1E)
        res = eng.empty(count, 2, N)
        timed("%s table trlwe_packing1_keyswitch (key %.0f MiB)" % (name, table.nbytes / 2 ** 20), lambda: eng.trlwe_packing1_keyswitch(table, cts, out=res))
        table.free()
        del res
    tks.free()
    del cts, gadget, acc, tmp, src, as_, bs_, words
