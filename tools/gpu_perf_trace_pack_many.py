"""Many samples per output by the trace: time per call of Engine.tlwe_trace_pack_many (mosfhet_hip_tlwe_trace_pack_many_batch) against the fastest way to the
same packed content with the small key before.

    python tools/gpu_perf_trace_pack_many.py [--modes many,yard,pack] [--shapes full1,full16,set1,mid] [--lib PATH] [--repeats 7]

--shapes (key t 4, base_bit 9 everywhere; the key rows are random words: the time does not depend on them):
    full1    N 2048, log_per 11, 1 output (2048 samples)        full16   N 2048, log_per 11, 16 outputs
    set1     N 1024, log_per 10, 4 outputs                       mid      N 2048, log_per 4, 256 outputs (4096 samples)
--modes, one after the other in one process:
    many     the new call
    yard     the yardstick, from entry points of the parent commit so that it can be taken on a library built from the parent (--lib names it): tlwe_trace_pack on all
             `total` samples, then out[o] = sum_j X^(j N / n) trace(in[o n + j]) as tensor operations (one gather with the shifts' indices, the signs, one sum)
    pack     context only: tlwe_pack of the same counts with a device-made key of N entries (another key, no factor N), at the split its plan recommends
hipEvent time around one whole call or composition after a warm-up of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.
Run the parent's library and this one in two processes that alternate.
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
ap.add_argument("--modes", default="many,yard")
ap.add_argument("--shapes", default="full1,full16,set1,mid")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes yard)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
T, BB = 4, 9
SHAPES = dict(full1=dict(N=2048, L=11, outputs=1), full16=dict(N=2048, L=11, outputs=16), set1=dict(N=1024, L=10, outputs=4), mid=dict(N=2048, L=4, outputs=256))


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
    N, L, outputs = S["N"], S["L"], S["outputs"]
    n, steps = 1 << L, N.bit_length() - 1
    total = outputs * n
    rows = rng.integers(0, 2 ** 64, size=(steps, T, 2, N), dtype=np.uint64)
    tks = eng.load_trlwe_ks_keys(rows, BB)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    cts = torch.randint(-2 ** 63, 2 ** 63 - 1, (total, N + 1), dtype=torch.int64, device=eng.device, generator=gen)
    out = eng.empty(outputs, 2, N)
    print("%s: %d samples at N = %d, %d per output, %d outputs; key t = %d, base_bit = %d, %d entries of %.2f MiB in all; %d merges and %d trace steps per output" % (
        name, total, N, n, outputs, T, BB, steps, steps * T * 2 * N * 8 / 2 ** 20, n - 1, steps - L), flush=True)
    if "many" in modes:
        plan = engine.tlwe_trace_pack_many_plan(N, T, BB, steps, total, L)
        ms = timed("%s many  tlwe_trace_pack_many" % name, lambda: eng.tlwe_trace_pack_many(tks, cts, L, out=out),
                   "  %d rounds of %d launches, pool %.1f MiB" % (plan["rounds"], plan["launches_per_round"], plan["pool_bytes"] / 2 ** 20))
        print("%s %.2f us per packed sample" % (name, 1e3 * ms / total), flush=True)
    if "yard" in modes:
        traced = eng.empty(total, 2, N)
        j, i = torch.arange(n, device=eng.device).view(n, 1), torch.arange(N, device=eng.device).view(1, N)
        src = i - j * (N // n)                                       # X^(j N / n) p [i] = p[i - j N / n], negated where the index wraps
        idx = (src % N).view(1, n, 1, N).expand(outputs, n, 2, N)
        sign = torch.where(src < 0, -1, 1).view(1, n, 1, N)
        res = eng.empty(outputs, 2, N)

        def yardstick():
            eng.tlwe_trace_pack(tks, cts, 0, out=traced)
            torch.sum(torch.gather(traced.view(outputs, n, 2, N), 3, idx) * sign, dim=1, out=res)

        timed("%s yard  tlwe_trace_pack on %d samples + shifts and adds" % (name, total), yardstick)
        timed("%s yard  ... its tlwe_trace_pack alone" % name, lambda: eng.tlwe_trace_pack(tks, cts, 0, out=traced))
        del traced, idx, sign, res
    if "pack" in modes:
        s = rng.integers(0, 2, size=N).astype(np.uint64)
        msgs = np.zeros((N, N), dtype=np.uint64)
        msgs[np.arange(N), 0] = s
        pk = eng.generate_trlwe_ks_keys(s, msgs, T, BB, 2.0 ** -50, 0x7E57)
        split = engine.tlwe_pack_plan(N, N, T, total, n)["split"]
        timed("%s pack  tlwe_pack, split %d (key %.0f MiB)" % (name, split, N * T * 2 * N * 8 / 2 ** 20), lambda: eng.tlwe_pack(pk, cts, per=n, split=split, out=out))
        pk.free()
    tks.free()
    del cts, out
