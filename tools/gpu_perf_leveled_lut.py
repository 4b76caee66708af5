"""Leveled LUT on a batch of independent TRGSW-encrypted inputs: time per call of Engine.leveled_lut (mosfhet_hip_leveled_lut_batch) and of the per-input route
that existed before it (--loop: per input a key view, one cmux launch per tree level, blind_rotate_ of count 1, trlwe_extract_tlwe -- tests/test_leveled_lut.py::
test_leveled_lut_equals_the_existing_route shows that both give the same words).

    python tools/gpu_perf_leveled_lut.py [--loop [--order reference]] [--lib PATH] [--sets 1024,3,10,13:2048,1,23,16:2048,4,9,12] [--counts 1,128,1024] [--repeats 7]

hipEvent time around one whole call (all `count` inputs) after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the
repeats.  --loop uses only entry points older than the new call, so the yardstick can be taken on a library built from the parent commit: --lib names it.
--order: the product order of the loop's key views (default: the library's, auto).  At N = 2048 with l = 2, 4 or 6 a small batch under `auto` runs on the
two-CU split kernels, which sum by accumulator component: faster for one input, but not the words of the reference's order that the new call (and `reference`) gives.
Selectors and table are random words (timing only).  Also prints, per shape, the bytes and FLOPs of level 0 as the algorithm needs them, for the shares of peak
(8 TB/s, 78.6 TFLOP/s FP64) against lut_level0_kernel's time from a kernel trace.
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
ap.add_argument("--loop", action="store_true", help="the per-input route through cmux / blind_rotate_ / trlwe_extract_tlwe instead of the new call")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build for --loop)")
ap.add_argument("--order", choices=("auto", "reference", "by_component"), help="--loop: product order set on every key view")
ap.add_argument("--sets", default="1024,3,10,13:2048,1,23,16:2048,4,9,12", help="N,l,Bg_bit,size[:...]")
ap.add_argument("--counts", default="1,128,1024")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()


def level0_work(N, l, size, count):
    """(bytes, FLOPs) of level 0 as the algorithm needs them: the intermediates written and read back by the next level, the base rows once, one selector per input
    (the prepared rows and the table are meant to stay in the L2s); 2l complex multiply-add rows per output component (8 FLOPs each) and two inverse transforms"""
    log_N = N.bit_length() - 1
    half = 1 << (size - log_N - 1) if size > log_N else 0
    M = N // 2
    byt = 2 * count * half * 2 * N * 8 + half * 2 * N * 8 + count * 2 * l * 2 * M * 16
    flops = count * half * (2 * l * 2 * M * 8 + 2 * 5 * M * (log_N - 1))
    return byt, flops


for spec in args.sets.split(":"):
    N, l, Bg, size = (int(x) for x in spec.split(","))
    log_N = N.bit_length() - 1
    n_luts = max(1, (1 << size) >> log_N)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    lut = torch.randint(-2 ** 63, 2 ** 63 - 1, (n_luts, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
    a = np.zeros(size + 1, dtype=np.uint64)
    for i in range(min(size, log_N)):
        a[i] = ((2 * N - (1 << i)) << (64 - (log_N + 1))) % 2 ** 64
    d_a = ma.to_device(a[None], eng.device)
    for count in (int(c) for c in args.counts.split(",")):
        sel = eng.trgsw_to_dft(torch.randint(-2 ** 63, 2 ** 63 - 1, (count, size, 2 * l, 2, N), dtype=torch.int64, device=eng.device, generator=gen))
        out = eng.empty(count, N + 1)
        if args.loop:
            work = eng.empty(max(1, n_luts // 2), 2, N)

            def run():
                for b in range(count):
                    key = eng.bootstrap_key_view(sel[b], 1, l, Bg)
                    if args.order:
                        key.set_product_order(args.order)
                    for i in range(size - log_N):
                        half = 1 << (size - log_N - i - 1)
                        src = lut if i == 0 else work          # (the first level reads the shared table and writes the input's own rows: no copy of the table)
                        eng.cmux(key, size - i - 1, src[:half], src[half:2 * half], out=work[:half])
                    acc = work[:1]
                    if size <= log_N:
                        acc.copy_(lut[:1])
                    eng.blind_rotate_(key, acc, d_a)
                    eng.trlwe_extract_tlwe(acc, 0, out=out[b:b + 1])
                    key.free()
        else:
            def run():
                eng.leveled_lut(sel, lut, size, l, Bg, out=out)
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
        byt, flops = level0_work(N, l, size, count)
        print("%-14s N=%d l=%d Bg=2^%d size=%d count=%-5d ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats); per input %.1f us; "
              "level 0 needs %.1f MB, %.2f GFLOP" % (("loop/" + (args.order or "auto")) if args.loop else "new", N, l, Bg, size, count, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms),
                                                     1e3 * med / count, byt / 1e6, flops / 1e9), flush=True)
        del sel, out
