"""Selector logic: time per call of Engine.trgsw_logic (mosfhet_hip_trgsw_logic_batch) for ONE LEVEL of AND gates against the composition of older entry points that
gives the same doubles -- so the yardstick can be taken on a library built from the parent commit (--lib), where the new call is skipped.

    python tools/gpu_perf_trgsw_logic.py [--lib PATH] [--shapes 2048,4,9:1024,2,8] [--gates 1,16,128] [--counts 1,64,1024] [--repeats 7]

The level: n_in = 2 g inputs, gate k = AND(input 2k, input 2k + 1).  Yardstick (all launches inside the timed region, every tensor it needs made outside it, the gather
of the gates' operands included -- the new call reads them in place):
    dft_to_torus of the left operands' rows, ONE external_product_dft_batch over the count * g * 2l rows against the right operands replicated once per row
    (key_stride; "rep"), or 2l such calls of count * g units each against the right operands in place ("2l"), dft_to_torus, torus_to_dft.
hipEvent time around one whole call after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.  Where the library
has the new call the yardstick's doubles are compared with its (==, as bit patterns).  Shapes whose tensors pass the cap below are skipped and named.  Inputs are
transforms of random words (timing only).
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: yardstick only)")
ap.add_argument("--shapes", default="2048,4,9:1024,2,8", help="N,l,Bg_bit[:...]")
ap.add_argument("--gates", default="1,16,128")
ap.add_argument("--counts", default="1,64,1024")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--max-gib", type=float, default=24.0, help="skip a measurement whose tensors pass this many GiB")
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
have_new = hasattr(engine.lib(), "mosfhet_hip_trgsw_logic_batch")
GiB = float(1 << 30)


def timed(label, shape, run):
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
    print("%-14s %s ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats)" % (label, shape, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med,
                                                                                                    len(ms)), flush=True)


def product(keys, stride, out, ct, N, l, Bg, units):
    engine._check(engine.lib().mosfhet_hip_external_product_dft_batch(eng.h, engine._ptr(keys), C.c_size_t(stride), engine._ptr(out), engine._ptr(ct), N, l, Bg, units,
                                                                      eng._stream()))


for spec in args.shapes.split(":"):
    N, l, Bg = (int(x) for x in spec.split(","))
    sample = 2 * l * 2 * N                      # doubles of one selector
    for g in (int(x) for x in args.gates.split(",")):
        for count in (int(c) for c in args.counts.split(",")):
            shape = "N=%d l=%d Bg=2^%d gates=%-3d count=%-5d" % (N, l, Bg, g, count)
            units = count * g
            need = units * sample * 8 * (2 + 1 + 1 + 1 + 1 + 2 * l) / GiB      # inputs, new out, X, Y, torus rows, products, replicated Y
            if need > args.max_gib:
                print("skipped        %s (%.1f GiB, of which %.1f of replicated right operands)" % (shape, need, units * sample * 8 * 2 * l / GiB), flush=True)
                continue
            gen = torch.Generator(device=eng.device).manual_seed(1)
            words = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, 2 * g, 2 * l, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
            d_in = eng.torus_to_dft(words.view(-1, N)).view(count, 2 * g, 2 * l, 2, N)
            del words
            new = None
            if have_new:
                c = eng.sellogic_create([(engine.SEL_AND, 2 * k, 2 * k + 1, -1) for k in range(g)], 2 * g, N)
                new = torch.empty(count, g, 2 * l, 2, N, dtype=torch.float64, device=eng.device)
                timed("new", shape, lambda: eng.trgsw_logic(c, d_in, l, Bg, out=new))
                c.close()
            prod = torch.empty(units * 2 * l, 2, N, dtype=torch.float64, device=eng.device)
            res = [None]

            def left_rows():
                X = d_in[:, 0::2].contiguous()
                return eng.dft_to_torus(X.view(-1, N)).view(units * 2 * l, 2, N)

            def finish():
                res[0] = eng.torus_to_dft(eng.dft_to_torus(prod.view(-1, N))).view(count, g, 2 * l, 2, N)

            def run_rep():
                tx = left_rows()
                keys = d_in[:, 1::2, None].expand(count, g, 2 * l, 2 * l, 2, N).contiguous()
                product(keys, sample, prod, tx, N, l, Bg, units * 2 * l)
                finish()

            def run_2l():
                tx = left_rows().view(units, 2 * l, 2, N)
                Y = d_in[:, 1::2].contiguous()
                out = prod.view(units, 2 * l, 2, N)
                for r in range(2 * l):
                    pr = torch.empty(units, 2, N, dtype=torch.float64, device=eng.device)
                    product(Y, sample, pr, tx[:, r].contiguous(), N, l, Bg, units)
                    out[:, r] = pr
                finish()

            for label, run in (("yardstick rep", run_rep), ("yardstick 2l", run_2l)):
                timed(label, shape, run)
                if new is not None:
                    assert torch.equal(res[0].view(torch.int64), new.view(torch.int64)), label + ": other doubles than the new call"
            del d_in, new, prod
            res[0] = None
            torch.cuda.empty_cache()
