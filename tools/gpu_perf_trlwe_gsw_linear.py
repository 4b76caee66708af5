"""Encrypted polynomial-weight linear layers on packed TRLWE samples: time per call of Engine.trlwe_gsw_linear (mosfhet_hip_trlwe_gsw_linear_batch) against
the fastest composition of the entry points before it for the same function.

    python tools/gpu_perf_trlwe_gsw_linear.py [--modes gsw,yard] [--gadgets 1024:2:8,2048:4:9] [--rows-out 1,16,64] [--counts 1,64,1024] [--lib PATH] [--repeats 7]

rows_in = 4 everywhere; inputs and TRGSW rows are random words (the time does not depend on them).
--modes, one after the other in one process:
    gsw      the new call, TRLWE mode: [count][4][2][N] -> [count][rows_out][2][N]; and, for context, the extract mode at 0
    yard     the yardstick, from entry points of the parent commit so that it can be taken on a library built from the parent (--lib names it): the inputs laid out
             [4][count][2][N]; per (output row j, input e) one mosfhet_hip_external_product_dft_batch over the count samples of input e with the one shared TRGSW_DFT
             W[j][e], and one mosfhet_hip_dft_lincomb_batch into row j's DFT-domain accumulator (the first product of a row is written straight into it); then one
             mosfhet_hip_dft_to_torus_batch over all rows.  Output buffers are allocated once, outside the timed region; everything else is inside it.
hipEvent time around one whole call or composition after a warm-up of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.
Run the parent's library and this one in two processes that alternate.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="gsw,yard")
ap.add_argument("--gadgets", default="1024:2:8,2048:4:9")
ap.add_argument("--rows-out", default="1,16,64")
ap.add_argument("--counts", default="1,64,1024")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes yard)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
L = engine.lib()
stream = torch.cuda.current_stream()
ROWS_IN = 4


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
    print("%-74s ms: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra), flush=True)
    return med


def ptr(t):
    return C.c_void_p(t.data_ptr())


modes = args.modes.split(",")
gen = torch.Generator(device=eng.device).manual_seed(1)
for N, l, Bg in (tuple(int(v) for v in g.split(":")) for g in args.gadgets.split(",")):
    for rows_out in (int(v) for v in args.rows_out.split(",")):
        W = torch.randint(-2 ** 63, 2 ** 63 - 1, (rows_out, ROWS_IN, 2 * l, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
        W_dft = eng.torus_to_dft(W.view(-1, N)).view(rows_out, ROWS_IN, 2 * l, 2, N)
        for count in (int(v) for v in args.counts.split(",")):
            tag = "N %d l %d Bg_bit %d rows_out %d count %d" % (N, l, Bg, rows_out, count)
            x = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, ROWS_IN, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
            if "gsw" in modes:
                lin = eng.gswlinear_create_from_selectors(W_dft.view(-1, 2 * l, 2, N), np.arange(rows_out + 1) * ROWS_IN, np.tile(np.arange(ROWS_IN), rows_out), ROWS_IN, Bg)
                plan = engine.trlwe_gsw_linear_plan(N, l, rows_out, ROWS_IN, count)
                full = eng.empty(count, rows_out, 2, N)
                timed("%s gsw    trlwe_gsw_linear" % tag, lambda: eng.trlwe_gsw_linear(lin, x, out=full),
                      "  %d rounds of %d teams, pool %.1f MiB" % (plan["rounds"], plan["teams"], plan["pool_bytes"] / 2 ** 20))
                ext = eng.empty(count, rows_out, N + 1)
                timed("%s gsw    trlwe_gsw_linear_extract" % tag, lambda: eng.trlwe_gsw_linear_extract(lin, x, 0, out=ext))
                del full, ext
                lin.close()
            if "yard" in modes:
                xt = x.transpose(0, 1).contiguous()                                                        # [4][count][2][N]
                acc = torch.empty(rows_out, count, 2, N, dtype=torch.float64, device=eng.device)
                prod = torch.empty(count, 2, N, dtype=torch.float64, device=eng.device)
                out = eng.empty(rows_out, count, 2, N)
                s, one, words = eng._stream(), C.c_double(1.0), C.c_size_t(count * 2 * N)

                # every pointer is made once: the timed region holds the library calls alone
                p_w = [[ptr(W_dft[j, e]) for e in range(ROWS_IN)] for j in range(rows_out)]
                p_acc, p_x, p_prod, p_out, p_all, zero = [ptr(acc[j]) for j in range(rows_out)], [ptr(xt[e]) for e in range(ROWS_IN)], ptr(prod), ptr(out), ptr(acc), C.c_size_t(0)

                def yardstick():
                    for j in range(rows_out):
                        for e in range(ROWS_IN):
                            engine._check(L.mosfhet_hip_external_product_dft_batch(eng.h, p_w[j][e], zero, p_acc[j] if e == 0 else p_prod, p_x[e], N, l, Bg, count, s))
                            if e:
                                engine._check(L.mosfhet_hip_dft_lincomb_batch(eng.h, p_acc[j], p_acc[j], p_prod, one, words, s))
                    engine._check(L.mosfhet_hip_dft_to_torus_batch(eng.h, p_out, p_all, N, rows_out * count * 2, s))

                timed("%s yard   external_product_dft + dft_lincomb per (j, e), one dft_to_torus" % tag, yardstick, "  %d launches" % (rows_out * (2 * ROWS_IN - 1) + 1))
                del xt, acc, prod, out
            del x
