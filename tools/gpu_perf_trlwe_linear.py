"""Polynomial-weight linear layers on packed TRLWE samples: time per call of Engine.trlwe_linear_extract (mosfhet_hip_trlwe_linear_extract_batch) against the
fastest way to the same function with the entry points before it.

    python tools/gpu_perf_trlwe_linear.py [--modes packed,yard] [--rings 1024,2048] [--rows-out 1,16,64] [--counts 1,64,1024] [--lib PATH] [--repeats 7]

rows_in = 4 everywhere; inputs, weights and bias are random words (the time does not depend on them).
--modes, one after the other in one process:
    packed   the new call, extract at 0: [count][4][2][N] -> [count][rows_out][N + 1]; and, for context, the TRLWE mode
    yard     the yardstick, from entry points of the parent commit so that it can be taken on a library built from the parent (--lib names it): trlwe_unpack of the
             count * 4 samples into count * 4 * N LWE samples, then tlwe_linear, dense, W [rows_out][4 N].  The unpacked batch is 4 N (N + 1) words per batch element
             (32 MiB at N = 1024): the yardstick runs in chunks of batch elements that keep it within --yard-bytes (1 GiB), all chunks inside the timed region.
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
ap.add_argument("--modes", default="packed,yard")
ap.add_argument("--rings", default="1024,2048")
ap.add_argument("--rows-out", default="1,16,64")
ap.add_argument("--counts", default="1,64,1024")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes yard)")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--yard-bytes", type=int, default=1 << 30)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
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


modes = args.modes.split(",")
gen = torch.Generator(device=eng.device).manual_seed(1)
for N in (int(v) for v in args.rings.split(",")):
    for rows_out in (int(v) for v in args.rows_out.split(",")):
        W = rng.integers(-128, 128, size=(rows_out, ROWS_IN, N), dtype=np.int64)
        for count in (int(v) for v in args.counts.split(",")):
            tag = "N %d rows_out %d count %d" % (N, rows_out, count)
            x = torch.randint(-2 ** 63, 2 ** 63 - 1, (count, ROWS_IN, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
            out = eng.empty(count, rows_out, N + 1)
            if "packed" in modes:
                lin = eng.polylinear_create_dense(W)
                plan = engine.trlwe_linear_plan(N, rows_out, ROWS_IN, count, extract=True)
                timed("%s packed trlwe_linear_extract" % tag, lambda: eng.trlwe_linear_extract(lin, x, 0, out=out),
                      "  %d rounds of %d teams, pool %.1f MiB" % (plan["rounds"], plan["teams"], plan["pool_bytes"] / 2 ** 20))
                full = eng.empty(count, rows_out, 2, N)
                timed("%s packed trlwe_linear (TRLWE mode)" % tag, lambda: eng.trlwe_linear(lin, x, out=full))
                del full
                lin.close()
            if "yard" in modes:
                ylin = eng.linear_dense(W.reshape(rows_out, ROWS_IN * N))
                chunk = max(1, min(count, args.yard_bytes // (ROWS_IN * N * (N + 1) * 8)))
                lwe = eng.empty(chunk * ROWS_IN * N, N + 1)

                def yardstick():
                    for b0 in range(0, count, chunk):
                        n = min(chunk, count - b0)
                        eng.trlwe_unpack(x[b0:b0 + n].view(n * ROWS_IN, 2, N), n * ROWS_IN * N, N, out=lwe[:n * ROWS_IN * N])
                        eng.tlwe_linear(ylin, lwe[:n * ROWS_IN * N].view(n, ROWS_IN * N, N + 1), out=out[b0:b0 + n])

                timed("%s yard   trlwe_unpack + tlwe_linear dense [%d][%d]" % (tag, rows_out, ROWS_IN * N), yardstick, "  chunks of %d batch elements" % chunk)
                ylin.close()
                del lwe
            del x, out
