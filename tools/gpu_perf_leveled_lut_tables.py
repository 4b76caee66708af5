"""Leveled LUT with several shared tables over the same inputs: time per call of Engine.leveled_lut_tables (mosfhet_hip_leveled_lut_tables_batch) against the
per-table loop -- `tables` calls of Engine.leveled_lut (mosfhet_hip_leveled_lut_batch) on one stream, which tests/test_leveled_lut_tables.py::
test_tables_equal_the_one_table_call shows to give the same words.

    python tools/gpu_perf_leveled_lut_tables.py [--modes loop,new,new:3] [--lib PATH] [--sets 1024,3,10,13:2048,1,23,16:2048,4,9,12] [--tables 1,4,8]
                                                [--counts 1,128,1024] [--repeats 7]

--modes: what to time, per shape one after the other (so that the modes of one shape alternate within one process):
    loop     `tables` calls of leveled_lut -- only entry points of the parent commit, so the yardstick can be taken on a library built from it: --lib names it
    new      leveled_lut_tables at the default number of tables per finishing workgroup
    new:G    ... with mosfhet_hip_set_leveled_lut_tables_group(G) (capped by the LDS of a CU: 8 at N = 1024, 3 at N = 2048)
hipEvent time around one whole call (all `count` inputs, all tables) after a warm-up call of the same shape; median, minimum, maximum and spread
(max - min) / median over the repeats.  Selectors and tables are random words (timing only).  Also prints, per shape, the selector bytes one pass over the inputs
reads -- what the loop reads `tables` times and the new call is meant to read once -- and their time at 8 TB/s.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="loop,new")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes loop)")
ap.add_argument("--sets", default="1024,3,10,13:2048,1,23,16:2048,4,9,12", help="N,l,Bg_bit,size[:...]")
ap.add_argument("--tables", default="1,4,8")
ap.add_argument("--counts", default="1,128,1024")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
modes = args.modes.split(",")

for spec in args.sets.split(":"):
    N, l, Bg, size = (int(x) for x in spec.split(","))
    log_N = N.bit_length() - 1
    n_luts = max(1, (1 << size) >> log_N)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    all_tables = [int(t) for t in args.tables.split(",")]
    luts = torch.randint(-2 ** 63, 2 ** 63 - 1, (max(all_tables), n_luts, 2, N), dtype=torch.int64, device=eng.device, generator=gen)
    for count in (int(c) for c in args.counts.split(",")):
        sel = eng.trgsw_to_dft(torch.randint(-2 ** 63, 2 ** 63 - 1, (count, size, 2 * l, 2, N), dtype=torch.int64, device=eng.device, generator=gen))
        sel_bytes = count * size * 2 * l * 2 * (N // 2) * 16
        for tables in all_tables:
            out = eng.empty(count, tables, N + 1)
            one = eng.empty(tables, count, N + 1)
            tabs = luts[:tables].contiguous()
            for mode in modes:
                group = int(mode.split(":")[1]) if ":" in mode else 0
                if mode == "loop":
                    def run():
                        for tb in range(tables):
                            eng.leveled_lut(sel, tabs[tb], size, l, Bg, out=one[tb])
                    what = "loop"
                else:
                    engine.set_leveled_lut_tables_group(group)
                    what = "new, G = %d" % eng.leveled_lut_tables_plan(N, l, size, tables, count)["group"]

                    def run():
                        eng.leveled_lut_tables(sel, tabs, size, l, Bg, out=out)
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
                print("%-12s N=%d l=%d Bg=2^%d size=%d tables=%d count=%-5d ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats); per (input, table) "
                      "%.2f us; selectors of one pass %.1f MB = %.3f ms at 8 TB/s" % (what, N, l, Bg, size, tables, count, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms),
                                                                                     1e3 * med / (count * tables), sel_bytes / 1e6, sel_bytes / 8e9), flush=True)
                if mode != "loop":
                    engine.set_leveled_lut_tables_group(0)
            del out, one
        del sel
