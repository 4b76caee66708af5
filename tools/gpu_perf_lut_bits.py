"""Function evaluation on LWE-encrypted bits: time per call of Engine.lut_bits (mosfhet_hip_lut_bits_batch) against the four-call composition it replaces --
circuit_bootstrap_3 -> trgsw_to_dft -> leveled_lut_tables -> tlwe_keyswitch on one stream, which tests/test_lut_bits.py shows to give the same words.

    python tools/gpu_perf_lut_bits.py [--modes four,new] [--lib PATH] [--shapes 8,8,128:8,8,1024:12,4,128] [--repeats 7] [--order reference]

--modes: what to time, per shape one after the other (so that the modes of one shape alternate within one process):
    four     the four calls -- only entry points of the parent commit, so the yardstick can be taken on a library built from it: --lib names it
    new      lut_bits with the output key
--shapes: size,tables,count[:...] at lvl2's ring and gadget (N = 2048, l = 4, Bg = 2^9, n = 632) with BASELINE.json configs[3]'s key shapes: packing key t = 6,
base_bit = 4 generated on the device and seed-compressed, private key t = 20, base_bit = 2, the lvl2 set's LWE key switch.  Key CONTENTS that do not change the
time (bootstrap key, private key, ciphertexts, tables) are random words.
hipEvent time around one whole call after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.  Also prints,
per shape, the bytes held between the stages: the composition's torus-domain TRGSWs and selectors of the whole batch against the new call's selectors of one chunk
(mosfhet_hip_lut_bits_plan) and one staging block of the packing switch.
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
ap.add_argument("--modes", default="four,new")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes four)")
ap.add_argument("--shapes", default="8,8,128:8,8,1024:12,4,128", help="size,tables,count[:...]")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--order", default="reference")
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
P = dict(ma.PARAMS_LVL2)
N, l, Bg, n = P["N"], P["l"], P["Bg_bit"], P["n"]
rng = np.random.default_rng(1)
key = eng.load_bootstrap_key(rng.integers(0, 2 ** 64, size=(n, 2 * l, 2, N), dtype=np.uint64), 1, l, Bg)
key.set_product_order(args.order)
kska = eng.load_trlwe_ks_keys(rng.integers(0, 2 ** 64, size=(2, 20, 2, N), dtype=np.uint64), 2)
s_ring, s_lwe = rng.integers(0, 2, size=N, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
pk = eng.generate_table_key(0, s_ring, s_ring, 6, 4, P["rlwe_sigma"], seed=99, compressed=True)
ksk = eng.generate_keyswitch_key(s_lwe, s_ring, P["t"], P["base_bit"], P["lwe_sigma"], seed=7)
gen = torch.Generator(device=eng.device).manual_seed(1)


def rand(*shape):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device=eng.device, generator=gen)


for spec in args.shapes.split(":"):
    size, tables, count = (int(x) for x in spec.split(","))
    bits = count * size
    n_luts = max(1, (1 << size) >> (N.bit_length() - 1))
    luts, cts = rand(tables, n_luts, 2, N), rand(count, size, n + 1)
    out = eng.empty(count, tables, n + 1)
    trgsw_bytes = bits * 2 * l * 2 * N * 8
    together = ((l * bits + 511) // 512) < l * ((bits + 511) // 512)
    for mode in args.modes.split(","):
        if mode == "four":
            trgsw = eng.empty(bits, 2 * l, 2, N)
            lut_out = eng.empty(count, tables, N + 1)

            def run():
                eng.circuit_bootstrap_3(key, kska, pk, cts.view(bits, n + 1), out=trgsw)
                sel = eng.trgsw_to_dft(trgsw).view(count, size, 2 * l, 2, N)
                eng.leveled_lut_tables(sel, luts, size, l, Bg, out=lut_out)
                eng.tlwe_keyswitch(ksk, lut_out.view(count * tables, N + 1), out=out.view(count * tables, n + 1))
            held = "holds %.1f MiB of torus TRGSWs + %.1f MiB of selectors" % (trgsw_bytes / 2 ** 20, trgsw_bytes / 2 ** 20)
        else:
            p = eng.lut_bits_plan(N, l, size, tables, count)
            stage = (l if ((l * p["cb_bits"] + 511) // 512) < l * ((p["cb_bits"] + 511) // 512) else 1) * p["cb_bits"] * 2 * N * 8
            held = "holds %.1f MiB of selectors (%d chunk(s) of %d inputs) + %.1f MiB of staging" % (p["selector_bytes"] / 2 ** 20, p["chunks"], p["chunk"], stage / 2 ** 20)

            def run():
                eng.lut_bits(key, kska, pk, luts, cts, ksk_out=ksk, out=out)
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
        print("%-5s size=%d tables=%d count=%-5d (%d bits, levels %s) ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats); per bit %.2f us; %s" % (
            mode, size, tables, count, bits, "together" if together else "one by one", med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), 1e3 * med / bits, held), flush=True)
        if mode == "four":
            del trgsw, lut_out
        torch.cuda.synchronize()
    del luts, cts, out
