"""Cleartext-weight linear layers on LWE batches: time per call of Engine.tlwe_linear and Engine.linear_keyswitch_functional_bootstrap
(mosfhet_hip_tlwe_linear_batch, mosfhet_hip_linear_keyswitch_functional_bootstrap_batch).

    python tools/gpu_perf_tlwe_linear.py [--modes gate,fused,alone,ubench] [--lib PATH] [--repeats 7]

--modes, one after the other in one process:
    gate     the yardstick of the fused call: keyswitch_functional_bootstrap of 4096 samples at SET_1 -- an entry point of the parent commit, so it can be
             taken on a library built from it: --lib names it
    fused    a gate level: sparse, fan-in 2, +-1 weights, a constant in the bias, 4096 outputs of 4096 inputs, one instance, in front of the same key switch and
             bootstrap in ONE call (the linear part moves 3 x 4096 samples of 1025 words: about 100 MB)
    alone    the linear call by itself at n = 1024: dense 784 -> 128 at count 64 with narrow and with wide weights, the sparse handle of the same full matrix,
             and a 3 x 3 convolution (fan-in 9, 4096 outputs of 4096 inputs) at count 16.  Per shape: time, multiplies per second, bytes per second against
             8 TB/s by the plan's byte model (passes over the input + the output; it prices a dense walk, so for a sparse handle it is an upper bound on
             traffic that no memory serves), and the same for every input and output word moved once (what HBM has to serve at least)
    ubench   the two multiply sequences ALONE: tools/ubench/linear_mac.hip (the kernel's own linear_mac<narrow / wide>, the words held in registers, the weights by
             the same scalar loads), built with hipcc if tools/ubench/linear_mac is not there, run as a child process; the yardstick for the multiplies per
             second of the `alone` lines
Key and ciphertext CONTENTS do not change the time: they are random words.  hipEvent time around one whole call after a warm-up call of the same shape; median,
minimum, maximum and spread (max - min) / median over the repeats.  For the method of DESIGN 4.12.5 run the yardstick and the new library in two processes that
alternate.
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
ap.add_argument("--modes", default="gate,fused,alone,ubench")
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: --modes gate)")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
if "ubench" in args.modes.split(","):          # first, in a process of its own, before this one opens the GPU
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ubench")
    exe = os.path.join(here, "linear_mac")
    if not os.path.exists(exe):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, os.path.join(here, "linear_mac.hip")])
    print(subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout, end="", flush=True)
    if args.modes == "ubench":
        sys.exit(0)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
gen = torch.Generator(device=eng.device).manual_seed(1)


def rand(*shape):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device=eng.device, generator=gen)


def timed(what, run, extra=lambda med: ""):
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
    print("%-44s ms per call: median %.4f  min %.4f  max %.4f  spread %.1f %%  (%d repeats)%s" % (what, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med, len(ms), extra(med)),
          flush=True)
    return med


modes = args.modes.split(",")
if "gate" in modes or "fused" in modes:
    P = dict(ma.PARAMS_SET1)
    N, l, Bg, n = P["N"], P["l"], P["Bg_bit"], P["n"]
    bsk = eng.load_bootstrap_key(rng.integers(0, 2 ** 64, size=(n, 2 * l, 2, N), dtype=np.uint64), 1, l, Bg)
    ksk = eng.load_keyswitch_key(rng.integers(0, 2 ** 64, size=(N, P["t"], (1 << P["base_bit"]) - 1, n + 1), dtype=np.uint64), P["base_bit"])
    outputs = 4096
    tv, cts, out = rand(1, 2, N), rand(outputs, N + 1), eng.empty(outputs, N + 1)
    if "gate" in modes:
        timed("gate   keyswitch_functional_bootstrap x %d" % outputs, lambda: eng.keyswitch_functional_bootstrap(ksk, bsk, tv, cts, 4, out=out))
    if "fused" in modes:
        col = rng.integers(0, outputs, size=2 * outputs).astype(np.int32)
        val = rng.choice(np.array([1, -1], dtype=np.int64), size=2 * outputs)
        lin = eng.linear_sparse(np.arange(outputs + 1, dtype=np.int32) * 2, col, val, outputs, bias=rng.integers(0, 2 ** 64, size=outputs, dtype=np.uint64))
        x, y = cts.view(1, outputs, N + 1), eng.empty(1, outputs, N + 1)
        moved = 3 * outputs * (N + 1) * 8
        timed("linear gate level alone (fan-in 2, %d outputs)" % outputs, lambda: eng.tlwe_linear(lin, x, out=y), lambda med: "; %.0f MB moved, %.2f TB/s" % (moved / 1e6, moved / med / 1e9))
        timed("fused  linear + keyswitch + bootstrap x %d" % outputs, lambda: eng.linear_keyswitch_functional_bootstrap(lin, ksk, bsk, tv, x, 4, out=y))
        lin.close()
    del tv, cts, out

if "alone" in modes:
    n = 1024
    w = n + 1

    def report(name, lin, x, out, mults):
        i = lin.info()
        p = engine.tlwe_linear_plan(i["rows_out"], i["rows_in"], n, x.shape[0], nnz=i["nnz"], narrow=i["narrow"])
        model, once = p["input_bytes"] + out.numel() * 8, (x.numel() + out.numel()) * 8
        timed("%s (%s, %s)" % (name, p["form"], p["multiply"]), lambda: eng.tlwe_linear(lin, x, out=out),
              lambda med: "; %.0f G multiplies/s; plan's model %.0f MB -> %.2f TB/s = %.0f %% of 8 TB/s; every word once %.0f MB -> %.2f TB/s = %.0f %% of 8 TB/s" % (
                  mults / med / 1e6, model / 1e6, model / med / 1e9, 100.0 * model / med / 1e9 / 8.0, once / 1e6, once / med / 1e9, 100.0 * once / med / 1e9 / 8.0))

    rows_out, rows_in, count = 128, 784, 64
    x, out = rand(count, rows_in, w), eng.empty(count, rows_out, w)
    narrow = rng.integers(-(1 << 31), 1 << 31, size=(rows_out, rows_in), dtype=np.int64)
    wide = rng.integers(-(1 << 63), (1 << 63) - 1, size=(rows_out, rows_in), dtype=np.int64)
    mults = count * rows_out * rows_in * w
    for tag, W in (("narrow", narrow), ("wide", wide)):
        dense = eng.linear_dense(W)
        report("dense 784 -> 128, count 64", dense, x, out, mults)
        dense.close()
        sparse = eng.linear_sparse(np.arange(rows_out + 1, dtype=np.int32) * rows_in, np.tile(np.arange(rows_in, dtype=np.int32), rows_out), W.reshape(-1), rows_in)
        report("the same full matrix as CSR", sparse, x, out, mults)
        sparse.close()
    del x, out
    side, count = 64, 16                                                      # a 3 x 3 convolution on a 64 x 64 image, wrapping at the edges
    pix = np.arange(side * side).reshape(side, side)
    col = np.stack([np.roll(np.roll(pix, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=-1).reshape(-1).astype(np.int32)
    val = np.tile(rng.integers(-8, 9, size=9).astype(np.int64), side * side)
    conv = eng.linear_sparse(np.arange(side * side + 1, dtype=np.int32) * 9, col, val, side * side)
    x, out = rand(count, side * side, w), eng.empty(count, side * side, w)
    report("3 x 3 convolution, 4096 outputs, count 16", conv, x, out, count * side * side * 9 * w)
    conv.close()
