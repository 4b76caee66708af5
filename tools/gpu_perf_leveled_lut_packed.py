"""Leveled LUT with several outputs packed into one table: time per call of Engine.leveled_lut_packed (mosfhet_hip_leveled_lut_packed_batch) against the same
function as one unpacked one-bit table per output through Engine.leveled_lut_tables -- an entry point of the parent commit, so the yardstick is taken on a library
built from it (--parent-lib).  Also the cost check for what exists (leveled_lut_tables at 8 tables on both builds) and lut_bits_packed against lut_bits.

    python tools/gpu_perf_leveled_lut_packed.py --parent-lib PATH [--what gain,cost,bits] [--counts 128,1024] [--repeats 7] [--timeout 240]

The driver (no GPU work of its own) starts one worker process per (build, visit): parent, new, parent, new -- two processes per build, alternating -- each under
its own `timeout`, and starts nothing after a worker that failed or ran out of time.  A worker times, per shape, one whole call between two hipEvents after a
warm-up call of the same shape, `repeats` times, and prints the times; the driver pools the two visits of a build and prints median, minimum, maximum and spread
(max - min) / median, and per shape the ratio parent / new and whether new < parent's median - parent's spread (gain) or new <= parent's median + parent's spread
(cost).  Selectors, tables, ciphertexts and key contents are random words (timing only); lut_bits uses BASELINE.json configs[3]'s key shapes.

  gain   N,l,Bg_bit,size,pack_log: parent = leveled_lut_tables with 2^pack_log tables, new = leveled_lut_packed with one table
  cost   leveled_lut_tables at 8 tables x 1024 inputs on both builds
  bits   lut_bits (8, 8 tables) on the parent against lut_bits_packed (8, 1 table, pack_log 3) on the new build
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN = "2048,4,9,8,3:1024,3,10,7,3:2048,4,9,12,3:2048,1,23,16,2"
COST = "1024,3,10,13:2048,1,23,16:2048,4,9,12"


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    if args.lib:
        engine.lib_path = lambda: os.path.abspath(args.lib)
    eng = ma.Engine(0)
    stream = torch.cuda.current_stream()
    gen = torch.Generator(device=eng.device).manual_seed(1)

    def rand(*shape):
        return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device=eng.device, generator=gen)

    def timed(run, **tag):
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
        print("RESULT " + json.dumps(dict(tag, ms=ms)), flush=True)

    counts = [int(c) for c in args.counts.split(",")]
    if args.what in ("gain", "cost"):
        for spec in args.shapes.split(":"):
            f = [int(x) for x in spec.split(",")]
            N, l, Bg, size = f[:4]
            p = f[4] if args.what == "gain" else 0
            packed = args.what == "gain" and args.side == "new"
            tables = 1 if packed else (1 << p if args.what == "gain" else 8)
            n_luts = max(1, (1 << (size + (p if packed else 0))) // N)
            luts = rand(tables, n_luts, 2, N)
            for count in ([1024] if args.what == "cost" else counts):
                sel = eng.trgsw_to_dft(rand(count, size, 2 * l, 2, N))
                if packed:
                    out = eng.empty(count, 1, 1 << p, N + 1)
                    timed(lambda: eng.leveled_lut_packed(sel, luts, size, l, Bg, p, out=out), what=args.what, shape=spec, count=count, call="leveled_lut_packed")
                else:
                    out = eng.empty(count, tables, N + 1)
                    timed(lambda: eng.leveled_lut_tables(sel, luts, size, l, Bg, out=out), what=args.what, shape=spec, count=count, call="leveled_lut_tables x %d" % tables)
                del sel, out
    else:
        P = dict(ma.PARAMS_LVL2)
        N, l, Bg, n = P["N"], P["l"], P["Bg_bit"], P["n"]
        rng = np.random.default_rng(1)
        key = eng.load_bootstrap_key(rng.integers(0, 2 ** 64, size=(n, 2 * l, 2, N), dtype=np.uint64), 1, l, Bg)
        key.set_product_order("reference")
        kska = eng.load_trlwe_ks_keys(rng.integers(0, 2 ** 64, size=(2, 20, 2, N), dtype=np.uint64), 2)
        s_ring, s_lwe = rng.integers(0, 2, size=N, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
        pk = eng.generate_table_key(0, s_ring, s_ring, 6, 4, P["rlwe_sigma"], seed=99, compressed=True)
        ksk = eng.generate_keyswitch_key(s_lwe, s_ring, P["t"], P["base_bit"], P["lwe_sigma"], seed=7)
        size, outs, p = 8, 8, 3
        for count in counts:
            cts, out = rand(count, size, n + 1), eng.empty(count, outs, n + 1)
            if args.side == "new":
                luts = rand(1, 1, 2, N)
                q = eng.lut_bits_packed_plan(N, l, size, 1, p, count)
                timed(lambda: eng.lut_bits_packed(key, kska, pk, luts, cts, p, ksk_out=ksk, out=out), what="bits", shape="8,1,3", count=count, call="lut_bits_packed",
                      staging_bytes=q["chunk"] * q["lut"]["outputs"] * (N + 1) * 8, selector_bytes=q["selector_bytes"])
            else:
                luts = rand(outs, 1, 2, N)
                q = eng.lut_bits_plan(N, l, size, outs, count)
                timed(lambda: eng.lut_bits(key, kska, pk, luts, cts, ksk_out=ksk, out=out), what="bits", shape="8,1,3", count=count, call="lut_bits x 8",
                      staging_bytes=q["chunk"] * outs * (N + 1) * 8, selector_bytes=q["selector_bytes"])
            del cts, out, luts
    eng.close()


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return med, ms[0], ms[-1], (ms[-1] - ms[0]) / med


def driver(args):
    libs = dict(parent=os.path.abspath(args.parent_lib), new=None)
    pooled = {}
    for what in args.what.split(","):
        shapes = dict(gain=args.gain, cost=args.cost, bits="-")[what]
        for visit in range(2):
            for side in ("parent", "new"):
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--what", what, "--side", side, "--shapes", shapes,
                       "--counts", args.counts, "--repeats", str(args.repeats)] + (["--lib", libs[side]] if libs[side] else [])
                print("# %s, %s build, visit %d" % (what, side, visit + 1), flush=True)
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for line in r.stdout.splitlines():
                    if line.startswith("RESULT "):
                        d = json.loads(line[7:])
                        pooled.setdefault((d["what"], d["shape"], d["count"]), {}).setdefault(side, dict(d, ms=[]))["ms"] += d["ms"]
                        print("  %-7s %-24s shape %-16s count %-5d ms %s" % (side, d["call"], d["shape"], d["count"], " ".join("%.3f" % x for x in d["ms"])), flush=True)
                if r.returncode:
                    print(r.stdout[-3000:])
                    print("# the worker ended with status %d: nothing more is started" % r.returncode, flush=True)
                    return r.returncode
    print("# pooled over the two visits of a build")
    for (what, shape, count), sides in pooled.items():
        (pm, p0, p1, ps), (nm, n0, n1, ns) = stats(sides["parent"]["ms"]), stats(sides["new"]["ms"])
        verdict = "faster than parent - spread: %s" % (nm < pm * (1 - ps)) if what == "gain" else "within parent + spread: %s" % (nm <= pm * (1 + ps))
        extra = "".join("; %s %s: staging %d bytes, selectors %d bytes" % (s, sides[s]["call"], sides[s]["staging_bytes"], sides[s]["selector_bytes"]) for s in sides
                        if "staging_bytes" in sides[s])
        print("%-4s %-16s count %-5d parent (%s) median %.3f min %.3f max %.3f spread %.1f %% | new (%s) median %.3f min %.3f max %.3f spread %.1f %% | parent / new %.2f; %s%s" % (
            what, shape, count, sides["parent"]["call"], pm, p0, p1, 100 * ps, sides["new"]["call"], nm, n0, n1, 100 * ns, pm / nm, verdict, extra), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libmosfhet_hip.so built from the parent commit")
    ap.add_argument("--what", default="gain,cost,bits")
    ap.add_argument("--gain", default=GAIN, help="N,l,Bg_bit,size,pack_log[:...]")
    ap.add_argument("--cost", default=COST, help="N,l,Bg_bit,size[:...]")
    ap.add_argument("--counts", default="128,1024")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per worker process")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--side", default="new")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--lib")
    a = ap.parse_args()
    if a.worker:
        worker(a)
    else:
        if not a.parent_lib:
            ap.error("--parent-lib is needed: the yardstick is a library built from the parent commit")
        sys.exit(driver(a))
