"""Encrypted automata: time per call of Engine.trlwe_automaton (mosfhet_hip_trlwe_automaton_batch) against the fastest composition of older entry points that gives
the same words -- so the yardstick can be taken on a library built from the parent commit (--lib), where the new call is skipped.

    python tools/gpu_perf_trlwe_automaton.py [--lib PATH] [--shapes 1024,2,8:2048,4,9] [--states 4,16,128] [--steps 16] [--counts 1,64,1024] [--repeats 7]

Yardstick (all launches inside the timed region, every tensor it needs made outside it), per step of the word:
    ram    torch kernels gather the two sources of every (input, state) and rotate them (index_select by next0 / next1, gather by the rotation's index row, times its
           sign row) into [count * states][2][2][N]; then ONE mosfhet_hip_trlwe_ram_read_batch at size 1 over the count * states units with a selector per unit -- the
           step's selector of every input copied once per state beforehand, outside the timed region, as are the index and sign rows of every (layer, state).
hipEvent time around one whole call after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.  Where the
library has the new call the yardstick's words are compared with its (==).  Shapes whose tensors pass the cap below are skipped and named.  Tables, initial vectors
and selectors are random words (timing only); one layer.
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
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: yardstick only)")
ap.add_argument("--shapes", default="1024,2,8:2048,4,9", help="N,l,Bg_bit[:...]")
ap.add_argument("--states", default="4,16,128")
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--counts", default="1,64,1024")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--max-gib", type=float, default=24.0, help="skip a measurement whose tensors pass this many GiB")
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
have_new = hasattr(engine.lib(), "mosfhet_hip_trlwe_automaton_batch")
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
    print("%-12s %s ms per call: median %.3f  min %.3f  max %.3f  spread %.1f %%  (%d repeats)" % (label, shape, med, ms[0], ms[-1], 100.0 * (ms[-1] - ms[0]) / med,
                                                                                                  len(ms)), flush=True)


def rand_words(gen, *shape):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device=eng.device, generator=gen)


def rotation_rows(rot, N):
    """index and sign rows of X^rot: (X^a p)[i] = sign[i] p[index[i]], [states][N] each"""
    i = np.arange(N)[None, :] - (rot[:, None] % N)
    neg = (i < 0) != ((rot[:, None] // N) % 2 == 1)
    return torch.from_numpy(i % N).to(eng.device), torch.from_numpy(np.where(neg, -1, 1).astype(np.int64)).to(eng.device)


steps = args.steps
for spec in args.shapes.split(":"):
    N, l, Bg = (int(x) for x in spec.split(","))
    sel_bytes = 2 * l * 2 * N * 8
    for S in (int(x) for x in args.states.split(",")):
        for count in (int(c) for c in args.counts.split(",")):
            shape = "N=%d l=%d Bg=2^%d states=%-3d steps=%d count=%-5d" % (N, l, Bg, S, steps, count)
            vec_gib = count * S * 2 * N * 8 / GiB
            need = 6 * vec_gib + count * steps * sel_bytes / GiB + count * S * steps * sel_bytes / GiB
            if need > args.max_gib:
                print("skipped      %s (%.1f GiB, of which %.1f of copied selectors)" % (shape, need, count * S * steps * sel_bytes / GiB), flush=True)
                continue
            gen = torch.Generator(device=eng.device).manual_seed(1)
            rng = np.random.default_rng(S)
            tables = [rng.integers(0, S, size=S), rng.integers(0, S, size=S), rng.integers(0, 2 * N, size=S), rng.integers(0, 2 * N, size=S)]
            sel = eng.trgsw_to_dft(rand_words(gen, count, steps, 2 * l, 2, N))
            init = rand_words(gen, count, S, 2, N)
            new_words = None
            if have_new:
                auto = eng.automaton_create(*tables, N)
                out = eng.empty(count, S, 2, N)
                timed("new", shape, lambda: eng.trlwe_automaton(auto, sel, init, l, Bg, out=out))
                new_words = out.clone()
                auto.close()
                del out
            # ---- yardstick "ram": gather + rotate as torch kernels, then a size-1 memory read per step over all (input, state) units
            nxt = [torch.from_numpy(tables[k]).to(eng.device) for k in (0, 1)]
            rows = [rotation_rows(tables[k], N) for k in (2, 3)]
            idx = [r[0].view(1, S, 1, N).expand(count, S, 2, N) for r in rows]
            sign = [r[1].view(1, S, 1, N) for r in rows]
            per_step = [sel[:, t:t + 1].expand(count, S, 2 * l, 2, N).reshape(count * S, 1, 2 * l, 2, N).contiguous() for t in range(steps)]
            res = [None]

            def run_ram():
                V = init
                for t in range(steps - 1, -1, -1):
                    R = [V.index_select(1, nxt[k]).gather(3, idx[k]) * sign[k] for k in (0, 1)]
                    V = eng.trlwe_ram_read(per_step[t], torch.stack(R, dim=2).view(count * S, 2, 2, N), 1, l, Bg).view(count, S, 2, N)
                res[0] = V

            timed("yardstick ram", shape, run_ram)
            if new_words is not None:
                assert torch.equal(res[0], new_words), "yardstick ram: other words than the new call"
            del sel, init, per_step, idx, sign, new_words
            res[0] = None
            torch.cuda.empty_cache()
