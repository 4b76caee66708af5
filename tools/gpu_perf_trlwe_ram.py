"""Encrypted memory: time per call of Engine.trlwe_ram_read / trlwe_ram_write (mosfhet_hip_trlwe_ram_read_batch / _write_batch) against the fastest composition of
older entry points that gives the same words -- so the yardstick can be taken on a library built from the parent commit (--lib), where the new calls are skipped.

    python tools/gpu_perf_trlwe_ram.py [--lib PATH] [--shapes 1024,2,8:2048,4,9] [--sizes 3,6,10] [--counts 1,64,1024] [--repeats 7] [--what read,write]

Yardsticks (all launches inside the timed region, every tensor they need made outside it):
    ep     per address bit ONE mosfhet_hip_external_product_dft_batch over all count x cells (write) or count x half (read) differences with a selector per unit
           -- the bit's selector of every input copied once per unit beforehand, outside the timed region, since the call takes one stride for all units -- then
           mosfhet_hip_dft_to_torus_batch and the word arithmetic as torch kernels: 4 - 5 launches per bit whatever the batch.  A write runs in the one-buffer form
           (e = v - cell), which gives the words of the CMUX form.
    cmux   (read only) per input a key view and one mosfhet_hip_cmux_batch per level at product order "reference": count x size launches.
hipEvent time around one whole call after a warm-up call of the same shape; median, minimum, maximum and spread (max - min) / median over the repeats.  Where the
library has the new calls the words of every yardstick are compared with theirs (==).  Shapes whose memory, copied selectors or product count pass the caps below are
skipped and named.  Memories, values and selectors are random words (timing only).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mosfhet_amd as ma
from mosfhet_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="a libmosfhet_hip.so to load instead of the tree's (the parent commit's build: yardsticks only)")
ap.add_argument("--shapes", default="1024,2,8:2048,4,9", help="N,l,Bg_bit[:...]")
ap.add_argument("--sizes", default="3,6,10")
ap.add_argument("--counts", default="1,64,1024")
ap.add_argument("--what", default="read,write")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--max-gib", type=float, default=24.0, help="skip a measurement whose tensors pass this many GiB")
ap.add_argument("--max-products", type=float, default=2.0 ** 23, help="skip a shape with more external products per call than this")
args = ap.parse_args()
if args.lib:
    engine.lib_path = lambda: os.path.abspath(args.lib)
eng = ma.Engine(0)
stream = torch.cuda.current_stream()
have_new = hasattr(engine.lib(), "mosfhet_hip_trlwe_ram_read_batch")
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


for spec in args.shapes.split(":"):
    N, l, Bg = (int(x) for x in spec.split(","))
    sel_bytes = 2 * l * 2 * N * 8
    for size in (int(x) for x in args.sizes.split(",")):
        cells = 1 << size
        for count in (int(c) for c in args.counts.split(",")):
            for what in args.what.split(","):
                write = what == "write"
                products = count * cells * size if write else count * (cells - 1)
                shape = "%-5s N=%d l=%d Bg=2^%d size=%-2d count=%-5d" % (what, N, l, Bg, size, count)
                mem_gib = count * cells * 2 * N * 8 / GiB
                if products > args.max_products or 2 * mem_gib + count * size * sel_bytes / GiB > args.max_gib:
                    print("skipped      %s (%.0f products, memory %.1f GiB)" % (shape, products, mem_gib), flush=True)
                    continue
                gen = torch.Generator(device=eng.device).manual_seed(1)
                sel = eng.trgsw_to_dft(rand_words(gen, count, size, 2 * l, 2, N))
                mem0 = rand_words(gen, count, cells, 2, N)
                val = rand_words(gen, count, 2, N)
                new_words = None
                if have_new:
                    mem = mem0.clone()
                    if write:
                        timed("new", shape, lambda: eng.trlwe_ram_write(sel, mem, val, size, l, Bg))
                        mem.copy_(mem0)
                        new_words = eng.trlwe_ram_write(sel, mem, val, size, l, Bg).clone()
                    else:
                        out = eng.empty(count, 2, N)
                        timed("new", shape, lambda: eng.trlwe_ram_read(sel, mem, size, l, Bg, out=out))
                        new_words = out.clone()
                    del mem
                # ---- yardstick "ep": one external product call per address bit, a copied selector per unit
                units = [count * cells] * size if write else [count * (cells >> (t + 1)) for t in range(size)]
                if sum(units) * sel_bytes / GiB + 3 * mem_gib > args.max_gib:
                    print("skipped      %s yardstick ep (%.1f GiB of copied selectors)" % (shape, sum(units) * sel_bytes / GiB), flush=True)
                elif write:
                    per_bit = [sel[:, j:j + 1].expand(count, cells, 2 * l, 2, N).reshape(count * cells, 2 * l, 2, N).contiguous() for j in range(size)]
                    idx = torch.arange(cells, device=eng.device)
                    keep = [((idx >> j) & 1).bool().view(1, cells, 1, 1) for j in range(size)]
                    mem = mem0.clone()

                    def run_ep_write():
                        e = val[:, None] - mem
                        for j in range(size):
                            d = torch.where(keep[j], e, -e)
                            r = eng.dft_to_torus(eng.external_product_dft(per_bit[j], d.view(count * cells, 2, N), l, Bg).view(-1, N)).view(count, cells, 2, N)
                            e = torch.where(keep[j], r, e + r)
                        mem.add_(e)

                    timed("yardstick ep", shape, run_ep_write)
                    if new_words is not None:
                        mem.copy_(mem0)
                        run_ep_write()
                        assert torch.equal(mem, new_words), "yardstick ep: other words than the new write"
                    del per_bit, mem
                else:
                    per_level = []
                    for t in range(size):
                        half = cells >> (t + 1)
                        per_level.append(sel[:, size - 1 - t:size - t].expand(count, half, 2 * l, 2, N).reshape(count * half, 2 * l, 2, N).contiguous())
                    res = [None]

                    def run_ep_read():
                        T = mem0
                        for t in range(size):
                            half = cells >> (t + 1)
                            d = (T[:, half:2 * half] - T[:, :half]).contiguous()
                            r = eng.dft_to_torus(eng.external_product_dft(per_level[t], d.view(count * half, 2, N), l, Bg).view(-1, N)).view(count, half, 2, N)
                            T = T[:, :half] + r
                        res[0] = T[:, 0]

                    timed("yardstick ep", shape, run_ep_read)
                    if new_words is not None:
                        assert torch.equal(res[0], new_words), "yardstick ep: other words than the new read"
                    del per_level
                # ---- yardstick "cmux" (read): per input one cmux launch per level on a key view
                if not write and count * size <= 4096:
                    keys = []
                    for b in range(count):
                        keys.append(eng.bootstrap_key_view(sel[b], 1, l, Bg))
                        keys[-1].set_product_order("reference")
                    work = eng.empty(count, max(1, cells // 2), 2, N)

                    def run_cmux_read():
                        for b in range(count):
                            for t in range(size):
                                half = cells >> (t + 1)
                                src = mem0[b] if t == 0 else work[b]
                                eng.cmux(keys[b], size - 1 - t, src[:half], src[half:2 * half], out=work[b, :half])

                    timed("yardstick cmux", shape, run_cmux_read)
                    if new_words is not None:
                        assert torch.equal(work[:, 0], new_words), "yardstick cmux: other words than the new read"
                    for k in keys:
                        k.free()
                    del work
                del sel, mem0, val, new_words
                torch.cuda.empty_cache()
