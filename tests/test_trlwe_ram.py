"""Encrypted memory: cells = 2^size TRLWE samples per batch element, read and written at an address given bit by bit as TRGSW_DFT selectors (include/mosfhet_hip.h:
mosfhet_hip_trlwe_ram_read_batch, mosfhet_hip_trlwe_ram_write_batch, mosfhet_hip_trlwe_ram_plan; lut_cmux_kernel modes 2 and 3 of
mosfhet_amd/csrc/leveled_lut_kernels.h).

The expected words are the restatement of tests/trlwe_ram_reference.py -- oracle.external_product and word arithmetic alone; a write in the CMUX form -- on
oracle.bk_to_dft of the same selector words.  Every device comparison is == on every word; there is no tolerance anywhere.  The decryption bound 2^(64 - prec - 1)
is a condition on the INPUTS, which the restatement alone meets on the CPU (test_restatement_decrypts prints the slack); it is no tolerance on the GPU side.
"""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import trlwe_ram_reference as ref
from test_leveled_lut import _map
from test_leveled_lut_edges import _target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
_CACHE = {}

# (N, l, Bg_bit): sigma of fresh samples
SIGMA = {(1024, 3, 10): 2.0 ** -44, (2048, 4, 9): 2.0 ** -44, (1024, 2, 8): 2.0 ** -25, (2048, 1, 23): 2.0 ** -52, (1024, 1, 23): 2.0 ** -52}
# the four gadgets of the noise table: (N, l, Bg_bit, size, prec, writes)
NOISE_SETS = {"N1024 l3 Bg10": (1024, 3, 10, 3, 4, 4), "N2048 l4 Bg9": (2048, 4, 9, 2, 4, 4), "N1024 l2 Bg8": (1024, 2, 8, 2, 2, 2), "N2048 l1 Bg23": (2048, 1, 23, 2, 4, 2)}
# parity: (N, l, Bg_bit, size, count)
WRITE_MAX_SIZE = 10      # the restatement of a write of 2^10 cells x 10 products at N = 1024, l = 2 takes seconds on the CPU (test_restatement_forms_agree prints it)
PARITY = {"N1024 l2 Bg8 size 1 x 1": (1024, 2, 8, 1, 1), "N1024 l2 Bg8 size 2 x 2": (1024, 2, 8, 2, 2), "N1024 l2 Bg8 size 3 x 5": (1024, 2, 8, 3, 5),
          "N1024 l2 Bg8 size 10 x 1": (1024, 2, 8, 10, 1), "N1024 l1 Bg23 size 6 x 7": (1024, 1, 23, 6, 7), "N1024 l3 Bg10 size 2 x 2": (1024, 3, 10, 2, 2),
          "N2048 l4 Bg9 size 2 x 2": (2048, 4, 9, 2, 2), "N2048 l1 Bg23 size 2 x 2": (2048, 1, 23, 2, 2)}


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _addresses(size, count, rng):
    """0, cells - 1 and a middle value first (a batch of one: the middle value at size > 1, cells - 1 at size 1), then random ones"""
    cells = 1 << size
    first = [0, cells - 1, cells // 2 - 1 if size > 1 else 0]
    if count == 1:
        first = [cells // 3 if size > 1 else 1]
    return (first + [int(rng.integers(0, cells)) for _ in range(count)])[:count]


def _selectors(oracle, r, s, addr, size, l, Bg, sigma):
    """[len(addr)][size][2l][2][N] torus words: selector j of input b encrypts bit j of addr[b]"""
    return np.stack([np.stack([oracle.trgsw_monomial_sample(r, (a >> j) & 1, 0, s, l, Bg, sigma) for j in range(size)]) for a in addr])


def _dfts(oracle, sel, l):
    return _map(lambda b: oracle.bk_to_dft(sel[b], 1, l), range(len(sel)))


def _want_read(oracle, mem, dft, l, Bg):
    return np.stack(_map(lambda b: ref.read(oracle, mem[b], dft[b], l, Bg), range(len(mem))))


def _want_write(oracle, mem, val, dft, l, Bg):
    count, cells = mem.shape[:2]
    out = _map(lambda u: ref.write_cell(oracle, mem[u // cells, u % cells], val[u // cells], dft[u // cells], u % cells, l, Bg), range(count * cells))
    return np.stack(out).reshape(mem.shape)


def _parity_case(oracle, name):
    """memories and values of random words; the selectors of the even inputs fresh encryptions of the address bits, of the odd inputs random words; the
    restatement's words of a read and of a write (cached: the tests of one run share them)"""
    if name in _CACHE:
        return _CACHE[name]
    N, l, Bg, size, count = PARITY[name]
    oracle.plan(N)
    seed = 0x4A3 + 131 * size + 7 * count + N + l
    r, rng = oracle.Rng(seed), np.random.default_rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    addr = _addresses(size, count, rng)
    sel = _selectors(oracle, r, s, addr, size, l, Bg, SIGMA[(N, l, Bg)])
    sel[1::2] = rng.integers(0, 2 ** 64, size=sel[1::2].shape, dtype=U64)
    mem = rng.integers(0, 2 ** 64, size=(count, 1 << size, 2, N), dtype=U64)
    val = rng.integers(0, 2 ** 64, size=(count, 2, N), dtype=U64)
    dft = _dfts(oracle, sel, l)
    S = dict(N=N, l=l, Bg=Bg, size=size, count=count, addr=addr, sel=sel, mem=mem, val=val, dft=dft, read=_want_read(oracle, mem, dft, l, Bg))
    wsize = min(size, WRITE_MAX_SIZE)
    S["wsize"] = wsize      # (a write of fewer address bits works on the first 2^wsize cells with the first wsize selectors)
    S["write"] = _want_write(oracle, mem[:, :1 << wsize], val, [d[:wsize] for d in dft], l, Bg)
    _CACHE[name] = S
    return S


def _noise_case(oracle, name):
    """a key, a memory of fresh samples of prec-bit messages on every coefficient per set of the noise table, `writes` writes at random addresses and a read, all by
    the restatement: dict(..., msgs0 = the messages [cells][N] of the fresh memory mem0, steps = [(addr, selector words, value words, value message)], mem_after,
    read_addr, read_sel, out)"""
    key = ("noise", name)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg, size, prec, writes = NOISE_SETS[name]
    oracle.plan(N)
    sigma, cells = SIGMA[(N, l, Bg)], 1 << size
    r, rng = oracle.Rng(0x40153 + N + l), np.random.default_rng(0x40153 + N + l)
    s = oracle.gen_binary_key(r, N).reshape(1, N)

    def fresh():
        m = rng.integers(0, 1 << prec, size=N, dtype=U64) << U64(64 - prec)
        return m, oracle.trlwe_sample(r, m.copy(), s, sigma)

    msgs0, mem = map(np.stack, zip(*[fresh() for _ in range(cells)]))
    mem0, steps = mem.copy(), []
    for _ in range(writes):
        a = int(rng.integers(0, cells))
        sel = _selectors(oracle, r, s, [a], size, l, Bg, sigma)[0]
        vm, val = fresh()
        mem = ref.write(oracle, mem, val, oracle.bk_to_dft(sel, 1, l), l, Bg)
        steps.append((a, sel, val, vm))
    ra = int(rng.integers(0, cells))
    rsel = _selectors(oracle, r, s, [ra], size, l, Bg, sigma)[0]
    out = ref.read(oracle, mem, oracle.bk_to_dft(rsel, 1, l), l, Bg)
    _CACHE[key] = dict(N=N, l=l, Bg=Bg, size=size, prec=prec, s=s, mem0=mem0, msgs0=msgs0, steps=steps, mem_after=mem, read_addr=ra, read_sel=rsel, out=out)
    return _CACHE[key]


def _worst(oracle, S, writes, mem, out):
    """(worst distance of a cell's phase from its message, of the read's phase from the message of the cell it addresses) after the case's first `writes` writes"""
    msgs = S["msgs0"].copy()
    for a, _, _, vm in S["steps"][:writes]:
        msgs[a] = vm
    cell = max(float(oracle.torus_dist(oracle.trlwe_phase(mem[i], S["s"]), msgs[i]).max()) for i in range(len(mem)))
    return cell, float(oracle.torus_dist(oracle.trlwe_phase(out, S["s"]), msgs[S["read_addr"]]).max())


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(NOISE_SETS))
def test_restatement_forms_agree(oracle, name):
    """At the four gadgets of the noise table, on random words: the one-buffer form of a write (e = v - cell; bit 1: e = sel (.) e, bit 0: e = e + sel (.) (-e);
    cell + e) gives the words of the CMUX form on every cell, and a read at size 1 is one oracle CMUX."""
    N, l, Bg, size, _, _ = NOISE_SETS[name]
    oracle.plan(N)
    rng = np.random.default_rng(N + l)
    r = oracle.Rng(N + l)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    sel = _selectors(oracle, r, s, [1, 2], size, l, Bg, SIGMA[(N, l, Bg)])
    sel[1] = rng.integers(0, 2 ** 64, size=sel[1].shape, dtype=U64)
    mem = rng.integers(0, 2 ** 64, size=(1 << size, 2, N), dtype=U64)
    val = rng.integers(0, 2 ** 64, size=(2, N), dtype=U64)
    for b in range(2):
        dft = oracle.bk_to_dft(sel[b], 1, l)
        t0 = time.time()
        a = ref.write(oracle, mem, val, dft, l, Bg)
        dt = time.time() - t0
        assert (a == ref.write(oracle, mem, val, dft, l, Bg, cell_fn=ref.write_cell_e)).all(), (name, b)
        one = ref.read(oracle, mem[:2], dft[:1], l, Bg)
        assert (one == mem[0] + oracle.external_product(mem[1] - mem[0], dft[0], l, Bg)).all()
        assert (one == ref.cmux(oracle, dft[0], mem[0], mem[1], l, Bg)).all()
    print("%s: %.0f us per external product of the restatement" % (name, 1e6 * dt / (size << size)))


@pytest.mark.parametrize("name", list(NOISE_SETS))
def test_restatement_decrypts(oracle, name):
    """The condition on the inputs, on the restatement alone: after the writes at random addresses every cell, and a read at a random address, is within half a slot
    2^(64 - prec - 1) of the expected message on every coefficient."""
    S = _noise_case(oracle, name)
    cell, read = _worst(oracle, S, len(S["steps"]), S["mem_after"], S["out"])
    bound = 64 - S["prec"] - 1
    print("%s, size %d, %d writes: worst cell 2^%.1f, read 2^%.1f, bound 2^%d" % (name, S["size"], len(S["steps"]), _log2(cell), _log2(read), bound))
    assert cell < 2.0 ** bound and read < 2.0 ** bound, (name, _log2(cell), _log2(read))


def test_ram_symbols_and_argument_checks(native_lib):
    """The library exports the entry points and the host layer's two; every refusal is MOSFHET_HIP_EINVAL with a message naming the argument, on fake pointers that
    are never dereferenced -- before any HIP call (this runs without a GPU)."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_trlwe_ram_read_batch", "mosfhet_hip_trlwe_ram_write_batch", "mosfhet_hip_trlwe_ram_plan", "mosfhet_trlwe_ram_read", "mosfhet_trlwe_ram_write"):
        assert hasattr(native_lib, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake, sel, mem = C.c_void_p(1 << 40), C.c_void_p(1 << 41), C.c_void_p(1 << 42)
    top = engine.LEVELED_LUT_MAX_LEVELS
    row = 2 * 1024 * 8
    for fn, other in ((native_lib.mosfhet_hip_trlwe_ram_read_batch, "d_out"), (native_lib.mosfhet_hip_trlwe_ram_write_batch, "d_val")):
        fn.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]
        # the read takes (ctx, d_out, sel, d_mem, ...), the write (ctx, d_mem, sel, d_val, ...)
        f = (lambda ctx, o, s_, m, *a, _fn=fn: _fn(ctx, o, s_, m, *a)) if other == "d_out" else (lambda ctx, o, s_, m, *a, _fn=fn: _fn(ctx, m, s_, o, *a))
        assert f(None, fake, sel, mem, 2, 1024, 2, 8, 4, None) == -1 and "ctx" in err()
        assert f(fake, None, sel, mem, 2, 1024, 2, 8, 4, None) == -1 and other in err()
        assert f(fake, fake, None, mem, 2, 1024, 2, 8, 4, None) == -1 and "d_sel_dft" in err()
        assert f(fake, fake, sel, None, 2, 1024, 2, 8, 4, None) == -1 and "d_mem" in err()
        assert f(fake, fake, sel, mem, 0, 1024, 2, 8, 4, None) == -1 and "size = 0" in err()
        assert f(fake, fake, sel, mem, top + 1, 1024, 2, 8, 4, None) == -1 and "size = %d" % (top + 1) in err()
        assert f(fake, fake, sel, mem, 2, 512, 2, 8, 4, None) == -1 and "N = 512" in err()
        assert f(fake, fake, sel, mem, 2, 4096, 2, 8, 4, None) == -1 and "N = 4096" in err()
        assert f(fake, fake, sel, mem, 2, 1024, 4, 16, 4, None) == -1 and "l=4 Bg_bit=16" in err()
        assert f(fake, fake, sel, mem, 2, 1024, 7, 8, 4, None) == -1 and "l = 7" in err()
        assert f(fake, fake, sel, mem, 2, 1024, 2, 32, 4, None) == -1 and "Bg_bit=32" in err()
        assert f(fake, fake, sel, mem, 2, 1024, 2, 8, -1, None) == -1 and "count = -1" in err()
        # overlap as address ranges: the memory of 4 inputs of 4 cells is 16 rows from `mem`; the other buffer 4 rows
        m0 = mem.value
        for o in (m0, m0 + 15 * row, m0 + 16 * row - 8, m0 - 4 * row + 8, m0 + 8):
            assert f(fake, C.c_void_p(o), sel, mem, 2, 1024, 2, 8, 4, None) == -1 and "overlaps d_mem" in err(), hex(o)
        # count = 0 does nothing and says OK, whatever the pointers
        assert f(fake, None, None, None, 2, 1024, 2, 8, 0, None) == 0
    # a workspace bound below one input's intermediates: refused (the read; a write has no workspace)
    rd = native_lib.mosfhet_hip_trlwe_ram_read_batch
    try:
        engine.set_leveled_lut_workspace(2 * row - 8)
        assert rd(fake, fake, sel, mem, 2, 1024, 2, 8, 4, None) == -1 and "workspace bound" in err()
    finally:
        engine.set_leveled_lut_workspace(0)
    plan = (C.c_longlong * 5)()
    assert native_lib.mosfhet_hip_trlwe_ram_plan(1024, 2, 2, 4, 0, 256, None) == -1 and "plan" in err()
    assert native_lib.mosfhet_hip_trlwe_ram_plan(4096, 1, 2, 4, 0, 256, plan) == -1 and "N = 4096" in err()
    assert native_lib.mosfhet_hip_trlwe_ram_plan(1024, 2, 2, 0, 0, 256, plan) == -1 and "count = 0" in err()
    assert native_lib.mosfhet_hip_trlwe_ram_plan(1024, 2, 2, 4, 0, 0, plan) == -1 and "cus = 0" in err()
    assert native_lib.mosfhet_hip_trlwe_ram_plan(1024, 2, top + 1, 4, 1, 256, plan) == -1 and "size = %d" % (top + 1) in err()


def test_ram_plan_sweep(native_lib):
    """mosfhet_hip_trlwe_ram_plan -- the function the launchers decide with -- over both rings, every size, small and large batches, a device of 256 and of 64 CUs:
    the formulas of the header; chunks of whole inputs as large as the bound allows; a lowered bound gives more chunks and never a larger workspace; a bound below
    one input is refused."""
    from mosfhet_amd import engine
    GiB = 1 << 30
    for cus in (256, 64):
        for N in (1024, 2048):
            for l in (1, 4):
                for size in range(1, engine.LEVELED_LUT_MAX_LEVELS + 1):
                    cells = 1 << size
                    per_input = cells // 2 * 2 * N * 8 if size > 1 else 0
                    for count in (1, 3, 257, 4096):
                        w = engine.trlwe_ram_plan(N, l, size, count, True, cus)
                        assert w == dict(cells=cells, launches=1, chunk=count, workspace_bytes=0, products=count * cells * size), (cus, N, l, size, count, w)
                        p = engine.trlwe_ram_plan(N, l, size, count, False, cus)
                        what = (cus, N, l, size, count, p)
                        assert p["cells"] == cells and p["products"] == count * (cells - 1), what
                        assert 1 <= p["chunk"] <= count, what
                        assert p["launches"] == size * -(-count // p["chunk"]), what
                        assert p["workspace_bytes"] == p["chunk"] * per_input and p["workspace_bytes"] <= GiB, what
                        assert p["chunk"] == count or (p["chunk"] + 1) * per_input > GiB, what      # as large as the bound allows
                        assert p == engine.trlwe_ram_plan(N, l, size, count, False, 256), what     # the CU count sizes grids only
    per_input = 4 * 2 * 1024 * 8
    try:
        p0 = engine.trlwe_ram_plan(1024, 2, 3, 5)
        assert p0 == dict(cells=8, launches=3, chunk=5, workspace_bytes=5 * per_input, products=35)
        engine.set_leveled_lut_workspace(2 * per_input + 8)
        assert engine.trlwe_ram_plan(1024, 2, 3, 5) == dict(cells=8, launches=9, chunk=2, workspace_bytes=2 * per_input, products=35)
        engine.set_leveled_lut_workspace(per_input)
        assert engine.trlwe_ram_plan(1024, 2, 3, 5) == dict(cells=8, launches=15, chunk=1, workspace_bytes=per_input, products=35)
        engine.set_leveled_lut_workspace(per_input - 8)                   # not even one input: refused, not overrun
        with pytest.raises(engine.MosfhetHipError, match="workspace bound"):
            engine.trlwe_ram_plan(1024, 2, 3, 5)
        assert engine.trlwe_ram_plan(1024, 2, 1, 5)["workspace_bytes"] == 0          # one level: no workspace, no refusal
        assert engine.trlwe_ram_plan(1024, 2, 3, 5, True)["workspace_bytes"] == 0    # a write neither
    finally:
        engine.set_leveled_lut_workspace(0)
    assert engine.trlwe_ram_plan(1024, 2, 3, 5) == p0
    for bad in (0, engine.LEVELED_LUT_MAX_LEVELS + 1):
        with pytest.raises(engine.MosfhetHipError, match="size"):
            engine.trlwe_ram_plan(1024, 2, bad, 1)


def test_ram_kernels_of_the_build(native_lib):
    """The new modes live in lut_cmux_kernel: it is still one instantiation per ring with at most 256 registers, 64 KiB of static LDS and no scratch; the library
    holds exactly 329 kernels; tools/check_lds_barriers.py lists the form that compiles the kernel with the memory modes and finds nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    import kernel_table
    forms = [f for f in chk.FORMS if "memory modes" in f[0]]
    assert forms, [f[0] for f in chk.FORMS]
    assert chk.build_and_check(forms) == []
    rows = kernel_table.table()
    mine = [r for r in rows if r["name"].startswith("lut_cmux_kernel")]
    assert sorted(r["name"].replace("> >", ">>") for r in mine) == ["lut_cmux_kernel<Fft1024>", "lut_cmux_kernel<Fft2048T<false, false>>"], [r["name"] for r in mine]
    for r in mine:
        print("%-50s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
        assert r["vgpr"] <= 256 and r["lds"] <= 64 * 1024 and r["scratch"] == 0, r
    assert len(rows) == 329, len(rows)


def test_ram_c_program_compiles(native_lib, tmp_path):
    """tests/c/trlwe_ram.c compiles with -Wall -Werror against include/mosfhet.h and links with the library (it runs in the GPU tests)."""
    _compile_c(str(tmp_path / "trlwe_ram"))


def _compile_c(exe):
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_ram.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _dev_sel(eng, sel):
    """[count][size][2l][2][N] torus words -> the same shape in the DFT domain, on the device"""
    import mosfhet_amd as ma
    return eng.trgsw_to_dft(ma.to_device(sel, eng.device))


def _read(eng, S, sel, mem, size=None):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.trlwe_ram_read(sel, ma.to_device(mem, eng.device), size or S["size"], S["l"], S["Bg"]))


def _write(eng, S, sel, mem, val, size=None):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.trlwe_ram_write(sel, ma.to_device(mem, eng.device), ma.to_device(val, eng.device), size or S["size"], S["l"], S["Bg"]))


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1, 2, got.shape[-1]), want.reshape(-1, 2, want.shape[-1])
    bad = [u for u in range(len(w)) if not (g[u] == w[u]).all()]
    assert not bad, "%s: %d of %d samples differ from the restatement (first: %s)" % (what, len(bad), len(w), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_ram_matches_the_restatement(eng, oracle, name):
    """Parity: a read and a write of every shape -- one level straight to the output, several levels through the workspace, the largest size, more units than
    resident workgroups, both rings, four gadgets; addresses 0, cells - 1 and a middle one; fresh selectors and random selector words -- equal the restatement on
    every word; the read leaves the memory as it was."""
    import mosfhet_amd as ma
    S = _parity_case(oracle, name)
    sel = _dev_sel(eng, S["sel"])
    d_mem = ma.to_device(S["mem"], eng.device)
    got = ma.to_numpy(eng.trlwe_ram_read(sel, d_mem, S["size"], S["l"], S["Bg"]))
    _assert_rows(got, S["read"], name + ", read")
    assert (ma.to_numpy(d_mem) == S["mem"]).all(), "the read changed the memory"
    ws = S["wsize"]
    got = _write(eng, S, sel[:, :ws].contiguous(), S["mem"][:, :1 << ws], S["val"], ws)
    _assert_rows(got, S["write"], name + ", write")


def _edge_inputs(N, l, Bg, seed):
    """size 2, 6 inputs.  Words of {0, 1, 2^63 - 1, 2^63, 2^64 - 1} in memory, value and selector rows (inputs 0 .. 3: every row word one value / alternating / drawn
    from the set / zero); inputs 4 and 5 planted so that the first product of every path decomposes a polynomial whose digits are all at one end of every level
    (tests/test_leveled_lut_edges.py: _target): cell 1 (bit 0 set) val - cell = top, cell 0 cell - val = bottom, the read's first level mem[2] - mem[0] alternating
    and mem[3] - mem[1] bottom -- against selector rows of -2^63 and of 2^63 - 1."""
    rng = np.random.default_rng(seed)
    words = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)
    draw = lambda *shape: words[rng.integers(0, 5, size=shape)]
    count, size = 6, 2
    mem, val, sel = draw(count, 4, 2, N), draw(count, 2, N), np.zeros((count, size, 2 * l, 2, N), dtype=U64)
    sel[0] = U64(2 ** 63)
    sel[1] = U64(2 ** 63 - 1)
    sel[1, ..., ::2] = U64(2 ** 63)
    sel[2] = draw(size, 2 * l, 2, N)
    lo, hi = U64(_target(l, Bg, 0)), U64(_target(l, Bg, (1 << Bg) - 1))
    alt = np.full(N, lo, dtype=U64)
    alt[::2] = hi
    for b, word in ((4, 2 ** 63), (5, 2 ** 63 - 1)):
        sel[b] = U64(word)
        val[b] = mem[b, 1] + hi
        mem[b, 0] = val[b] + lo
        mem[b, 2] = mem[b, 0] + alt
        mem[b, 3] = mem[b, 1] + lo
    return mem, val, sel


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 3, 10), (1024, 2, 8), (2048, 4, 9)])
def test_ram_value_edges(eng, oracle, shape):
    """Value edges.  The extreme words and the planted digit extremes of _edge_inputs (the sums reach 2l N 2^(Bg-1) 2^63, past what rounding without the reduction
    mod 1 holds at l = 3, Bg_bit = 10); then selectors summed on the device to a + 2^16 b, beyond what any transform of torus words reaches, against the
    restatement on the device's own doubles copied back.  Read and write, every word."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg = shape
    oracle.plan(N)
    S = dict(N=N, l=l, Bg=Bg, size=2)
    mem, val, sel = _edge_inputs(N, l, Bg, N + l)
    # the planted differences do sit at the ends of every level
    for d, ends in ((val[4] - mem[4, 1], "top"), (mem[4, 0] - val[4], "bottom"), (mem[5, 3] - mem[5, 1], "bottom")):
        for i in range(l):
            digits = oracle.poly_decompose_i(np.ascontiguousarray(d[0]), Bg, l, i).view(np.int64)
            assert (digits == ((1 << (Bg - 1)) - 1 if ends == "top" else -(1 << (Bg - 1)))).all(), (shape, ends, i)
    dft = _dfts(oracle, sel, l)
    d_sel = _dev_sel(eng, sel)
    _assert_rows(_read(eng, S, d_sel, mem), _want_read(oracle, mem, dft, l, Bg), "%s, extreme words, read" % (shape,))
    _assert_rows(_write(eng, S, d_sel, mem, val), _want_write(oracle, mem, val, dft, l, Bg), "%s, extreme words, write" % (shape,))
    rng = np.random.default_rng(N + l + 1)
    a, b = [_dev_sel(eng, rng.integers(0, 2 ** 64, size=(2, 2, 2 * l, 2, N), dtype=U64)) for _ in range(2)]
    big = eng.dft_lincomb(a, b, 2.0 ** 16)
    host = engine.slot_order_to_oracle(big.cpu().numpy().reshape(-1, N), N).reshape(2, 2, 2 * l, 2, N)
    mag = float(np.abs(host).max())
    print("%s: largest |selector double| of a + 2^16 b: 2^%.1f" % (shape, _log2(mag)))
    assert np.isfinite(host).all() and mag > 2.0 ** 78
    dft = [np.ascontiguousarray(host[i]) for i in range(2)]
    _assert_rows(_read(eng, S, big, mem[:2]), _want_read(oracle, mem[:2], dft, l, Bg), "%s, a + 2^16 b, read" % (shape,))
    _assert_rows(_write(eng, S, big, mem[:2], val[:2]), _want_write(oracle, mem[:2], val[:2], dft, l, Bg), "%s, a + 2^16 b, write" % (shape,))


SENTINEL = 0x5EA75EA75EA75EA7


@pytest.mark.gpu
def test_ram_calls_stay_inside_their_buffers(eng, oracle):
    """Run contexts.  Size 3, 5 inputs, the memory and the output each inside a sentinel-filled buffer one input longer at both ends: a write touches nothing
    outside [count][cells][2][N], a read nothing outside [count][2][N] and no memory word; selectors and values are unchanged."""
    import torch
    import mosfhet_amd as ma
    S = _parity_case(oracle, "N1024 l2 Bg8 size 3 x 5")
    N, count, cells = S["N"], S["count"], 8
    sel, val = _dev_sel(eng, S["sel"]), ma.to_device(S["val"], eng.device)
    sel0, val0 = sel.clone(), val.clone()
    mbuf = torch.full((count + 2, cells, 2, N), SENTINEL, dtype=torch.int64, device=eng.device)
    obuf = torch.full((count + 2, 2, N), SENTINEL, dtype=torch.int64, device=eng.device)
    mbuf[1:-1] = ma.to_device(S["mem"], eng.device)
    eng.trlwe_ram_read(sel, mbuf[1:-1], S["size"], S["l"], S["Bg"], out=obuf[1:-1])
    torch.cuda.synchronize(eng.device)
    got, m = ma.to_numpy(obuf), ma.to_numpy(mbuf)
    assert (got[0] == U64(SENTINEL)).all() and (got[-1] == U64(SENTINEL)).all(), "the read wrote outside its output"
    assert (m[0] == U64(SENTINEL)).all() and (m[-1] == U64(SENTINEL)).all() and (m[1:-1] == S["mem"]).all(), "the read wrote to the memory"
    _assert_rows(got[1:-1], S["read"], "read between sentinels")
    eng.trlwe_ram_write(sel, mbuf[1:-1], val, S["size"], S["l"], S["Bg"])
    torch.cuda.synchronize(eng.device)
    m = ma.to_numpy(mbuf)
    assert (m[0] == U64(SENTINEL)).all() and (m[-1] == U64(SENTINEL)).all(), "the write wrote outside the memory"
    _assert_rows(m[1:-1], S["write"], "write between sentinels")
    assert torch.equal(sel, sel0) and torch.equal(val, val0), "a call changed its selectors or values"


@pytest.mark.gpu
def test_ram_words_do_not_depend_on_the_batch(eng, oracle):
    """Run contexts.  Size 3, 5 inputs: a stale pool (the size-6 read of 7 inputs first, in this thread's workspace); one input per chunk equals one chunk; every
    input alone (count = 1) and at every position of the rotated batch gives the words it gives in the batch; count = 0 does nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    L = _parity_case(oracle, "N1024 l1 Bg23 size 6 x 7")
    _assert_rows(_read(eng, L, _dev_sel(eng, L["sel"]), L["mem"]), L["read"], "the larger call in front")
    S = _parity_case(oracle, "N1024 l2 Bg8 size 3 x 5")
    N, l, Bg, size, count = S["N"], S["l"], S["Bg"], S["size"], S["count"]
    sel = _dev_sel(eng, S["sel"])
    _assert_rows(_read(eng, S, sel, S["mem"]), S["read"], "behind the larger call")
    try:
        engine.set_leveled_lut_workspace(4 * 2 * N * 8)
        assert eng.trlwe_ram_plan(N, l, size, count) == dict(cells=8, launches=15, chunk=1, workspace_bytes=4 * 2 * N * 8, products=35)
        _assert_rows(_read(eng, S, sel, S["mem"]), S["read"], "one input per chunk")
        engine.set_leveled_lut_workspace(2 * 4 * 2 * N * 8)
        assert eng.trlwe_ram_plan(N, l, size, count)["chunk"] == 2
        _assert_rows(_read(eng, S, sel, S["mem"]), S["read"], "two inputs per chunk, the last chunk short")
    finally:
        engine.set_leveled_lut_workspace(0)
    for b in range(count):
        one = sel[b:b + 1].contiguous()
        _assert_rows(_read(eng, S, one, S["mem"][b:b + 1]), S["read"][b:b + 1], "input %d alone, read" % b)
        _assert_rows(_write(eng, S, one, S["mem"][b:b + 1], S["val"][b:b + 1]), S["write"][b:b + 1], "input %d alone, write" % b)
    for shift in range(1, count):
        idx = (np.arange(count) + shift) % count
        rs = sel[torch.from_numpy(idx).to(eng.device)].contiguous()
        _assert_rows(_read(eng, S, rs, S["mem"][idx]), S["read"][idx], "rotated by %d, read" % shift)
        _assert_rows(_write(eng, S, rs, S["mem"][idx], S["val"][idx]), S["write"][idx], "rotated by %d, write" % shift)
    empty = torch.empty((0, size, 2 * l, 2, N), dtype=torch.float64, device=eng.device)
    assert tuple(eng.trlwe_ram_read(empty, eng.empty(0, 8, 2, N), size, l, Bg).shape) == (0, 2, N)
    eng.trlwe_ram_write(empty, eng.empty(0, 8, 2, N), eng.empty(0, 2, N), size, l, Bg)


@pytest.mark.gpu
def test_ram_calls_are_captured_in_a_graph(eng, oracle):
    """Run contexts.  A write followed by a read at size 3, captured on one side stream after an eager call of that shape, replayed twice on different inputs copied
    into the captured buffers: each replay == the eager words (which equal the restatement).  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    S = _parity_case(oracle, "N1024 l2 Bg8 size 3 x 5")
    size, l, Bg = S["size"], S["l"], S["Bg"]
    all_sel = _dev_sel(eng, S["sel"])
    halves = [slice(0, 2), slice(2, 4)]
    eager = []
    for h in halves:
        m = ma.to_device(S["mem"][h], eng.device)
        eng.trlwe_ram_write(all_sel[h].contiguous(), m, ma.to_device(S["val"][h], eng.device), size, l, Bg)
        out = eng.trlwe_ram_read(all_sel[h].contiguous(), m, size, l, Bg)
        eager.append((ma.to_numpy(m), ma.to_numpy(out)))
        _assert_rows(eager[-1][0], S["write"][h], "eager write")
    d_sel, d_mem, d_val = all_sel[halves[0]].clone(), ma.to_device(S["mem"][halves[0]], eng.device), ma.to_device(S["val"][halves[0]], eng.device)
    d_out = eng.empty(2, 2, S["N"])
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.trlwe_ram_write(d_sel, d_mem, d_val, size, l, Bg)
        eng.trlwe_ram_read(d_sel, d_mem, size, l, Bg, out=d_out)
    for r in (1, 0):
        d_sel.copy_(all_sel[halves[r]])
        d_mem.copy_(ma.to_device(S["mem"][halves[r]], eng.device))
        d_val.copy_(ma.to_device(S["val"][halves[r]], eng.device))
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_mem) == eager[r][0]).all(), "replay %d: the written memory differs from the plain call" % r
        assert (ma.to_numpy(d_out) == eager[r][1]).all(), "replay %d: the read differs from the plain call" % r
    del g


@pytest.mark.gpu
def test_host_threads_run_ram_calls_on_their_own_streams(eng, oracle):
    """Run contexts.  Two host threads, each on a stream of its own, each five times its own shape (size 3 with 5 inputs, size 6 with 7): every read and write equals
    the restatement.  A read's workspace belongs to the calling thread's pool; one shared between the threads would mix the two shapes' intermediates."""
    import torch
    import mosfhet_amd as ma
    jobs = [_parity_case(oracle, "N1024 l2 Bg8 size 3 x 5"), _parity_case(oracle, "N1024 l1 Bg23 size 6 x 7")]
    dev = [(_dev_sel(eng, S["sel"]), ma.to_device(S["mem"], eng.device), ma.to_device(S["val"], eng.device)) for S in jobs]
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(t):
        try:
            S, (sel, mem, val) = jobs[t], dev[t]
            with torch.cuda.stream(torch.cuda.Stream(device=eng.device)):
                for _ in range(5):
                    got = ma.to_numpy(eng.trlwe_ram_read(sel, mem, S["size"], S["l"], S["Bg"]))
                    m = mem.clone()
                    eng.trlwe_ram_write(sel, m, val, S["size"], S["l"], S["Bg"])
                    bad[t] += int(not (got == S["read"]).all()) + int(not (ma.to_numpy(m) == S["write"]).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad


@pytest.mark.gpu
def test_ram_refuses_overlapping_buffers(eng, oracle):
    """Run contexts.  Real pointers: an output or a value that lies inside the memory, or ends inside it, is refused with a message; the memory is unchanged."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    S = _parity_case(oracle, "N1024 l2 Bg8 size 2 x 2")
    sel = _dev_sel(eng, S["sel"])
    buf = eng.empty(2 + 1, 4, 2, S["N"])
    buf[:2] = ma.to_device(S["mem"], eng.device)
    mem = buf[:2]
    inside, behind = buf[1][:2], buf[2][:2]       # [2][2][N] views: inside the memory, and directly behind it
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_mem"):
        eng.trlwe_ram_read(sel, mem, 2, S["l"], S["Bg"], out=inside)
    with pytest.raises(engine.MosfhetHipError, match="d_val overlaps d_mem"):
        eng.trlwe_ram_write(sel, mem, inside, 2, S["l"], S["Bg"])
    assert (ma.to_numpy(mem) == S["mem"]).all()
    _assert_rows(ma.to_numpy(eng.trlwe_ram_read(sel, mem, 2, S["l"], S["Bg"], out=behind)), S["read"], "an output directly behind the memory")


@pytest.mark.gpu
def test_ram_read_equals_the_existing_routes(eng, oracle):
    """Against the existing route.  A size-1 read equals mosfhet_hip_cmux_batch with that selector as a one-entry key view, at product order "reference"; and with every
    batch element given the same memory, a read equals the tree part of the leveled LUT's oracle composition: the composition of tests/test_leveled_lut.py on the
    table = the memory, with the address selectors in the tree's places, is the rotation and extraction of what the read returns."""
    import mosfhet_amd as ma
    from test_leveled_lut import _composition
    S = _parity_case(oracle, "N1024 l2 Bg8 size 3 x 5")
    N, l, Bg, count = S["N"], S["l"], S["Bg"], S["count"]
    sel = _dev_sel(eng, S["sel"])
    for b in range(count):
        one = sel[b, :1].contiguous()                                   # selector 0 of input b: [1][2l][2][N]
        key = eng.bootstrap_key_view(one, 1, l, Bg)
        key.set_product_order("reference")
        d = ma.to_device(S["mem"][b, :2], eng.device)
        old = ma.to_numpy(eng.cmux(key, 0, d[:1], d[1:2]))[0]
        new = ma.to_numpy(eng.trlwe_ram_read(one[None], d[None], 1, l, Bg))[0]
        key.free()
        assert (old == new).all(), "input %d: a size-1 read differs from cmux on a key view" % b
        assert (new == ref.read(oracle, S["mem"][b, :2], S["dft"][b][:1], l, Bg)).all()
    log_N, size = 10, 2
    rng = np.random.default_rng(7)
    shared = S["mem"][0, :4]
    low = oracle.bk_to_dft(rng.integers(0, 2 ** 64, size=(log_N, 2 * l, 2, N), dtype=U64), 1, l)      # the rotation's selectors: any words
    got = ma.to_numpy(eng.trlwe_ram_read(sel[:, :size].contiguous(), ma.to_device(np.stack([shared] * count), eng.device), size, l, Bg))
    a = np.array([((2 * N - (1 << i)) << (64 - (log_N + 1))) % 2 ** 64 for i in range(log_N)], dtype=U64)
    for b in range(count):
        full = np.concatenate([low, S["dft"][b][:size]])
        want = _composition(oracle, shared, full, N, l, Bg, log_N + size)
        assert (oracle.trlwe_extract_tlwe(oracle.blind_rotate(got[b].copy(), a, full[:log_N], l, Bg), 0) == want).all(), "input %d: the read is not the tree of eval_LUT" % b


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["N2048 l4 Bg9", "N1024 l2 Bg8"])
def test_ram_write_write_read_decrypts(eng, oracle, name):
    """Decryption.  The first two writes of the noise case and a read on the device: the words of the restatement at every step, and every cell and the read within
    2^(64 - prec - 1) of the expected message (test_restatement_decrypts: the restatement alone meets that bound, with more writes)."""
    import mosfhet_amd as ma
    S = _noise_case(oracle, name)
    N, l, Bg, size = S["N"], S["l"], S["Bg"], S["size"]
    d_mem = ma.to_device(S["mem0"][None], eng.device)
    mem = S["mem0"]
    for a, sel, val, _ in S["steps"][:2]:
        eng.trlwe_ram_write(_dev_sel(eng, sel[None]), d_mem, ma.to_device(val[None], eng.device), size, l, Bg)
        mem = ref.write(oracle, mem, val, oracle.bk_to_dft(sel, 1, l), l, Bg)
        assert (ma.to_numpy(d_mem)[0] == mem).all(), "%s: the memory after a write at %d differs from the restatement" % (name, a)
    out = ma.to_numpy(eng.trlwe_ram_read(_dev_sel(eng, S["read_sel"][None]), d_mem, size, l, Bg))[0]
    assert (out == ref.read(oracle, mem, oracle.bk_to_dft(S["read_sel"], 1, l), l, Bg)).all()
    cell, read = _worst(oracle, S, 2, ma.to_numpy(d_mem)[0], out)
    bound = 64 - S["prec"] - 1
    print("%s: two writes and a read on the device: worst cell 2^%.1f, read 2^%.1f, bound 2^%d" % (name, _log2(cell), _log2(read), bound))
    assert cell < 2.0 ** bound and read < 2.0 ** bound, (name, _log2(cell), _log2(read))


@pytest.mark.gpu
def test_ram_with_address_selectors_from_the_circuit_bootstrap(eng, oracle):
    """Decryption chain, plumbing.  The key set-up of tests/test_lut_bits.py at its smallest set (lvl2's ring and gadget, the cheap private and packing keys): the
    address selectors come from mosfhet_hip_circuit_bootstrap_3_dft_batch on LWE-encrypted address bits and go into a write and a read of size 2 with no repacking in
    between.  That set's one-digit packing key leaves selectors too noisy to decrypt anything (tests/test_lut_bits.py compares words on it, too), so the chain is held
    to the words of the restatement on the oracle's circuit bootstrap of the same bits."""
    import mosfhet_amd as ma
    from test_lut_bits import _pipeline
    D = _pipeline(eng, oracle)
    N, l, Bg, size, count = D["N"], D["l"], D["Bg"], 2, 2
    bits = np.stack([np.arange(b * D["size"], b * D["size"] + size) for b in range(count)]).reshape(-1)      # the first two bits of each of the two inputs
    d_cts = D["d_cts"][eng.torch.from_numpy(bits).to(eng.device)].contiguous()
    sel = eng.circuit_bootstrap_3_dft(D["keys"]["reference"], D["kska"], D["pk"], d_cts).reshape(count, size, 2 * l, 2, N)
    dft = [np.ascontiguousarray(D["want_dft1"][bits[b * size:(b + 1) * size]]) for b in range(count)]
    rng = np.random.default_rng(0xCB)
    mem = rng.integers(0, 2 ** 64, size=(count, 4, 2, N), dtype=U64)
    val = rng.integers(0, 2 ** 64, size=(count, 2, N), dtype=U64)
    S = dict(size=size, l=l, Bg=Bg)
    want = _want_write(oracle, mem, val, dft, l, Bg)
    _assert_rows(_write(eng, S, sel, mem, val), want, "write with circuit-bootstrapped selectors")
    _assert_rows(_read(eng, S, sel, want), _want_read(oracle, want, dft, l, Bg), "read with circuit-bootstrapped selectors")


@pytest.mark.gpu
def test_ram_through_the_host_structs(native_lib, tmp_path):
    """tests/c/trlwe_ram.c: mosfhet_trlwe_ram_write then mosfhet_trlwe_ram_read on 3 inputs equal the CMUX chains written against include/mosfhet.h
    (trlwe_sub / trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add) word for word at size 1 and 2, and decrypt."""
    exe = str(tmp_path / "trlwe_ram")
    _compile_c(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_ram ok" in r.stdout, r.stdout[-3000:]
