"""Selector logic: circuits of gates over TRGSW_DFT selectors on the device (include/mosfhet_hip.h: mosfhet_hip_sellogic_create, mosfhet_hip_trgsw_logic_batch,
mosfhet_hip_trgsw_logic_plan; mosfhet_amd/csrc/capi_sellogic.inc, sel_gate_body in trace_kernels.h; include/mosfhet_compat.h: mosfhet_trgsw_logic).

Expected words come from tests/trgsw_logic_reference.py: the contract restated from oracle.dft_to_torus, oracle.external_product and oracle.trgsw_to_dft.  Every device
comparison is == on all doubles against eng.torus_to_dft of the restatement's torus-domain rows, and == on all words between eng.dft_to_torus of the device's selector
and T() of the restatement's wire.  The decryption bound is 2^57: half a slot of four-bit messages in slots of 2^60 less two bits, the bound
tests/test_trace_conversions.py holds the gadget conversion's selectors to."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trgsw_logic_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U64 = np.uint64
_CACHE = {}
GADGETS = [(1024, 2, 8), (2048, 4, 9), (1024, 1, 23), (1024, 6, 7)]
FINE = (2048, 4, 9, 2.0 ** -44)          # the gadget and noise at which a gate's output is usable
BOUND = 2.0 ** 57


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("N,l,Bg_bit", GADGETS)
def test_restatement_against_the_oracle(oracle, N, l, Bg_bit):
    """The restatement itself, on uniform torus words; the code under test plays no part.  AND, row for row, is oracle.external_product of the row of X taken back by
    oracle.dft_to_torus with oracle.trgsw_to_dft(Y) (trgsw_mul_DFT2).  NOT of NOT gives back the words of a sample that survives the double round trip (the trivial
    samples of 0 and 1, whose H - X survives too: both checked).  MUX with Z the trivial sample of 0 gives T(Y) exactly (every digit meets a zero row); with Z the
    trivial sample of 1 it gives T(X) up to the product's rounding: the gadget keeps l Bg_bit bits, so the reconstruction is off by at most 2^(63 - l Bg_bit), and
    the transforms of values below 2^63 sqrt(N) in doubles of 53 bits add at most 2^20 (measured and printed: about 2^12)."""
    oracle.plan(N)
    rng = np.random.default_rng([0x5E1, N, l, Bg_bit])
    xw, yw = rng.integers(0, 2 ** 64, size=(2, 2 * l, 2, N), dtype=U64)
    X, Y = oracle.trgsw_to_dft(xw, 1, l), oracle.trgsw_to_dft(yw, 1, l)
    got = ref.gate_rows(oracle, ref.AND, X, Y, None, l, Bg_bit)
    with oracle.product_order("reference"):
        for r in range(2 * l):
            left = np.stack([oracle.dft_to_torus(np.ascontiguousarray(X[r, c])) for c in range(2)])
            assert (got[r] == oracle.external_product(left, Y, l, Bg_bit)).all(), r
    for mu in (0, 1):
        w = ref.trivial_one(N, l, Bg_bit, mu)
        H = ref.trivial_one(N, l, Bg_bit)
        for words in (w, H - w):
            assert (ref.rows_of(oracle, oracle.trgsw_to_dft(words, 1, l)) == words).all(), "the trivial sample does not survive the round trip"
        rows = ref.circuit_rows(oracle, [(ref.NOT, 0, -1, -1), (ref.NOT, 1, -1, -1)], w[None], l, Bg_bit)
        assert (rows[0] == H - w).all() and (rows[1] == w).all(), mu
    TX, TY = ref.rows_of(oracle, X), ref.rows_of(oracle, Y)
    zero, one = [oracle.trgsw_to_dft(ref.trivial_one(N, l, Bg_bit, mu), 1, l) for mu in (0, 1)]
    assert (ref.gate_rows(oracle, ref.MUX, X, Y, zero, l, Bg_bit) == TY).all()
    d = (ref.gate_rows(oracle, ref.MUX, X, Y, one, l, Bg_bit) - TX).view(np.int64)
    worst = int(np.abs(d).max())
    bound = 2 ** (63 - l * Bg_bit) + 2 ** 20
    print("(%d, %d, %d): MUX(x, y, 1) - T(x): worst 2^%.1f, bound 2^%.1f" % (N, l, Bg_bit, _log2(worst), _log2(bound)))
    assert worst <= bound


def _noise_setup(oracle, N, l, Bg, sigma, seed):
    oracle.plan(N)
    r = oracle.Rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    d, m = ref.probe(oracle, r, s, sigma)
    return r, s, d, m


def _worst_of(oracle, rows, values, wires, d, m, s, l, Bg, n_in):
    return max(ref.selector_error(oracle, rows[w - n_in], values[w - n_in], d, m, s, l, Bg) for w in wires)


def test_gates_decrypt_on_the_restatement(oracle):
    """(2048, 4, 9), sigma 2^-44, fixed seeds, the probe a sample of four-bit messages in slots of 2^60; the figure is the worst phase error of
    oracle.external_product(probe, gate output) against bit x messages.  Every op on all input combinations, the 4-bit incrementer on {0, 5, 7, 15, 11}, the 3-bit
    one-hot demultiplexer on the addresses {0, 3, 6} (all 8 lines) and 6-gate AND and XOR chains with the accumulated wire on the LEFT each stay below 2^57.  The
    code under test plays no part.
    Recorded, with only `> 2^59` asserted so that the header's warning cannot go stale: the chain with the accumulated wire on the RIGHT at depth 2, and one AND at
    (1024, 2, 8) with sigma 2.989e-8 -- both lost."""
    N, l, Bg, sigma = FINE
    r, s, d, m = _noise_setup(oracle, N, l, Bg, sigma, 0x5E110)
    ops2 = (ref.AND, ref.NAND, ref.OR, ref.NOR, ref.XOR, ref.XNOR, ref.ANDNOT)
    gates = [(ref.NOT, 0, -1, -1)] + [(op, 0, 1, -1) for op in ops2] + [(ref.MUX, 0, 1, 2)]
    worst = {}
    for a in range(2):
        for b in range(2):
            for c in range(2):
                rows = ref.circuit_rows(oracle, gates, ref.encrypted_bits(oracle, r, (a, b, c), s, l, Bg, sigma), l, Bg)
                vals = ref.evaluate(gates, (a, b, c))
                for g, gate in enumerate(gates):
                    e = ref.selector_error(oracle, rows[g], vals[g], d, m, s, l, Bg)
                    worst[gate[0]] = max(worst.get(gate[0], 0.0), e)
    names = ("NOT", "AND", "NAND", "OR", "NOR", "XOR", "XNOR", "ANDNOT", "MUX")
    print("one gate, all input combinations: " + ", ".join("%s 2^%.1f" % (names[op], _log2(worst[op])) for op in sorted(worst)))
    assert max(worst.values()) < BOUND, worst
    n_in, inc, sums = ref.incrementer(4)
    w = 0.0
    for v in (0, 5, 7, 15, 11):
        bits = [(v >> i) & 1 for i in range(4)]
        rows = ref.circuit_rows(oracle, inc, ref.encrypted_bits(oracle, r, bits, s, l, Bg, sigma), l, Bg)
        vals = ref.evaluate(inc, bits)
        assert sum(vals[k - n_in] << i for i, k in enumerate(sums)) == (v + 1) % 16
        w = max(w, _worst_of(oracle, rows, vals, range(n_in, n_in + len(inc)), d, m, s, l, Bg, n_in))
    print("4-bit incrementer, sums and carries: 2^%.1f" % _log2(w))
    assert w < BOUND
    n_in, dmx, lines = ref.demultiplexer(3)
    w = 0.0
    for addr in (0, 3, 6):
        bits = [(addr >> i) & 1 for i in range(3)]
        rows = ref.circuit_rows(oracle, dmx, ref.encrypted_bits(oracle, r, bits, s, l, Bg, sigma), l, Bg)
        vals = ref.evaluate(dmx, bits)
        assert [vals[k - n_in] for k in lines] == [int(a == addr) for a in range(8)]
        w = max(w, _worst_of(oracle, rows, vals, lines, d, m, s, l, Bg, n_in))
    print("3-bit one-hot demultiplexer, all 8 lines: 2^%.1f" % _log2(w))
    assert w < BOUND
    for op, bits in ((ref.AND, [1] * 7), (ref.XOR, [1, 0, 1, 1, 0, 1, 1])):
        n_in, ch = ref.chain(op, 6)
        rows = ref.circuit_rows(oracle, ch, ref.encrypted_bits(oracle, r, bits, s, l, Bg, sigma), l, Bg)
        vals = ref.evaluate(ch, bits)
        errs = [ref.selector_error(oracle, rows[g], vals[g], d, m, s, l, Bg) for g in range(6)]
        print("%s chain, accumulated wire on the left, depth 1 .. 6: %s" % (names[op], " ".join("2^%.1f" % _log2(e) for e in errs)))
        assert max(errs) < BOUND
    n_in, ch = ref.chain(ref.AND, 2, accumulated_left=False)
    rows = ref.circuit_rows(oracle, ch, ref.encrypted_bits(oracle, r, [1, 1, 1], s, l, Bg, sigma), l, Bg)
    errs = [ref.selector_error(oracle, rows[g], 1, d, m, s, l, Bg) for g in range(2)]
    print("AND chain, accumulated wire on the RIGHT, depth 1, 2: 2^%.1f 2^%.1f" % (_log2(errs[0]), _log2(errs[1])))
    assert errs[1] > 2.0 ** 59
    r1, s1, d1, m1 = _noise_setup(oracle, 1024, 2, 8, 2.989040792967434e-8, 0x5E111)
    rows = ref.circuit_rows(oracle, [(ref.AND, 0, 1, -1)], ref.encrypted_bits(oracle, r1, [1, 1], s1, 2, 8, 2.989040792967434e-8), 2, 8)
    e = ref.selector_error(oracle, rows[0], 1, d1, m1, s1, 2, 8)
    print("one AND at (1024, 2, 8), sigma 2.989e-8: 2^%.1f" % _log2(e))
    assert e > 2.0 ** 59


def test_sellogic_symbols_and_argument_checks(native_lib):
    """The library exports the entry points and the binding its functions; every refusal returns MOSFHET_HIP_EINVAL with a message naming the argument, on fake
    pointers and without a device: creation (an operand that is not earlier, an unused field that is not -1, op 9, n_in = 0, n_gates = 4097, N = 4096), the batch
    call (null pointers, l Bg_bit = 64, count = -1, overlap), the plan, and the binding's wrong-N refusal; count == 0 does nothing."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_sellogic_create", "mosfhet_hip_sellogic_destroy", "mosfhet_hip_sellogic_info", "mosfhet_hip_trgsw_logic_batch",
                 "mosfhet_hip_trgsw_logic_plan", "mosfhet_trgsw_logic"):
        assert hasattr(native_lib, name), name
    for name in ("sellogic_create", "trgsw_logic_plan", "SelLogic", "SEL_NOT", "SEL_AND", "SEL_NAND", "SEL_OR", "SEL_NOR", "SEL_XOR", "SEL_XNOR", "SEL_ANDNOT", "SEL_MUX"):
        assert hasattr(engine, name), name
    for name in ("sellogic_create", "trgsw_logic", "trgsw_logic_plan"):
        assert hasattr(engine.Engine, name), name
    assert [engine.SEL_NOT, engine.SEL_AND, engine.SEL_NAND, engine.SEL_OR, engine.SEL_NOR, engine.SEL_XOR, engine.SEL_XNOR, engine.SEL_ANDNOT, engine.SEL_MUX] == list(range(9))
    assert engine.SELLOGIC_MAX_WIRES == 4096
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced
    mk = native_lib.mosfhet_hip_sellogic_create
    mk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    out = C.c_void_p()
    ints = lambda rows: (C.c_int * (4 * len(rows)))(*[v for row in rows for v in row])
    one = ints([(1, 0, 1, -1)])
    assert mk(None, one, 1, 2, 1024) == EINVAL and "out" in err()
    assert mk(C.byref(out), None, 1, 2, 1024) == EINVAL and "h_gates" in err()
    assert mk(C.byref(out), one, 1, 2, 4096) == EINVAL and "N = 4096" in err()
    assert mk(C.byref(out), one, 1, 0, 1024) == EINVAL and "n_in = 0" in err()
    assert mk(C.byref(out), one, 1, 4097, 1024) == EINVAL and "n_in = 4097" in err()
    assert mk(C.byref(out), one, 0, 2, 1024) == EINVAL and "n_gates = 0" in err()
    assert mk(C.byref(out), one, 4097, 2, 1024) == EINVAL and "n_gates = 4097" in err()
    assert mk(C.byref(out), ints([(9, 0, 1, -1)]), 1, 2, 1024) == EINVAL and "op = 9" in err()
    assert mk(C.byref(out), ints([(-1, 0, 1, -1)]), 1, 2, 1024) == EINVAL and "op = -1" in err()
    assert mk(C.byref(out), ints([(1, 0, 2, -1)]), 1, 2, 1024) == EINVAL and "gates[0].y = 2" in err()          # its own output
    assert mk(C.byref(out), ints([(1, 0, 1, -1), (5, 2, 4, -1)]), 2, 2, 1024) == EINVAL and "gates[1].y = 4" in err()   # a later wire
    assert mk(C.byref(out), ints([(1, -1, 1, -1)]), 1, 2, 1024) == EINVAL and "gates[0].x = -1" in err()        # a used field left unset
    assert mk(C.byref(out), ints([(1, 0, 1, 0)]), 1, 2, 1024) == EINVAL and "gates[0].z = 0" in err()           # an unused field set
    assert mk(C.byref(out), ints([(0, 0, 0, -1)]), 1, 2, 1024) == EINVAL and "gates[0].y = 0" in err()
    assert mk(C.byref(out), ints([(8, 0, 1, -1)]), 1, 2, 1024) == EINVAL and "gates[0].z = -1" in err()         # MUX uses all three
    assert out.value is None
    assert mk(C.byref(out), ints([(1, 0, 0, -1), (8, 2, 1, 0)]), 2, 2, 1024) == 0 and out.value               # x = y is allowed
    info = (C.c_longlong * 5)()
    gi = native_lib.mosfhet_hip_sellogic_info
    gi.argtypes = [C.c_void_p, C.c_void_p]
    assert gi(out, info) == 0 and list(info) == [1024, 2, 2, 2, 2]
    assert gi(None, info) == EINVAL and "circuit" in err()
    assert gi(out, None) == EINVAL and "info" in err()
    f = native_lib.mosfhet_hip_trgsw_logic_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]
    assert f(None, fake, out, fake, 2, 8, 1, None) == EINVAL and "ctx" in err()
    assert f(fake, fake, None, fake, 2, 8, 1, None) == EINVAL and "circuit" in err()
    assert f(fake, fake, out, fake, 2, 8, -1, None) == EINVAL and "count = -1" in err()
    for l, Bg in ((2, 32), (0, 8), (7, 8), (2, 0), (4, 16), (1, 64)):
        assert f(fake, fake, out, fake, l, Bg, 1, None) == EINVAL and ("gadget" in err() or "l = " in err()), (l, Bg, err())
    assert f(fake, None, out, fake, 2, 8, 1, None) == EINVAL and "d_out_dft" in err()
    assert f(fake, fake, out, None, 2, 8, 1, None) == EINVAL and "d_in_dft" in err()
    sample = 2 * 2 * 2 * 1024 * 8
    base = 1 << 20
    at = lambda off: C.c_void_p(base + off)
    assert f(fake, at(0), out, at(0), 2, 8, 1, None) == EINVAL and "overlaps" in err()
    assert f(fake, at(2 * sample - 8), out, at(0), 2, 8, 1, None) == EINVAL and "overlaps" in err()            # the last word of the inputs
    assert f(fake, at(0), out, at(2 * sample - 8), 2, 8, 1, None) == EINVAL and "overlaps" in err()            # the last word of the outputs
    assert f(fake, fake, out, fake, 2, 8, 0, None) == 0                                                        # count == 0: nothing to do
    assert f(fake, None, out, None, 2, 8, 0, None) == 0
    p = native_lib.mosfhet_hip_trgsw_logic_plan
    p.argtypes = [C.c_int] * 8 + [C.c_void_p]
    plan = (C.c_longlong * 5)()
    assert p(1024, 2, 2, 2, 2, 1, 1, 256, None) == EINVAL and "plan" in err()
    assert p(4096, 2, 2, 2, 2, 1, 1, 256, plan) == EINVAL and "N = 4096" in err()
    assert p(1024, 7, 2, 2, 2, 1, 1, 256, plan) == EINVAL and "l = 7" in err()
    assert p(1024, 2, 0, 2, 2, 1, 1, 256, plan) == EINVAL and "n_in = 0" in err()
    assert p(1024, 2, 2, 4097, 2, 1, 1, 256, plan) == EINVAL and "n_gates = 4097" in err()
    assert p(1024, 2, 2, 2, 3, 1, 1, 256, plan) == EINVAL and "levels = 3" in err()
    assert p(1024, 2, 2, 4, 2, 1, 1, 256, plan) == EINVAL and "widest_level = 1" in err()                     # 4 gates in 2 levels: at least 2 wide
    assert p(1024, 2, 2, 4, 2, 4, 1, 256, plan) == EINVAL and "widest_level = 4" in err()                     # ... and at most 3
    assert p(1024, 2, 2, 2, 2, 1, -1, 256, plan) == EINVAL and "count = -1" in err()
    assert p(1024, 2, 2, 2, 2, 1, 1, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(1024, 2, 2, 2, 2, 1, 0, 256, plan) == 0 and list(plan) == [0, 0, 0, 0, 0]
    assert native_lib.mosfhet_hip_sellogic_destroy(out) == 0
    assert native_lib.mosfhet_hip_sellogic_destroy(None) == 0

    class FakeTensor:            # the binding compares N before anything touches the tensor
        shape = (1, 2, 4, 2, 2048)
    c = engine.sellogic_create([(1, 0, 1, -1)], 2, 1024)
    with pytest.raises(engine.MosfhetHipError, match="made for N = 1024"):
        engine.Engine.trgsw_logic(None, c, FakeTensor(), 2, 8)
    c.close()
    with pytest.raises(engine.MosfhetHipError, match="gates\\[1\\].x = 3"):
        engine.sellogic_create([(1, 0, 1, -1), (0, 3, -1, -1)], 2, 1024)


def test_sellogic_plan_and_levels():
    """mosfhet_hip_trgsw_logic_plan swept: one launch per level while the widest level's teams fit one grid of 2^24 teams, then chunks of whole batch elements
    (launches = levels x chunks, the widest launch = chunk x widest x 2l teams); the plan's work figures are those of n_gates AND gates (count x 2l x n_gates
    products, 4 inverse and 2l + 2 forward transforms each), and a handle's own product count is count x 2l x its product gates: 0 for a NOT-only circuit.  info on a
    hand-made 3-level circuit, and on the circuits of the other tests against the restatement's level rule."""
    from mosfhet_amd import engine
    grid = 1 << 24
    for N, l in ((1024, 2), (2048, 4), (1024, 6), (1024, 1)):
        for n_gates, levels, widest in ((1, 1, 1), (12, 3, 6), (40, 1, 40), (4096, 1, 4096), (4096, 4096, 1), (100, 7, 50)):
            for count in (1, 5, 64, grid // (widest * 2 * l), grid // (widest * 2 * l) + 1, 3 * (grid // (widest * 2 * l)) + 1):
                p = engine.trgsw_logic_plan(N, l, 3, n_gates, levels, widest, count)
                fit = grid // (widest * 2 * l)
                chunk = min(count, fit)
                assert p["launches"] == levels * -(-count // chunk), (N, l, n_gates, levels, widest, count, p)
                assert p["teams"] == chunk * widest * 2 * l and p["teams"] <= grid, p
                rows = count * n_gates * 2 * l
                assert (p["products"], p["inverses"], p["forwards"]) == (rows, 4 * rows, (2 * l + 2) * rows), p
                assert engine.trgsw_logic_plan(N, l, 3, n_gates, levels, widest, count, cus=64) == p
    fit = grid // (4096 * 12)
    assert engine.trgsw_logic_plan(1024, 6, 1, 4096, 1, 4096, fit)["launches"] == 1
    assert engine.trgsw_logic_plan(1024, 6, 1, 4096, 1, 4096, fit + 1) == dict(launches=2, teams=fit * 4096 * 12, products=(fit + 1) * 4096 * 12,
                                                                                   inverses=4 * (fit + 1) * 4096 * 12, forwards=14 * (fit + 1) * 4096 * 12)
    c = engine.sellogic_create([(engine.SEL_NOT, 0, -1, -1), (engine.SEL_AND, 2, 1, -1), (engine.SEL_NOT, 1, -1, -1), (engine.SEL_MUX, 3, 4, 0), (engine.SEL_XOR, 0, 1, -1)], 2, 2048)
    assert c.info() == dict(N=2048, n_in=2, n_gates=5, levels=3, product_gates=3), c.info()
    c.close()
    c = engine.sellogic_create([(engine.SEL_NOT, 0, -1, -1), (engine.SEL_NOT, 1, -1, -1), (engine.SEL_NOT, 0, -1, -1)], 1, 1024)
    assert c.info() == dict(N=1024, n_in=1, n_gates=3, levels=2, product_gates=0), c.info()      # NOT-only: no products
    c.close()
    for n_in, gates in (ref.every_op_circuit(), ref.incrementer(4)[:2], ref.demultiplexer(3)[:2], ref.chain(ref.XOR, 6)):
        c = engine.sellogic_create(gates, n_in, 1024)
        assert c.levels == max(ref.levels_of(gates, n_in)) and c.product_gates == sum(g[0] != ref.NOT for g in gates), c.info()
        c.close()
    assert max(ref.levels_of(ref.every_op_circuit()[1], 3)) == 3 and sorted({g[0] for g in ref.every_op_circuit()[1]}) == list(range(9))


def test_sellogic_kernels_of_the_build(native_lib):
    """The gate is a run-time kind of trace_conversions_kernel: that kernel is still listed once per ring, without scratch; the library holds exactly 329 kernels;
    tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    mine = [r for r in rows if r["name"].startswith("trace_conversions_kernel")]
    for r in mine:
        print("%-60s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    assert len(mine) == 3 and len({r["name"] for r in mine}) == 3, [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0, r
    assert len(rows) == 329, len(rows)
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    print(report)
    assert ", 0 violations" in report, report


def _compile_c(tmp_path):
    exe = str(tmp_path / "trgsw_logic")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trgsw_logic.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sellogic_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trgsw_logic.c compiles with -Wall -Werror against include/mosfhet.h and links against the built library (its device part: test_sellogic_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def _want(oracle, gates, words, l, Bg, in_dft=None):
    """per batch element: the rows before F of every gate and T() of every gate's wire -> ([count][n_gates][2l][2][N], the same shape)"""
    rows = np.stack([ref.circuit_rows(oracle, gates, words[b] if words is not None else None, l, Bg, None if in_dft is None else in_dft[b])
                     for b in range(len(words if words is not None else in_dft))])
    back = np.stack([np.stack([ref.rows_of(oracle, oracle.trgsw_to_dft(np.ascontiguousarray(g), 1, l)) for g in rb]) for rb in rows])
    return rows, back


def _case(oracle, N, l, Bg, count, which="every op"):
    """uniform torus words in the inputs, the restatement's rows and wire words; made once per shape and left unchanged"""
    key = (N, l, Bg, count, which)
    if key not in _CACHE:
        oracle.plan(N)
        n_in, gates = ref.every_op_circuit() if which == "every op" else (3, [(1 + k % 7, k % 3, (k + 1 + k // 3) % 3, -1) for k in range(40)])
        words = np.random.default_rng([0x5E1C, N, l, Bg]).integers(0, 2 ** 64, size=(5, n_in, 2 * l, 2, N), dtype=U64)[:count]
        rows, back = _want(oracle, gates, words, l, Bg)
        _CACHE[key] = dict(N=N, l=l, Bg=Bg, n_in=n_in, gates=gates, words=words, rows=rows, back=back)
    return _CACHE[key]


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _dev(eng, a):
    import mosfhet_amd as ma
    return ma.to_device(a, eng.device)


def _to_dft(eng, words):
    """torus words [...][N] -> the same shape in the DFT domain on the device (F, polynomial by polynomial)"""
    d = _dev(eng, words)
    return eng.torus_to_dft(d.view(-1, d.shape[-1])).view(*d.shape)


def _assert_selectors(eng, got, rows, back, what):
    """got: device doubles [count][n_gates][2l][2][N]; == eng.torus_to_dft(rows) on every double (as bit patterns), and eng.dft_to_torus(got) == back on every word"""
    import mosfhet_amd as ma
    want = _to_dft(eng, rows)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    g, w = got.cpu().numpy().view(U64), want.cpu().numpy().view(U64)
    bad = sorted({(int(b), int(k)) for b, k in zip(*np.nonzero((g != w).any(axis=(2, 3, 4))))})
    assert not bad, "%s: the selectors of %d (batch element, gate) pairs differ from the restatement (first: %s)" % (what, len(bad), bad[:8])
    words = ma.to_numpy(eng.dft_to_torus(got.reshape(-1, got.shape[-1]))).reshape(back.shape)
    assert (words == back).all(), "%s: dft_to_torus of the device's selectors differs from the restatement's wires" % what


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 5])
@pytest.mark.parametrize("N,l,Bg_bit", GADGETS)
def test_logic_matches_the_restatement(eng, oracle, N, l, Bg_bit, count):
    """Parity: n_in = 3, the 12-gate circuit of three levels that uses every op, with a gate whose x = y, a MUX whose operands are gates of two levels and an input
    read by five gates, on uniform torus words: every double of every gate's selector.  At (1024, 6, 7), count 5, also 40 gates in one level: 2400 teams in one
    launch, more than the resident workgroups of the device."""
    D = _case(oracle, N, l, Bg_bit, count)
    c = eng.sellogic_create(D["gates"], D["n_in"], N)
    assert c.levels == 3
    d_in = _to_dft(eng, D["words"])
    before = d_in.clone()
    got = eng.trgsw_logic(c, d_in, l, Bg_bit)
    _assert_selectors(eng, got, D["rows"], D["back"], "(%d, %d, %d) x %d" % (N, l, Bg_bit, count))
    assert eng.torch.equal(d_in, before), "the call changed its inputs"
    c.close()
    if (N, l, Bg_bit, count) == (1024, 6, 7, 5):
        W = _case(oracle, N, l, Bg_bit, count, "wide")
        c = eng.sellogic_create(W["gates"], 3, N)
        assert c.levels == 1 and c.n_gates == 40
        _assert_selectors(eng, eng.trgsw_logic(c, _to_dft(eng, W["words"]), l, Bg_bit), W["rows"], W["back"], "40 gates in one level")
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg_bit", [(1024, 2, 8), (1024, 6, 7), (2048, 4, 9)])
def test_logic_value_edges(eng, oracle, N, l, Bg_bit):
    """Input rows drawn from {0, 1, 2^63 - 1, 2^63, 2^64 - 1} (none of which survives the double round trip beside 0 and 1: the left operand the kernel decomposes is
    T(X), not X), one component all 2^63 - 1 and one all 2^63; these words never give the digit Bg / 2 - 1 (tests/test_trlwe_gsw_linear.py), so two more are planted
    in input 0 -- every digit at Bg / 2 - 1, every digit at -Bg / 2 -- and the words the restatement really decomposes, T(X), are seen to reach both ends at every
    level.  Then one input that is 4 x a selector, made by eng.dft_lincomb: exact in doubles, and T() of it wraps mod 2^64."""
    oracle.plan(N)
    n_in, gates = ref.every_op_circuit()
    words = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)
    rng = np.random.default_rng([0xED6E5, N, l])
    x = words[rng.integers(0, len(words), size=(2, n_in, 2 * l, 2, N))]
    x[1, 1, :, 0] = U64(2 ** 63 - 1)
    x[1, 1, :, 1] = U64(2 ** 63)
    half = 1 << (Bg_bit - 1)
    x[0, 0, :, 0, 3] = x[0, 0, :, 1, N - 1] = U64(sum((half - 1) << (64 - (i + 1) * Bg_bit) for i in range(l)))
    x[0, 0, :, 1, 5] = x[0, 0, :, 0, 0] = U64(sum((-half) << (64 - (i + 1) * Bg_bit) for i in range(l)) % 2 ** 64)
    left = ref.rows_of(oracle, oracle.trgsw_to_dft(np.ascontiguousarray(x[0, 0]), 1, l))
    assert not (left == x[0, 0]).all(), "the planted rows survive the round trip: the test would not meet T(X) != X"
    for i in range(l):
        digits = np.concatenate([oracle.poly_decompose_i(np.ascontiguousarray(p), Bg_bit, l, i).view(np.int64) for p in left.reshape(-1, N)])
        assert digits.min() == -half and digits.max() == half - 1, (i, digits.min(), digits.max())
    c = eng.sellogic_create(gates, n_in, N)
    rows, back = _want(oracle, gates, x, l, Bg_bit)
    _assert_selectors(eng, eng.trgsw_logic(c, _to_dft(eng, x), l, Bg_bit), rows, back, "(%d, %d, %d), extreme words" % (N, l, Bg_bit))
    u = rng.integers(0, 2 ** 64, size=(1, n_in, 2 * l, 2, N), dtype=U64)
    d_in = _to_dft(eng, u)
    d_in[0, 1] = eng.dft_lincomb(None, d_in[0, 1].contiguous(), 4.0)
    wires = [oracle.trgsw_to_dft(np.ascontiguousarray(w), 1, l) for w in u[0]]
    wires[1] = 4.0 * wires[1]
    rows, back = _want(oracle, gates, None, l, Bg_bit, in_dft=[wires])
    _assert_selectors(eng, eng.trgsw_logic(c, d_in, l, Bg_bit), rows, back, "(%d, %d, %d), 4 x a selector" % (N, l, Bg_bit))
    c.close()


SENTINEL = float.fromhex("0x1.5ea75ea75ea75p+300")


@pytest.mark.gpu
def test_logic_run_contexts(eng, oracle):
    """(1024, 2, 8), count 5.  Sentinel doubles one batch element long at both ends of d_out_dft stay; every batch element alone and the reversed batch give the words
    they give in the batch; count == 0 returns an empty tensor; one handle runs on two contexts of the same device; an output that overlaps the inputs is refused
    on real tensors and nothing is written."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg, count = 1024, 2, 8, 5
    D = _case(oracle, N, l, Bg, count)
    n_in, n_gates = D["n_in"], len(D["gates"])
    c = eng.sellogic_create(D["gates"], n_in, N)
    d_in = _to_dft(eng, D["words"])
    buf = torch.full((count + 2, n_gates, 2 * l, 2, N), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.trgsw_logic(c, d_in, l, Bg, out=buf[1:-1])
    torch.cuda.synchronize(eng.device)
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), "the call wrote outside d_out_dft"
    _assert_selectors(eng, buf[1:-1].contiguous(), D["rows"], D["back"], "between sentinels")
    whole = buf[1:-1].clone()
    for b in range(count):
        assert torch.equal(eng.trgsw_logic(c, d_in[b:b + 1].contiguous(), l, Bg)[0], whole[b]), "batch element %d alone" % b
    assert torch.equal(eng.trgsw_logic(c, d_in.flip(0).contiguous(), l, Bg), whole.flip(0)), "the reversed batch"
    assert tuple(eng.trgsw_logic(c, d_in[:0].contiguous(), l, Bg).shape) == (0, n_gates, 2 * l, 2, N)
    other = ma.Engine(0)
    try:
        assert torch.equal(other.trgsw_logic(c, d_in, l, Bg), whole), "the same handle on a second context"
    finally:
        other.close()
    sample = 2 * l * 2 * N
    flat = torch.zeros((2 * n_in + 2 * n_gates) * sample, dtype=torch.float64, device=eng.device)
    flat[:2 * n_in * sample] = d_in[:2].reshape(-1)
    before = flat.clone()
    two_in = flat[:2 * n_in * sample].view(2, n_in, 2 * l, 2, N)
    shape = (2, n_gates, 2 * l, 2, N)
    for start in (0, 2 * n_in * sample - 1):
        with pytest.raises(engine.MosfhetHipError, match="d_out_dft overlaps d_in_dft"):
            eng.trgsw_logic(c, two_in, l, Bg, out=flat[start:start + 2 * n_gates * sample].view(shape))
    torch.cuda.synchronize(eng.device)
    assert torch.equal(flat, before), "a refused call wrote to its output"
    got = eng.trgsw_logic(c, two_in, l, Bg, out=flat[2 * n_in * sample:].view(shape))                 # adjacent: fine
    assert torch.equal(got, whole[:2])
    c.close()


@pytest.mark.gpu
def test_logic_is_captured_in_a_graph(eng, oracle):
    """The call captured on a side stream after one eager call (the table is on the device from then on), replayed on two different inputs copied into the captured
    buffer: each replay == the eager doubles.  One stream, no parallel branches."""
    import torch
    N, l, Bg = 1024, 2, 8
    D = _case(oracle, N, l, Bg, 5)
    c = eng.sellogic_create(D["gates"], D["n_in"], N)
    all_in = _to_dft(eng, D["words"])
    halves = [slice(0, 2), slice(2, 4)]
    eager = [eng.trgsw_logic(c, all_in[h].contiguous(), l, Bg).clone() for h in halves]
    _assert_selectors(eng, eager[0], D["rows"][:2], D["back"][:2], "eager")
    d_in, d_out = all_in[halves[0]].clone(), torch.empty_like(eager[0])
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.trgsw_logic(c, d_in, l, Bg, out=d_out)
    for r in (1, 0):
        d_in.copy_(all_in[halves[r]])
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d_out, eager[r]), "replay %d differs from the plain call" % r
    del g
    c.close()


@pytest.mark.gpu
def test_two_host_threads_run_logic_on_their_own_streams(eng, oracle):
    """Two host threads, each on a stream of its own, run five calls each on ONE shared handle whose table reaches the device in whichever thread comes first (the
    handle's lock), at counts 5 and 2: every result equals the restatement's doubles."""
    import torch
    N, l, Bg = 1024, 2, 8
    D = _case(oracle, N, l, Bg, 5)
    c = eng.sellogic_create(D["gates"], D["n_in"], N)
    d_in = _to_dft(eng, D["words"])
    want = _to_dft(eng, D["rows"])
    jobs = [(d_in, want), (d_in[:2].contiguous(), want[:2].contiguous())]
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=eng.device)):
                for _ in range(5):
                    got = eng.trgsw_logic(c, jobs[k][0], l, Bg)
                    torch.cuda.current_stream().synchronize()
                    bad[k] += int(not torch.equal(got.view(torch.int64), jobs[k][1].view(torch.int64)))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg_bit", [(1024, 2, 8), (2048, 4, 9)])
def test_logic_equals_the_existing_routes(eng, oracle, N, l, Bg_bit):
    """One AND gate == eng.dft_to_torus of X's rows, mosfhet_hip_external_product_dft_batch with Y per batch element (key_stride, Y replicated over the 2l rows),
    eng.dft_to_torus, eng.torus_to_dft; one NOT gate == the torch composition H - dft_to_torus(X), torus_to_dft -- double for double, over a batch of 3."""
    import torch
    D = _case(oracle, N, l, Bg_bit, 5)
    d_in = _to_dft(eng, D["words"][:3])
    X, Y = d_in[:, 0].contiguous(), d_in[:, 1].contiguous()
    c = eng.sellogic_create([(ref.AND, 0, 1, -1), (ref.NOT, 0, -1, -1)], 3, N)
    got = eng.trgsw_logic(c, d_in, l, Bg_bit)
    c.close()
    tx = eng.dft_to_torus(X.view(-1, N)).view(3 * 2 * l, 2, N)
    keys = Y[:, None].expand(3, 2 * l, 2 * l, 2, N).reshape(3 * 2 * l, 2 * l, 2, N).contiguous()
    prod = eng.external_product_dft(keys, tx, l, Bg_bit)
    old = eng.torus_to_dft(eng.dft_to_torus(prod.view(-1, N))).view(3, 2 * l, 2, N)
    assert torch.equal(got[:, 0].contiguous().view(torch.int64), old.view(torch.int64)), "one AND gate differs from the composition of the existing calls"
    H = _dev(eng, ref.trivial_one(N, l, Bg_bit))
    neg = eng.torus_to_dft((H[None] - tx.view(3, 2 * l, 2, N)).view(-1, N)).view(3, 2 * l, 2, N)
    assert torch.equal(got[:, 1].contiguous().view(torch.int64), neg.view(torch.int64)), "one NOT gate differs from the torch composition"


def _fine_case(oracle):
    """(2048, 4, 9), sigma 2^-44: a key, the probe, and per input value the restatement of the incrementer and of the demultiplexer; made once"""
    if "fine" not in _CACHE:
        N, l, Bg, sigma = FINE
        r, s, d, m = _noise_setup(oracle, N, l, Bg, sigma, 0x5E112)
        inc, dmx = ref.incrementer(3), ref.demultiplexer(3)
        vals = (0, 3, 6)
        bits = [[(v >> i) & 1 for i in range(3)] for v in vals]
        words = np.stack([ref.encrypted_bits(oracle, r, b, s, l, Bg, sigma) for b in bits])
        _CACHE["fine"] = dict(N=N, l=l, Bg=Bg, sigma=sigma, r=r, s=s, d=d, m=m, inc=inc, dmx=dmx, vals=vals, bits=bits, words=words)
    return _CACHE["fine"]


@pytest.mark.gpu
def test_logic_decrypts_on_the_device(eng, oracle):
    """(2048, 4, 9), sigma 2^-44, the addresses {0, 3, 6} as three fresh selectors each.  The 3-bit incrementer's sum selectors drive Engine.trlwe_ram_read on an
    8-cell memory of four-bit messages: the cell at address + 1 decrypts within 2^57.  The demultiplexer's one-hot lines, as one-entry key views
    (mosfhet_hip_bsk_view_create), drive mosfhet_hip_cmux_batch between a sample of zeros and the probe: every line selects the words the restatement's selector
    selects (the oracle's external product on the restatement's wire), and they decrypt to line x message within 2^57."""
    import mosfhet_amd as ma
    F = _fine_case(oracle)
    N, l, Bg, s, r = F["N"], F["l"], F["Bg"], F["s"], F["r"]
    d_in = _to_dft(eng, F["words"])
    n_in, inc, sums = F["inc"]
    c = eng.sellogic_create(inc, n_in, N)
    out = eng.trgsw_logic(c, d_in, l, Bg)
    c.close()
    rows, back = _want(oracle, inc, F["words"], l, Bg)
    _assert_selectors(eng, out, rows, back, "incrementer")
    addr = out[:, [k - n_in for k in sums]].contiguous()                       # [3][3][2l][2][N]: bit i of address + 1
    msgs = (np.arange(8, dtype=U64) * U64(2) + U64(1)) << U64(60)               # cell a holds 2a + 1 on every coefficient
    mem = np.stack([np.stack([oracle.trlwe_sample(r, np.full(N, msgs[a], dtype=U64), s, F["sigma"]) for a in range(8)])] * 3)
    got = ma.to_numpy(eng.trlwe_ram_read(addr, _dev(eng, mem), 3, l, Bg))
    worst = max(float(oracle.torus_dist(oracle.trlwe_phase(got[b], s), np.full(N, msgs[(v + 1) % 8], dtype=U64)).max()) for b, v in enumerate(F["vals"]))
    print("memory read at the incremented address: worst distance 2^%.1f (bound 2^57)" % _log2(worst))
    assert worst < BOUND
    n_in, dmx, lines = F["dmx"]
    c = eng.sellogic_create(dmx, n_in, N)
    out = eng.trgsw_logic(c, d_in, l, Bg)
    c.close()
    rows, back = _want(oracle, dmx, F["words"], l, Bg)
    _assert_selectors(eng, out, rows, back, "demultiplexer")
    zero, probe = _dev(eng, np.zeros((1, 2, N), dtype=U64)), _dev(eng, F["d"][None])
    worst = 0.0
    for b, v in enumerate(F["vals"]):
        for a, k in enumerate(lines):
            key = eng.bootstrap_key_view(out[b, k - n_in:k - n_in + 1].contiguous(), 1, l, Bg)
            key.set_product_order("reference")
            sel = ma.to_numpy(eng.cmux(key, 0, zero, probe))[0]
            key.free()
            wire = oracle.trgsw_to_dft(np.ascontiguousarray(rows[b, k - n_in]), 1, l)
            with oracle.product_order("reference"):
                assert (sel == oracle.external_product(F["d"], wire, l, Bg)).all(), (v, a)
            want = F["m"] if a == v else np.zeros_like(F["m"])
            worst = max(worst, float(oracle.torus_dist(oracle.trlwe_phase(sel, s), want).max()))
    print("CMUX by the one-hot lines: worst distance 2^%.1f (bound 2^57)" % _log2(worst))
    assert worst < BOUND


@pytest.mark.gpu
def test_logic_with_selectors_from_the_circuit_bootstrap(eng, oracle):
    """Plumbing.  The key set-up of tests/test_lut_bits.py: the selectors come from mosfhet_hip_circuit_bootstrap_3_dft_batch on LWE-encrypted bits and go into a
    two-gate circuit with no repacking in between.  Such selectors are not expected to survive a product (include/mosfhet_hip.h), so the call is held to the
    words of the restatement on the oracle's circuit bootstrap of the same bits."""
    from test_lut_bits import _pipeline
    D = _pipeline(eng, oracle)
    N, l, Bg, count = D["N"], D["l"], D["Bg"], 2
    bits = np.stack([np.arange(b * D["size"], b * D["size"] + 2) for b in range(count)]).reshape(-1)
    d_cts = D["d_cts"][eng.torch.from_numpy(bits).to(eng.device)].contiguous()
    sel = eng.circuit_bootstrap_3_dft(D["keys"]["reference"], D["kska"], D["pk"], d_cts).reshape(count, 2, 2 * l, 2, N)
    wires = [[np.ascontiguousarray(D["want_dft1"][k]) for k in bits[b * 2:(b + 1) * 2]] for b in range(count)]
    gates = [(ref.XOR, 0, 1, -1), (ref.MUX, 2, 0, 1)]
    rows, back = _want(oracle, gates, None, l, Bg, in_dft=wires)
    c = eng.sellogic_create(gates, 2, N)
    _assert_selectors(eng, eng.trgsw_logic(c, sel, l, Bg), rows, back, "circuit-bootstrapped selectors")
    c.close()


@pytest.mark.gpu
def test_sellogic_host_face(native_lib, tmp_path):
    """tests/c/trgsw_logic.c on host structs: one AND gate through mosfhet_trgsw_logic equals the drop-in layer's own trgsw_mul_DFT2 word for word, and the 4-bit
    incrementer's sum selectors decrypt a + 1 at (2048, 4, 9)."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trgsw_logic ok" in r.stdout, r.stdout[-3000:]
