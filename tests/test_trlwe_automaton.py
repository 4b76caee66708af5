"""Encrypted automata: a deterministic weighted automaton / layered branching program run backwards over words of TRGSW_DFT-encrypted bits (include/mosfhet_hip.h:
mosfhet_hip_automaton_create, mosfhet_hip_trlwe_automaton_batch, mosfhet_hip_trlwe_automaton_plan; lut_cmux_kernel mode 4 of mosfhet_amd/csrc/leveled_lut_kernels.h).

The expected words are the restatement of tests/trlwe_automaton_reference.py -- oracle.external_product, oracle.poly_mul_by_xai and word arithmetic alone -- on
oracle.bk_to_dft of the same selector words.  Every device comparison is == on every word; there is no tolerance anywhere.  The decryption bound 2^(64 - prec - 1)
is a condition on the INPUTS, which the restatement alone meets on the CPU (test_restatement_decrypts prints the slack); it is no tolerance on the GPU side.
"""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import trlwe_automaton_reference as ref
import trlwe_ram_reference as ram_ref
from test_leveled_lut import _map
from test_leveled_lut_edges import _target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
_CACHE = {}

# (N, l, Bg_bit): sigma of fresh samples
SIGMA = {(1024, 3, 10): 2.0 ** -44, (2048, 4, 9): 2.0 ** -44, (1024, 2, 8): 2.0 ** -25, (2048, 1, 23): 2.0 ** -52, (1024, 1, 23): 2.0 ** -52}
# the four gadgets of the noise table: (N, l, Bg_bit, prec)
NOISE_SETS = {"N1024 l2 Bg8": (1024, 2, 8, 2), "N1024 l3 Bg10": (1024, 3, 10, 4), "N2048 l4 Bg9": (2048, 4, 9, 4), "N2048 l1 Bg23": (2048, 1, 23, 4)}
# parity: (N, l, Bg_bit, states, steps, count, layers or a name of _tables, the start >= 0 to try)
PARITY = {"N1024 l2 Bg8 1 state 1 step x 1": (1024, 2, 8, 1, 1, 1, 1, 0),
          "N1024 l2 Bg8 3 states 2 steps x 2": (1024, 2, 8, 3, 2, 2, 1, 1),
          "N1024 l2 Bg8 3 states 4 steps x 5, edge rotations": (1024, 2, 8, 3, 4, 5, "edges", 2),
          "N1024 l2 Bg8 3 states 5 steps x 3, 2 layers": (1024, 2, 8, 3, 5, 3, 2, 0),
          "N1024 l2 Bg8 4 states 3 steps x 2, 3 layers": (1024, 2, 8, 4, 3, 2, 3, 3),
          "N1024 l2 Bg8 128 states 2 steps x 9": (1024, 2, 8, 128, 2, 9, 1, 77),
          "N1024 l1 Bg23 5 states 3 steps x 7": (1024, 1, 23, 5, 3, 7, 1, 4),
          "N1024 l3 Bg10 3 states 3 steps x 2": (1024, 3, 10, 3, 3, 2, 1, 1),
          "N2048 l4 Bg9 3 states 3 steps x 2": (2048, 4, 9, 3, 3, 2, 1, 2),
          "N2048 l1 Bg23 2 states 2 steps x 2": (2048, 1, 23, 2, 2, 2, 1, 1)}
SMALL = "N1024 l2 Bg8 3 states 4 steps x 5, edge rotations"

# the machine of the noise table: state 0 counts the ones in the exponent (a 1 multiplies by X), states 1 (even) and 2 (odd) swap on a 1
COUNTER = ([[0, 1, 2]], [[0, 2, 1]], [[0, 0, 0]], [[1, 0, 0]])


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _tables(N, states, layers, rng):
    """[layers][states] x (next0, next1, rot0, rot1).  "edges": one layer of 3 states with rotations from {0, 1, N - 1, N, N + 1, 2N - 1}, a self-loop (state 0 on a 0),
    fan-in (states 0 and 1 both read source 0, with different rotations) and next0 = next1 with rot0 = rot1 (state 2, whose difference is zero).  Else random entries,
    the first layer's rotations of state 0 again from that set, so that N - 1 (which "edges" has no place for) is met at 2 layers."""
    if layers == "edges":
        assert states == 3
        return (np.array([[0, 0, 1]]), np.array([[1, 0, 1]]), np.array([[0, 1, N + 1]]), np.array([[2 * N - 1, N, N + 1]]))
    t = [rng.integers(0, states, size=(layers, states)), rng.integers(0, states, size=(layers, states)),
         rng.integers(0, 2 * N, size=(layers, states)), rng.integers(0, 2 * N, size=(layers, states))]
    t[2][0, 0], t[3][0, 0] = N - 1, 2 * N - 1
    return tuple(t)


def _selectors(oracle, r, s, words, steps, l, Bg, sigma):
    """[len(words)][steps][2l][2][N] torus words: selector t of input b encrypts bit t of words[b]"""
    return np.stack([np.stack([oracle.trgsw_monomial_sample(r, (w >> t) & 1, 0, s, l, Bg, sigma) for t in range(steps)]) for w in words])


def _dfts(oracle, sel, l):
    return _map(lambda b: oracle.bk_to_dft(sel[b], 1, l), range(len(sel)))


def _want(oracle, tables, dft, init, l, Bg):
    """V_0 of every input: [count][states][2][N]; init [count][states][2][N] or [states][2][N] (shared)"""
    return np.stack(_map(lambda b: ref.run(oracle, tables, dft[b], init if init.ndim == 3 else init[b], l, Bg), range(len(dft))))


def _parity_case(oracle, name):
    """tables, initial vectors of random words, the selectors of the even inputs fresh encryptions of the word's bits and of the odd inputs random words; the
    restatement's V_0 per input and with input 0's vector shared by the batch (cached: the tests of one run share them)"""
    if name in _CACHE:
        return _CACHE[name]
    N, l, Bg, states, steps, count, layers, start = PARITY[name]
    oracle.plan(N)
    seed = 0xA07 + 131 * states + 17 * steps + 7 * count + N + l
    r, rng = oracle.Rng(seed), np.random.default_rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    tables = _tables(N, states, layers, rng)
    words = [int(w) for w in rng.integers(0, 1 << steps, size=count)]
    sel = _selectors(oracle, r, s, words, steps, l, Bg, SIGMA[(N, l, Bg)])
    sel[1::2] = rng.integers(0, 2 ** 64, size=sel[1::2].shape, dtype=U64)
    init = rng.integers(0, 2 ** 64, size=(count, states, 2, N), dtype=U64)
    dft = _dfts(oracle, sel, l)
    S = dict(N=N, l=l, Bg=Bg, states=states, steps=steps, count=count, tables=tables, start=start, sel=sel, init=init, dft=dft,
             want=_want(oracle, tables, dft, init, l, Bg), want_shared=_want(oracle, tables, dft, init[0], l, Bg))
    _CACHE[name] = S
    return S


def _noise_case(oracle, name, steps):
    """a key, an initial vector of fresh samples of prec-bit messages on every coefficient, a random word of `steps` fresh selectors, and the counter + parity machine
    run over it by the restatement: dict(..., msgs [3][N], word, sel, init, out = V_0)"""
    key = ("noise", name, steps)
    if key in _CACHE:
        return _CACHE[key]
    N, l, Bg, prec = NOISE_SETS[name]
    oracle.plan(N)
    sigma = SIGMA[(N, l, Bg)]
    r, rng = oracle.Rng(0xA0153 + N + l + steps), np.random.default_rng(0xA0153 + N + l + steps)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    msgs = rng.integers(0, 1 << prec, size=(3, N), dtype=U64) << U64(64 - prec)
    init = np.stack([oracle.trlwe_sample(r, msgs[q].copy(), s, sigma) for q in range(3)])
    word = int(rng.integers(0, 1 << 62)) & ((1 << steps) - 1) if steps < 64 else int(rng.integers(0, 2 ** 64, dtype=U64))
    sel = _selectors(oracle, r, s, [word], steps, l, Bg, sigma)[0]
    out = ref.run(oracle, COUNTER, oracle.bk_to_dft(sel, 1, l), init, l, Bg)
    _CACHE[key] = dict(N=N, l=l, Bg=Bg, prec=prec, steps=steps, s=s, msgs=msgs, word=word, sel=sel, init=init, out=out)
    return _CACHE[key]


def _worst(oracle, S, V0):
    """worst distance of a state's phase from its message: state 0 X^ones m_0; states 1, 2: m_1, m_2, swapped on odd parity"""
    ones = bin(S["word"]).count("1")
    msgs = [oracle.poly_mul_by_xai(np.ascontiguousarray(S["msgs"][0]), ones), S["msgs"][1 + (ones & 1)], S["msgs"][2 - (ones & 1)]]
    return max(float(oracle.torus_dist(oracle.trlwe_phase(V0[q], S["s"]), msgs[q]).max()) for q in range(3))


def _create(tables, N):
    from mosfhet_amd import engine
    return engine.automaton_create(*tables, N)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1024, 2, 8), (1024, 3, 10), (2048, 4, 9), (2048, 1, 23)])
def test_restatement_equals_known_compositions(oracle, shape):
    """On random words and on fresh selectors: one state with next = (0, 0), rot0 = 0, rot1 = a is acc + sel (.) ((X^a - 1) acc) built from
    oracle.poly_mul_by_xai_minus_1 (the blind rotation's step); two states, one step, start = 0, next = (0, 1), no rotation is trlwe_ram_reference.cmux."""
    N, l, Bg = shape
    oracle.plan(N)
    rng, r = np.random.default_rng(N + l), oracle.Rng(N + l)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    sel = _selectors(oracle, r, s, [1, 0], 1, l, Bg, SIGMA[shape])
    sel[1] = rng.integers(0, 2 ** 64, size=sel[1].shape, dtype=U64)
    init = rng.integers(0, 2 ** 64, size=(2, 2, N), dtype=U64)
    for b in range(2):
        dft = oracle.bk_to_dft(sel[b], 1, l)
        for a in (0, 1, N - 1, N, N + 1, 2 * N - 1, int(rng.integers(0, 2 * N))):
            got = ref.run(oracle, ([[0]], [[0]], [[0]], [[a]]), dft, init[:1], l, Bg)
            acc = init[0]
            d = np.stack([oracle.poly_mul_by_xai_minus_1(np.ascontiguousarray(acc[c]), a) for c in range(2)])
            assert (got[0] == acc + oracle.external_product(d, dft[0], l, Bg)).all(), (shape, b, a)
        got = ref.run(oracle, ([[0, 0]], [[1, 1]], [[0, 0]], [[0, 0]]), dft, init, l, Bg, start=0)
        assert (got == ram_ref.cmux(oracle, dft[0], init[0], init[1], l, Bg)).all(), (shape, b)


@pytest.mark.parametrize("steps", [16, 64])
@pytest.mark.parametrize("name", list(NOISE_SETS))
def test_restatement_decrypts(oracle, name, steps):
    """The condition on the inputs, on the restatement alone: the counter + parity machine over a random word of fresh selectors, from fresh samples: every
    coefficient of every state is within half a slot 2^(64 - prec - 1) of its message."""
    S = _noise_case(oracle, name, steps)
    w = _worst(oracle, S, S["out"])
    bound = 64 - S["prec"] - 1
    print("%s, %d steps, word %x: worst state 2^%.1f, bound 2^%d" % (name, steps, S["word"], _log2(w), bound))
    assert w < 2.0 ** bound, (name, steps, _log2(w))


def _batch(native_lib):
    fn = native_lib.mosfhet_hip_trlwe_automaton_batch
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p]
    return fn


def test_automaton_symbols_and_argument_checks(native_lib):
    """The library exports the entry points and the host layer's one; every refusal is MOSFHET_HIP_EINVAL with a message naming the argument, on fake pointers that
    are never dereferenced -- before any HIP call (this runs without a GPU; a handle is made on the host)."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_automaton_create", "mosfhet_hip_automaton_destroy", "mosfhet_hip_automaton_info", "mosfhet_hip_trlwe_automaton_batch",
                 "mosfhet_hip_trlwe_automaton_plan", "mosfhet_trlwe_automaton"):
        assert hasattr(native_lib, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    assert engine.AUTOMATON_MAX_STATES == 4096 and engine.AUTOMATON_MAX_STEPS == 4096
    # creation
    i32 = lambda *v: np.array(v, dtype=np.int32)
    ok = [i32(0, 1, 2), i32(0, 2, 1), i32(0, 0, 0), i32(1, 0, 2047)]
    a = engine.automaton_create(*ok, 1024)
    assert a.info() == dict(N=1024, states=3, layers=1)
    two = engine.automaton_create(*[np.stack([t, t]) for t in ok], 1024)
    assert two.info() == dict(N=1024, states=3, layers=2)
    two.close()
    for k, (bad, what) in enumerate([(3, "next0[0][1] = 3"), (-1, "next1[0][1] = -1"), (2048, "rot0[0][1] = 2048"), (-1, "rot1[0][1] = -1")]):
        t = [x.copy() for x in ok]
        t[k][1] = bad
        with pytest.raises(engine.MosfhetHipError, match=what.replace("[", r"\[").replace("]", r"\]")):
            engine.automaton_create(*t, 1024)
    assert engine.automaton_create(*ok[:3], i32(1, 0, 4095), 2048).info()["N"] == 2048        # (a rotation below 2N of ITS ring)
    for N in (512, 4096):
        with pytest.raises(engine.MosfhetHipError, match="N = %d" % N):
            engine.automaton_create(*ok, N)
    h = C.c_void_p()
    p = [x.ctypes.data_as(C.c_void_p) for x in ok]
    mk = native_lib.mosfhet_hip_automaton_create
    assert mk(None, *p, 3, 1, 1024) == -1 and "out" in err()
    for k, what in enumerate(("h_next0", "h_next1", "h_rot0", "h_rot1")):
        q = list(p)
        q[k] = None
        assert mk(C.byref(h), *q, 3, 1, 1024) == -1 and what in err()
    assert mk(C.byref(h), *p, 0, 1, 1024) == -1 and "states = 0" in err()
    assert mk(C.byref(h), *p, 4097, 1, 1024) == -1 and "states = 4097" in err()
    assert mk(C.byref(h), *p, 3, 0, 1024) == -1 and "layers = 0" in err()
    assert mk(C.byref(h), *p, 3, 4097, 1024) == -1 and "layers = 4097" in err()
    info = (C.c_longlong * 3)()
    assert native_lib.mosfhet_hip_automaton_info(None, info) == -1 and "automaton" in err()
    assert native_lib.mosfhet_hip_automaton_info(a.h, None) == -1 and "info" in err()
    # the call: (ctx, d_out, automaton, d_sel_dft, d_init, init_shared, steps, start, l, Bg_bit, count, stream)
    f = _batch(native_lib)
    fake, sel, init = C.c_void_p(1 << 40), C.c_void_p(1 << 41), C.c_void_p(1 << 42)
    row = 2 * 1024 * 8
    assert f(None, fake, a.h, sel, init, 0, 4, -1, 2, 8, 4, None) == -1 and "ctx" in err()
    assert f(fake, None, a.h, sel, init, 0, 4, -1, 2, 8, 4, None) == -1 and "d_out" in err()
    assert f(fake, fake, None, sel, init, 0, 4, -1, 2, 8, 4, None) == -1 and "automaton" in err()
    assert f(fake, fake, a.h, None, init, 0, 4, -1, 2, 8, 4, None) == -1 and "d_sel_dft" in err()
    assert f(fake, fake, a.h, sel, None, 0, 4, -1, 2, 8, 4, None) == -1 and "d_init" in err()
    assert f(fake, fake, a.h, sel, init, 0, 0, -1, 2, 8, 4, None) == -1 and "steps = 0" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4097, -1, 2, 8, 4, None) == -1 and "steps = 4097" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, 3, 2, 8, 4, None) == -1 and "start = 3" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, -1, 4, 16, 4, None) == -1 and "l=4 Bg_bit=16" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, -1, 7, 8, 4, None) == -1 and "l = 7" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, -1, 2, 32, 4, None) == -1 and "Bg_bit=32" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, -1, 0, 8, 4, None) == -1 and "l=0" in err()
    assert f(fake, fake, a.h, sel, init, 0, 4, -1, 2, 8, -1, None) == -1 and "count = -1" in err()
    # overlap as address ranges: the vectors of 4 inputs of 3 states are 12 rows from `init` (3 when shared); the output 12 rows, or 4 with a start state
    i0 = init.value
    for o in (i0, i0 + 11 * row, i0 + 12 * row - 8, i0 - 12 * row + 8, i0 + 8):
        assert f(fake, C.c_void_p(o), a.h, sel, init, 0, 4, -1, 2, 8, 4, None) == -1 and "d_out overlaps d_init" in err(), hex(o)
    for o in (i0 + 3 * row - 8, i0 - 4 * row + 8):
        assert f(fake, C.c_void_p(o), a.h, sel, init, 1, 4, 0, 2, 8, 4, None) == -1 and "d_out overlaps d_init" in err(), hex(o)
    # count = 0 does nothing and says OK, whatever the pointers
    assert f(fake, None, a.h, None, None, 0, 4, -1, 2, 8, 0, None) == 0
    # a workspace bound below one input's two state vectors: refused
    try:
        engine.set_leveled_lut_workspace(2 * 3 * row - 8)
        assert f(fake, fake, a.h, sel, init, 0, 4, -1, 2, 8, 4, None) == -1 and "workspace bound" in err()
    finally:
        engine.set_leveled_lut_workspace(0)
    plan = (C.c_longlong * 5)()
    pl = native_lib.mosfhet_hip_trlwe_automaton_plan       # (N, l, states, layers, steps, start, count, cus, plan)
    assert pl(1024, 2, 3, 1, 4, -1, 4, 256, None) == -1 and "plan" in err()
    assert pl(4096, 1, 3, 1, 4, -1, 4, 256, plan) == -1 and "N = 4096" in err()
    assert pl(1024, 2, 3, 1, 4, -1, 0, 256, plan) == -1 and "count = 0" in err()
    assert pl(1024, 2, 3, 1, 4, -1, 4, 0, plan) == -1 and "cus = 0" in err()
    assert pl(1024, 2, 4097, 1, 4, -1, 4, 256, plan) == -1 and "states = 4097" in err()
    assert pl(1024, 2, 3, 4097, 4, -1, 4, 256, plan) == -1 and "layers = 4097" in err()
    assert pl(1024, 2, 3, 1, 4, 3, 4, 256, plan) == -1 and "start = 3" in err()
    # a handle made for another N: the binding knows the ring from its tensors and refuses before the call (the C call takes N from the handle)
    import torch

    class Stub:
        h = fake
    Stub.torch = torch
    with pytest.raises(engine.MosfhetHipError, match="made for N = 1024"):
        engine.Engine.trlwe_automaton(Stub, a, torch.empty((1, 2, 8, 2, 2048), dtype=torch.float64), torch.empty((1, 3, 2, 2048), dtype=torch.int64), 4, 9)
    a.close()


def test_automaton_plan_sweep(native_lib):
    """mosfhet_hip_trlwe_automaton_plan -- the function the launcher decides with -- over both rings, several state counts, word lengths and batches, a start state on and
    off, a device of 256 and of 64 CUs: the products formula; 0 / 1 / 2 buffers; chunks of whole inputs as large as the bound allows; a lowered bound gives more
    chunks and never a larger workspace; a bound below one input is refused."""
    from mosfhet_amd import engine
    GiB = 1 << 30
    for cus in (256, 64):
        for N in (1024, 2048):
            for states in (1, 3, 128, 4096):
                for steps in (1, 2, 3, 64, 4096):
                    buffers = min(steps - 1, 2)
                    per_input = buffers * states * 2 * N * 8
                    for count in (1, 3, 257, 4096):
                        for start in (-1, 0, states - 1):
                            p = engine.trlwe_automaton_plan(N, 2, states, 1, steps, count, start, cus)
                            what = (cus, N, states, steps, count, start, p)
                            assert p["products"] == count * (states * (steps - 1) + (states if start < 0 else 1)), what
                            assert p["buffers"] == buffers and 1 <= p["chunk"] <= count, what
                            assert p["launches"] == steps * -(-count // p["chunk"]), what
                            assert p["workspace_bytes"] == p["chunk"] * per_input and p["workspace_bytes"] <= GiB, what
                            assert p["chunk"] == count or (p["chunk"] + 1) * per_input > GiB, what      # as large as the bound allows
                            assert p == engine.trlwe_automaton_plan(N, 2, states, 7, steps, count, start, 256), what     # CUs size grids only; layers nothing
    vec = 3 * 2 * 1024 * 8
    try:
        p0 = engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5)
        assert p0 == dict(launches=4, chunk=5, workspace_bytes=2 * 5 * vec, products=5 * 12, buffers=2)
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5, 1)["products"] == 5 * 10
        engine.set_leveled_lut_workspace(2 * 2 * vec + 8)
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5) == dict(launches=12, chunk=2, workspace_bytes=2 * 2 * vec, products=60, buffers=2)
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 2, 5) == dict(launches=4, chunk=4, workspace_bytes=4 * vec, products=30, buffers=1)
        engine.set_leveled_lut_workspace(2 * vec)
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5) == dict(launches=20, chunk=1, workspace_bytes=2 * vec, products=60, buffers=2)
        engine.set_leveled_lut_workspace(2 * vec - 8)                    # not even one input: refused, not overrun
        with pytest.raises(engine.MosfhetHipError, match="workspace bound"):
            engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5)
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 2, 5)["chunk"] == 1      # one buffer still fits
        assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 1, 5) == dict(launches=1, chunk=5, workspace_bytes=0, products=15, buffers=0)   # one step: no workspace
    finally:
        engine.set_leveled_lut_workspace(0)
    assert engine.trlwe_automaton_plan(1024, 2, 3, 1, 4, 5) == p0
    for bad in (0, engine.AUTOMATON_MAX_STEPS + 1):
        with pytest.raises(engine.MosfhetHipError, match="steps"):
            engine.trlwe_automaton_plan(1024, 2, 3, 1, bad, 1)


def test_automaton_kernels_of_the_build(native_lib):
    """The step lives in lut_cmux_kernel: it is still one instantiation per ring with at most 256 registers, 64 KiB of static LDS and no scratch; the library holds
    exactly 329 kernels; tools/check_lds_barriers.py lists the leveled-LUT form, which compiles the kernel with the automaton step, and finds nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    import kernel_table
    forms = [f for f in chk.FORMS if "automaton step" in f[0]]
    assert forms and all("leveled LUT" in f[0] and "memory modes" in f[0] for f in forms), [f[0] for f in chk.FORMS]
    assert chk.build_and_check(forms) == []
    rows = kernel_table.table()
    mine = [r for r in rows if r["name"].startswith("lut_cmux_kernel")]
    assert sorted(r["name"].replace("> >", ">>") for r in mine) == ["lut_cmux_kernel<Fft1024>", "lut_cmux_kernel<Fft2048T<false, false>>"], [r["name"] for r in mine]
    for r in mine:
        print("%-50s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
        assert r["vgpr"] <= 256 and r["lds"] <= 64 * 1024 and r["scratch"] == 0, r
    assert len(rows) == 329, len(rows)


def test_automaton_c_program_compiles(native_lib, tmp_path):
    """tests/c/trlwe_automaton.c compiles with -Wall -Werror against include/mosfhet.h and links with the library (it runs in the GPU tests)."""
    _compile_c(str(tmp_path / "trlwe_automaton"))


def _compile_c(exe):
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_automaton.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _dev_sel(eng, sel):
    """[count][steps][2l][2][N] torus words -> the same shape in the DFT domain, on the device"""
    import mosfhet_amd as ma
    return eng.trgsw_to_dft(ma.to_device(sel, eng.device))


def _run(eng, S, auto, sel, init, start=-1):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.trlwe_automaton(auto, sel, ma.to_device(init, eng.device), S["l"], S["Bg"], start))


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1, 2, got.shape[-1]), want.reshape(-1, 2, want.shape[-1])
    bad = [u for u in range(len(w)) if not (g[u] == w[u]).all()]
    assert not bad, "%s: %d of %d samples differ from the restatement (first: %s)" % (what, len(bad), len(w), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_automaton_matches_the_restatement(eng, oracle, name):
    """Parity: every shape -- one step straight from the initial vector to the output, two steps through one buffer, more through both; one, two and `steps` layers;
    rotations at the ends of both halves of [0, 2N), self-loops, fan-in and a zero difference; more units than resident workgroups; both rings, four gadgets; fresh
    selectors and random selector words -- equals the restatement on every word: every state, one start state (that row of the full result, computed alone in the
    last launch), and one initial vector shared by the batch (the replicated vector's words).  The initial vector is left as it was."""
    import mosfhet_amd as ma
    S = _parity_case(oracle, name)
    auto = _create(S["tables"], S["N"])
    sel = _dev_sel(eng, S["sel"])
    d_init = ma.to_device(S["init"], eng.device)
    got = ma.to_numpy(eng.trlwe_automaton(auto, sel, d_init, S["l"], S["Bg"]))
    _assert_rows(got, S["want"], name + ", every state")
    assert (ma.to_numpy(d_init) == S["init"]).all(), "the call changed the initial vector"
    _assert_rows(_run(eng, S, auto, sel, S["init"], S["start"]), S["want"][:, S["start"]], name + ", start = %d" % S["start"])
    shared = _run(eng, S, auto, sel, S["init"][0])
    _assert_rows(shared, S["want_shared"], name + ", shared initial vector")
    _assert_rows(shared, _run(eng, S, auto, sel, np.stack([S["init"][0]] * S["count"])), name + ", shared against replicated")
    _assert_rows(_run(eng, S, auto, sel, S["init"][0], S["start"]), S["want_shared"][:, S["start"]], name + ", shared, start = %d" % S["start"])
    auto.close()


EDGE_TABLES = ([[0, 1, 2, 3]], [[1, 2, 3, 3]], [[0, 0, 0, 0]], [[0, 0, 0, 0]])      # state q: V[q] + sel (.) (V[q + 1] - V[q]); state 3: a zero difference


def _edge_inputs(N, l, Bg, seed):
    """4 states, 2 steps, 6 inputs, EDGE_TABLES with N put into rot1 of state 3 by the caller (difference -2 V[3]).  Words of {0, 1, 2^63 - 1, 2^63, 2^64 - 1} in
    the initial vectors and selector rows (inputs 0 .. 3: every row word one value / alternating / drawn from the set / zero); inputs 4 and 5 planted so that the
    first step of states 0, 1, 2 decomposes a polynomial whose digits are all at one end of every level (tests/test_leveled_lut_edges.py: _target): V[1] - V[0] =
    top, V[2] - V[1] = bottom, V[3] - V[2] alternating -- against selector rows of -2^63 and of 2^63 - 1."""
    rng = np.random.default_rng(seed)
    words = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)
    draw = lambda *shape: words[rng.integers(0, 5, size=shape)]
    count, steps = 6, 2
    init, sel = draw(count, 4, 2, N), np.zeros((count, steps, 2 * l, 2, N), dtype=U64)
    sel[0] = U64(2 ** 63)
    sel[1] = U64(2 ** 63 - 1)
    sel[1, ..., ::2] = U64(2 ** 63)
    sel[2] = draw(steps, 2 * l, 2, N)
    lo, hi = U64(_target(l, Bg, 0)), U64(_target(l, Bg, (1 << Bg) - 1))
    alt = np.full(N, lo, dtype=U64)
    alt[::2] = hi
    for b, word in ((4, 2 ** 63), (5, 2 ** 63 - 1)):
        sel[b] = U64(word)
        init[b, 1] = init[b, 0] + hi
        init[b, 2] = init[b, 1] + lo
        init[b, 3] = init[b, 2] + alt
    return init, sel


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 3, 10), (1024, 2, 8), (2048, 4, 9)])
def test_automaton_value_edges(eng, oracle, shape):
    """Value edges.  The extreme words and the planted digit extremes of _edge_inputs (the sums reach 2l N 2^(Bg-1) 2^63, past what rounding without the reduction
    mod 1 holds at l = 3, Bg_bit = 10); then selectors summed on the device to a + 2^16 b, beyond what any transform of torus words reaches, against the restatement
    on the device's own doubles copied back.  Every word of every state."""
    from mosfhet_amd import engine
    N, l, Bg = shape
    oracle.plan(N)
    S = dict(N=N, l=l, Bg=Bg)
    tables = [np.array(t) for t in EDGE_TABLES]
    tables[3][0, 3] = N
    init, sel = _edge_inputs(N, l, Bg, N + l)
    for d, ends in ((init[4, 1] - init[4, 0], "top"), (init[4, 2] - init[4, 1], "bottom"), (init[5, 2] - init[5, 1], "bottom")):
        for i in range(l):
            digits = oracle.poly_decompose_i(np.ascontiguousarray(d[0]), Bg, l, i).view(np.int64)
            assert (digits == ((1 << (Bg - 1)) - 1 if ends == "top" else -(1 << (Bg - 1)))).all(), (shape, ends, i)
    auto = _create(tables, N)
    _assert_rows(_run(eng, S, auto, _dev_sel(eng, sel), init), _want(oracle, tables, _dfts(oracle, sel, l), init, l, Bg), "%s, extreme words" % (shape,))
    rng = np.random.default_rng(N + l + 1)
    a, b = [_dev_sel(eng, rng.integers(0, 2 ** 64, size=(2, 2, 2 * l, 2, N), dtype=U64)) for _ in range(2)]
    big = eng.dft_lincomb(a, b, 2.0 ** 16)
    host = engine.slot_order_to_oracle(big.cpu().numpy().reshape(-1, N), N).reshape(2, 2, 2 * l, 2, N)
    mag = float(np.abs(host).max())
    print("%s: largest |selector double| of a + 2^16 b: 2^%.1f" % (shape, _log2(mag)))
    assert np.isfinite(host).all() and mag > 2.0 ** 78
    dft = [np.ascontiguousarray(host[i]) for i in range(2)]
    _assert_rows(_run(eng, S, auto, big, init[:2]), _want(oracle, tables, dft, init[:2], l, Bg), "%s, a + 2^16 b" % (shape,))
    auto.close()


SENTINEL = 0x5EA75EA75EA75EA7


@pytest.mark.gpu
def test_automaton_stays_inside_its_buffers(eng, oracle):
    """Run contexts.  3 states, 4 steps, 5 inputs, the initial vectors and the output each inside a sentinel-filled buffer one input longer at both ends: the call
    writes nothing outside [count][states][2][N] (with a start state: [count][2][N]) and no word of the initial vectors; the selectors are unchanged."""
    import torch
    import mosfhet_amd as ma
    S = _parity_case(oracle, SMALL)
    N, count, states = S["N"], S["count"], S["states"]
    auto = _create(S["tables"], N)
    sel = _dev_sel(eng, S["sel"])
    sel0 = sel.clone()
    ibuf = torch.full((count + 2, states, 2, N), SENTINEL, dtype=torch.int64, device=eng.device)
    obuf = torch.full((count + 2, states, 2, N), SENTINEL, dtype=torch.int64, device=eng.device)
    sbuf = torch.full((count + 2, 2, N), SENTINEL, dtype=torch.int64, device=eng.device)
    ibuf[1:-1] = ma.to_device(S["init"], eng.device)
    eng.trlwe_automaton(auto, sel, ibuf[1:-1], S["l"], S["Bg"], out=obuf[1:-1])
    eng.trlwe_automaton(auto, sel, ibuf[1:-1], S["l"], S["Bg"], S["start"], out=sbuf[1:-1])
    torch.cuda.synchronize(eng.device)
    for got, want, what in ((ma.to_numpy(obuf), S["want"], "every state"), (ma.to_numpy(sbuf), S["want"][:, S["start"]], "one state")):
        assert (got[0] == U64(SENTINEL)).all() and (got[-1] == U64(SENTINEL)).all(), "%s: the call wrote outside its output" % what
        _assert_rows(got[1:-1], want, what + " between sentinels")
    i = ma.to_numpy(ibuf)
    assert (i[0] == U64(SENTINEL)).all() and (i[-1] == U64(SENTINEL)).all() and (i[1:-1] == S["init"]).all(), "the call wrote to the initial vectors"
    assert torch.equal(sel, sel0), "the call changed its selectors"
    auto.close()


@pytest.mark.gpu
def test_automaton_words_do_not_depend_on_the_batch(eng, oracle):
    """Run contexts.  A stale pool (the 128-state call first, in this thread's workspace); bounds forcing chunks of 1 and of 2 inputs equal one chunk; every input
    alone (count = 1) and at every position of the rotated batch gives the words it gives in the batch; count = 0 does nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    L = _parity_case(oracle, "N1024 l2 Bg8 128 states 2 steps x 9")
    big = _create(L["tables"], L["N"])
    _assert_rows(_run(eng, L, big, _dev_sel(eng, L["sel"]), L["init"]), L["want"], "the larger call in front")
    big.close()
    S = _parity_case(oracle, SMALL)
    N, l, Bg, states, steps, count = S["N"], S["l"], S["Bg"], S["states"], S["steps"], S["count"]
    auto = _create(S["tables"], N)
    sel = _dev_sel(eng, S["sel"])
    _assert_rows(_run(eng, S, auto, sel, S["init"]), S["want"], "behind the larger call")
    vec = states * 2 * N * 8
    try:
        engine.set_leveled_lut_workspace(2 * vec)
        assert eng.trlwe_automaton_plan(N, l, states, 1, steps, count) == dict(launches=20, chunk=1, workspace_bytes=2 * vec, products=60, buffers=2)
        _assert_rows(_run(eng, S, auto, sel, S["init"]), S["want"], "one input per chunk")
        _assert_rows(_run(eng, S, auto, sel, S["init"][0], S["start"]), S["want_shared"][:, S["start"]], "one input per chunk, shared vector, one state")
        engine.set_leveled_lut_workspace(2 * 2 * vec)
        assert eng.trlwe_automaton_plan(N, l, states, 1, steps, count)["chunk"] == 2
        _assert_rows(_run(eng, S, auto, sel, S["init"]), S["want"], "two inputs per chunk, the last chunk short")
        _assert_rows(_run(eng, S, auto, sel, S["init"], S["start"]), S["want"][:, S["start"]], "two inputs per chunk, one state")
    finally:
        engine.set_leveled_lut_workspace(0)
    for b in range(count):
        _assert_rows(_run(eng, S, auto, sel[b:b + 1].contiguous(), S["init"][b:b + 1]), S["want"][b:b + 1], "input %d alone" % b)
    for shift in range(1, count):
        idx = (np.arange(count) + shift) % count
        rs = sel[torch.from_numpy(idx).to(eng.device)].contiguous()
        _assert_rows(_run(eng, S, auto, rs, S["init"][idx]), S["want"][idx], "rotated by %d" % shift)
    empty = torch.empty((0, steps, 2 * l, 2, N), dtype=torch.float64, device=eng.device)
    assert tuple(eng.trlwe_automaton(auto, empty, eng.empty(0, states, 2, N), l, Bg).shape) == (0, states, 2, N)
    assert tuple(eng.trlwe_automaton(auto, empty, eng.empty(states, 2, N), l, Bg, 1).shape) == (0, 2, N)
    auto.close()


@pytest.mark.gpu
def test_automaton_calls_are_captured_in_a_graph(eng, oracle):
    """Run contexts.  A call for every state followed by one for a start state, captured on one side stream after an eager call of that shape, replayed twice on
    different inputs copied into the captured buffers: each replay == the eager words (which equal the restatement).  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    S = _parity_case(oracle, SMALL)
    l, Bg, start = S["l"], S["Bg"], S["start"]
    auto = _create(S["tables"], S["N"])
    all_sel = _dev_sel(eng, S["sel"])
    halves = [slice(0, 2), slice(2, 4)]
    eager = []
    for h in halves:
        i = ma.to_device(S["init"][h], eng.device)
        eager.append((ma.to_numpy(eng.trlwe_automaton(auto, all_sel[h].contiguous(), i, l, Bg)), ma.to_numpy(eng.trlwe_automaton(auto, all_sel[h].contiguous(), i, l, Bg, start))))
        _assert_rows(eager[-1][0], S["want"][h], "eager, every state")
        _assert_rows(eager[-1][1], S["want"][h, start], "eager, one state")
    d_sel, d_init = all_sel[halves[0]].clone(), ma.to_device(S["init"][halves[0]], eng.device)
    d_out, d_one = eng.empty(2, S["states"], 2, S["N"]), eng.empty(2, 2, S["N"])
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.trlwe_automaton(auto, d_sel, d_init, l, Bg, out=d_out)
        eng.trlwe_automaton(auto, d_sel, d_init, l, Bg, start, out=d_one)
    for r in (1, 0):
        d_sel.copy_(all_sel[halves[r]])
        d_init.copy_(ma.to_device(S["init"][halves[r]], eng.device))
        d_out.zero_()
        d_one.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_out) == eager[r][0]).all(), "replay %d: every state differs from the plain call" % r
        assert (ma.to_numpy(d_one) == eager[r][1]).all(), "replay %d: one state differs from the plain call" % r
    del g
    auto.close()


@pytest.mark.gpu
def test_host_threads_run_automata_on_their_own_streams(eng, oracle):
    """Run contexts.  Two host threads, each on a stream of its own, each five times its own shape (3 states x 4 steps x 5 inputs; 5 states x 3 steps x 7): every
    call equals the restatement.  The state-vector buffers belong to the calling thread's pool; shared between the threads they would mix the two shapes' vectors."""
    import torch
    import mosfhet_amd as ma
    jobs = [_parity_case(oracle, SMALL), _parity_case(oracle, "N1024 l1 Bg23 5 states 3 steps x 7")]
    autos = [_create(S["tables"], S["N"]) for S in jobs]
    dev = [(_dev_sel(eng, S["sel"]), ma.to_device(S["init"], eng.device)) for S in jobs]
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(t):
        try:
            S, (sel, init) = jobs[t], dev[t]
            with torch.cuda.stream(torch.cuda.Stream(device=eng.device)):
                for _ in range(5):
                    got = ma.to_numpy(eng.trlwe_automaton(autos[t], sel, init, S["l"], S["Bg"]))
                    bad[t] += int(not (got == S["want"]).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad
    for a in autos:
        a.close()


@pytest.mark.gpu
def test_automaton_refuses_overlapping_buffers(eng, oracle):
    """Run contexts.  Real pointers: an output that lies inside the initial vectors, or ends inside them, is refused with a message; the vectors are unchanged; an
    output directly behind them is fine."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    S = _parity_case(oracle, "N1024 l2 Bg8 3 states 2 steps x 2")
    auto = _create(S["tables"], S["N"])
    sel = _dev_sel(eng, S["sel"])
    buf = eng.empty(4, 3, 2, S["N"])
    buf[1:3] = ma.to_device(S["init"], eng.device)
    init = buf[1:3]
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_init"):
        eng.trlwe_automaton(auto, sel, init, S["l"], S["Bg"], out=init)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_init"):
        eng.trlwe_automaton(auto, sel, init, S["l"], S["Bg"], out=buf[0:2])
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_init"):
        eng.trlwe_automaton(auto, sel, init, S["l"], S["Bg"], 1, out=buf[2][:2])
    assert (ma.to_numpy(init) == S["init"]).all()
    _assert_rows(ma.to_numpy(eng.trlwe_automaton(auto, sel, init, S["l"], S["Bg"], 1, out=buf[3][:2])), S["want"][:, 1], "an output directly behind the vectors")
    auto.close()


@pytest.mark.gpu
def test_automaton_equals_the_existing_routes(eng, oracle):
    """Existing routes, word for word.  Two states, one step, start = 0, next = (0, 1): mosfhet_hip_trlwe_ram_read_batch at size 1 on the same two samples, and
    mosfhet_hip_cmux_batch with the selector as a one-entry key view at product order "reference".  One state, layers = steps = size <= log2 N, layer t rotating by
    2N - 2^(steps-1-t) with the selectors reversed, then trlwe_extract_tlwe(., 0): mosfhet_hip_leveled_lut_batch on a one-row table."""
    import mosfhet_amd as ma
    S = _parity_case(oracle, SMALL)
    N, l, Bg, count = S["N"], S["l"], S["Bg"], S["count"]
    sel = _dev_sel(eng, S["sel"])
    mux = _create(([[0, 0]], [[1, 1]], [[0, 0]], [[0, 0]]), N)
    pairs = ma.to_device(S["init"][:, :2], eng.device)
    one = sel[:, :1].contiguous()
    new = ma.to_numpy(eng.trlwe_automaton(mux, one, pairs, l, Bg, 0))
    assert (new == ma.to_numpy(eng.trlwe_ram_read(one, pairs, 1, l, Bg))).all(), "two states, one step differ from a size-1 memory read"
    for b in range(count):
        key = eng.bootstrap_key_view(one[b], 1, l, Bg)
        key.set_product_order("reference")
        old = ma.to_numpy(eng.cmux(key, 0, pairs[b, :1].contiguous(), pairs[b, 1:2].contiguous()))[0]
        key.free()
        assert (old == new[b]).all(), "input %d: two states, one step differ from cmux on a key view" % b
    mux.close()
    for size in (1, 4, 10):
        rng = np.random.default_rng(size)
        steps = size
        words = _dev_sel(eng, rng.integers(0, 2 ** 64, size=(3, size, 2 * l, 2, N), dtype=U64))
        table = rng.integers(0, 2 ** 64, size=(1, 2, N), dtype=U64)
        old = ma.to_numpy(eng.leveled_lut(words, ma.to_device(table, eng.device), size, l, Bg))
        rot = [[2 * N - (1 << (steps - 1 - t))] for t in range(steps)]
        zero = [[0]] * steps
        auto = _create((zero, zero, zero, rot), N)
        acc = ma.to_numpy(eng.trlwe_automaton(auto, words.flip(1).contiguous(), ma.to_device(table, eng.device), l, Bg, 0))
        auto.close()
        for b in range(3):
            assert (oracle.trlwe_extract_tlwe(acc[b], 0) == old[b]).all(), "size %d, input %d: the one-state automaton differs from the leveled LUT's rotation" % (size, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["N2048 l4 Bg9", "N1024 l2 Bg8"])
def test_automaton_decrypts_on_the_device(eng, oracle, name):
    """Decryption.  The counter + parity machine over 16 steps on the device: the words of the restatement, and every state within 2^(64 - prec - 1) of its message
    (test_restatement_decrypts: the restatement alone meets that bound, also at 64 steps)."""
    S = _noise_case(oracle, name, 16)
    auto = _create(COUNTER, S["N"])
    got = _run(eng, S, auto, _dev_sel(eng, S["sel"][None]), S["init"][None])[0]
    auto.close()
    assert (got == S["out"]).all(), "%s: V_0 differs from the restatement" % name
    w = _worst(oracle, S, got)
    bound = 64 - S["prec"] - 1
    print("%s: 16 steps on the device: worst state 2^%.1f, bound 2^%d" % (name, _log2(w), bound))
    assert w < 2.0 ** bound, (name, _log2(w))


@pytest.mark.gpu
def test_automaton_with_selectors_from_the_circuit_bootstrap(eng, oracle):
    """Plumbing.  The key set-up of tests/test_lut_bits.py at its smallest set (lvl2's ring and gadget, the cheap private and packing keys): the word's selectors come
    from mosfhet_hip_circuit_bootstrap_3_dft_batch on LWE-encrypted bits and go into the call with no repacking in between.  That set's one-digit packing key leaves
    selectors too noisy to decrypt anything (tests/test_lut_bits.py compares words on it, too), so the chain is held to the words of the restatement on the
    oracle's circuit bootstrap of the same bits."""
    from test_lut_bits import _pipeline
    D = _pipeline(eng, oracle)
    N, l, Bg, steps, count = D["N"], D["l"], D["Bg"], 2, 2
    bits = np.stack([np.arange(b * D["size"], b * D["size"] + steps) for b in range(count)]).reshape(-1)      # the first two bits of each of the two inputs
    d_cts = D["d_cts"][eng.torch.from_numpy(bits).to(eng.device)].contiguous()
    sel = eng.circuit_bootstrap_3_dft(D["keys"]["reference"], D["kska"], D["pk"], d_cts).reshape(count, steps, 2 * l, 2, N)
    dft = [np.ascontiguousarray(D["want_dft1"][bits[b * steps:(b + 1) * steps]]) for b in range(count)]
    rng = np.random.default_rng(0xCB)
    tables = _tables(N, 3, 2, rng)
    init = rng.integers(0, 2 ** 64, size=(count, 3, 2, N), dtype=U64)
    auto = _create(tables, N)
    _assert_rows(_run(eng, dict(l=l, Bg=Bg), auto, sel, init), _want(oracle, tables, dft, init, l, Bg), "circuit-bootstrapped selectors")
    auto.close()


@pytest.mark.gpu
def test_automaton_streams_a_word_in_chunks(eng, oracle):
    """Streaming.  An 8-step word in two calls of 4, last half first, the first call's output fed back in as the second's initial vector, equals one call of 8 --
    which equals the restatement (3 states, 2 layers: the chunk length is a multiple of the period, so both chunks start on layer 0)."""
    import mosfhet_amd as ma
    N, l, Bg, states, count = 1024, 2, 8, 3, 2
    oracle.plan(N)
    rng = np.random.default_rng(0x57)
    tables = _tables(N, states, 2, rng)
    sel = rng.integers(0, 2 ** 64, size=(count, 8, 2 * l, 2, N), dtype=U64)
    init = rng.integers(0, 2 ** 64, size=(count, states, 2, N), dtype=U64)
    auto = _create(tables, N)
    d_sel, d_init = _dev_sel(eng, sel), ma.to_device(init, eng.device)
    whole = ma.to_numpy(eng.trlwe_automaton(auto, d_sel, d_init, l, Bg))
    _assert_rows(whole, _want(oracle, tables, _dfts(oracle, sel, l), init, l, Bg), "one call of 8")
    mid = eng.trlwe_automaton(auto, d_sel[:, 4:].contiguous(), d_init, l, Bg)
    _assert_rows(ma.to_numpy(eng.trlwe_automaton(auto, d_sel[:, :4].contiguous(), mid, l, Bg)), whole, "two calls of 4")
    _assert_rows(ma.to_numpy(eng.trlwe_automaton(auto, d_sel[:, :4].contiguous(), mid, l, Bg, 2)), whole[:, 2], "two calls of 4, one state")
    auto.close()


@pytest.mark.gpu
def test_automaton_through_the_host_structs(native_lib, tmp_path):
    """tests/c/trlwe_automaton.c: mosfhet_trlwe_automaton on 3 inputs equals the backward CMUX chain written against include/mosfhet.h (trlwe_mul_by_xai / trlwe_sub /
    trgsw_mul_trlwe_DFT / trlwe_from_DFT / trlwe_add) word for word -- every state, one state, a batch of one, a shared initial vector -- and decrypts."""
    exe = str(tmp_path / "trlwe_automaton")
    _compile_c(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_automaton ok" in r.stdout, r.stdout[-3000:]
