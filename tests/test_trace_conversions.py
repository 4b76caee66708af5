"""The LWE -> TRLWE switch by the trace and the gadget -> TRGSW conversion on the device (include/mosfhet_hip.h: mosfhet_hip_tlwe_trace_pack_batch,
mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch, mosfhet_hip_trgsw_from_gadget_batch, mosfhet_hip_trace_plan; mosfhet_amd/csrc/capi_trace.inc, trace_kernels.h;
include/mosfhet_compat.h: mosfhet_tlwe_trace_pack).

Expected words come from tests/trace_reference.py, which composes oracle primitives that are each held to the reference, in the order of the reference's
trlwe_packing1_keyswitch_CDKS21, trlwe_RLWE_priv_keyswitch and trgsw_from_gadget.  Every comparison of device words with the helper is == on all words.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
_CACHE = {}
U64 = np.uint64


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _dist(oracle, a, b):
    return float(oracle.torus_dist(np.ascontiguousarray(a), np.ascontiguousarray(b)).max())


def _case(oracle, N, t, base_bit, count, sigma):
    """Key, key rows and samples of one shape, made once and left unchanged: dict(s, rows [log2 N + 2][t][2][N] torus words -- the log2 N trace keys, then the two
    entries of the gadget key (v = -s) --, dft = their transforms in the oracle's order, msgs, cts [count][N + 1] under s as the extracted ring key)"""
    import trace_reference as R
    key = (N, t, base_bit, count, sigma)
    if key not in _CACHE:
        rng = oracle.Rng(0x7ACE + 131 * N + 17 * t + base_bit)
        s = oracle.gen_binary_key(rng, N)
        rows = np.concatenate([R.gen_trace_keys(oracle, rng, s, t, base_bit, sigma), R.gen_gadget_keys(oracle, rng, s, t, base_bit, sigma)])
        msgs = (rng.words(count) % U64(16)) << U64(60)
        cts = np.stack([oracle.tlwe_sample(rng, m, s, sigma) for m in msgs])
        _CACHE[key] = dict(s=s, rows=rows, dft=oracle.ks_to_dft(rows), msgs=msgs, cts=cts, rng=rng)
    return _CACHE[key]


def _want_trace(oracle, D, t, base_bit, N, entry0=0):
    import trace_reference as R
    key = ("trace", id(D), entry0)
    if key not in _CACHE:
        _CACHE[key] = R.trace_pack_batch(oracle, D["cts"], D["dft"][entry0:entry0 + R.log2n(N)], t, base_bit, N)
    return _CACHE[key]


def _gadget_case(oracle, D, N, l, Bg_bit, count, sigma, seed=None):
    """gadget rows [count][l][2][N] of the bits 0, 1, 1, ... under D's key, and the helper's TRGSWs in the torus domain [count][2l][2][N].  With a seed the noise
    comes from a generator of the case's own, so that the rows do not depend on which tests drew from D's generator before."""
    import trace_reference as R
    key = ("gadget", id(D), l, Bg_bit, count, seed)
    if key not in _CACHE:
        rng = D["rng"] if seed is None else oracle.Rng(seed)
        bits = [0, 1, 1, 0, 1][:count]
        g = np.empty((count, l, 2, N), dtype=U64)
        for c, m in enumerate(bits):
            for i in range(l):
                msg = np.zeros(N, dtype=U64)
                msg[0] = U64(m) << U64(64 - (i + 1) * Bg_bit)
                g[c, i] = oracle.trlwe_sample(rng, msg, D["s"].reshape(1, N), sigma)
        _CACHE[key] = dict(bits=bits, gadget=g)
    return _CACHE[key]


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
TRACE_SHAPES = [(1024, 4, 9, 2.0 ** -45), (2048, 4, 9, 2.0 ** -50)]


def test_trace_step_is_eval_automorphism(oracle):
    """One step of the helper (poly_permute on both components, trlwe_keyswitch, add) equals acc + oracle.trlwe_eval_automorphism(acc, gen, key) bit for bit, at every
    step of a trace at N = 1024 (t 4, base_bit 9) and (t 2, base_bit 8): the helper is the composition the device's existing automorphism call computes."""
    import trace_reference as R
    for t, bb in ((4, 9), (2, 8)):
        N = 1024
        D = _case(oracle, N, t, bb, 3, 2.0 ** -45)
        acc = R.embed(D["cts"][0], N)
        for j, gen in enumerate(R.trace_gens(N)):
            nxt = R.trace_step(oracle, acc, gen, D["dft"][j], t, bb)
            with np.errstate(over="ignore"):
                other = acc + oracle.trlwe_eval_automorphism(acc, gen, np.ascontiguousarray(D["dft"][j]), t, bb)
            assert (nxt == other).all(), (t, bb, j)
            acc = nxt
        assert (acc == _want_trace(oracle, D, t, bb, N)[0]).all()


@pytest.mark.parametrize("shape", TRACE_SHAPES)
def test_trace_helper_decrypts(oracle, shape):
    """The helper's trace of samples under the extracted ring key has phase N m at coefficient 0 and 0 elsewhere, within 2^58 -- the reference's own bound
    (test/tests.c:850).  Measured with this file's keys: N 1024, t 4, base_bit 9, sigma 2^-45: 2^40.7; N 2048, sigma 2^-50: 2^42.0 (printed again by every run; other keys of the same
    shapes gave 2^42.1 and 2^40.3).
    A zero-mask sample gives a = 0, b = N in.b X^0 exactly: every digit is zero."""
    import trace_reference as R
    N, t, bb, sigma = shape
    D = _case(oracle, N, t, bb, 3, sigma)
    want = _want_trace(oracle, D, t, bb, N)
    worst = 0.0
    for c in range(3):
        exp = np.zeros(N, dtype=U64)
        with np.errstate(over="ignore"):
            exp[0] = D["msgs"][c] * U64(N)
        worst = max(worst, _dist(oracle, oracle.trlwe_phase(want[c], D["s"].reshape(1, N)), exp))
    print("N %d t %d bb %d: phase - N m = 2^%.1f" % (N, t, bb, _log2(worst)))
    assert worst <= 2.0 ** 58, _log2(worst)
    zero = np.zeros(N + 1, dtype=U64)
    zero[N] = U64(0x0123456789ABCDEF)
    z = R.trace_pack(oracle, zero, D["dft"], t, bb, N)
    with np.errstate(over="ignore"):
        assert (z[0] == 0).all() and z[1, 0] == zero[N] * U64(N) and (z[1, 1:] == 0).all()


def test_gadget_helper_decrypts_and_selects(oracle):
    """N = 1024, l = 2, Bg_bit = 8, key t = 4, base_bit = 9, sigma 2^-45.  Rows i < l of the helper's TRGSW decrypt to -s m 2^(64 - (i + 1) Bg_bit): measured 2^38.1
    .. 2^39.9 away.  The bound is 2^43: the digits cut the mask at 2^(64 - 36), a rounding error uniform in +-2^27 per coefficient (variance 2^54 / 3), multiplied by s v = -s s,
    whose N coefficients have mean squares of about (N / 4)^2 / 3 -- variance 2^54 / 3 x N x 2^16 / 3 = 2^76.8, deviation 2^38.4, four deviations for the maximum
    over N coefficients 2^40.4, and 2.6 bits of room for other keys; the key's own noise (2^19 per row word) adds 2^35.  oracle.external_product with the assembled
    TRGSW of m = 1 selects a message on multiples of 1/16 with error 2^52.5 (measured), of m = 0 gives 0 within 2^50.0; asserted below 2^57 = half a slot less two bits."""
    import trace_reference as R
    N, l, Bg, t, bb, sigma = 1024, 2, 8, 4, 9, 2.0 ** -45
    D = _case(oracle, N, t, bb, 3, sigma)
    G = _gadget_case(oracle, D, N, l, Bg, 3, sigma)
    s1 = D["s"].reshape(1, N)
    kd = D["dft"][R.log2n(N):]
    msg = D["rng"].words(N) & U64(0xF000000000000000)
    ct = oracle.trlwe_sample(D["rng"], msg, s1, sigma)
    for c, m in enumerate(G["bits"]):
        trgsw = R.trgsw_from_gadget(oracle, G["gadget"][c], kd, t, bb)
        for i in range(l):
            with np.errstate(over="ignore"):
                exp = (U64(0) - D["s"]) * (U64(m) << U64(64 - (i + 1) * Bg))
            d = _dist(oracle, oracle.trlwe_phase(trgsw[i], s1), exp)
            print("bit %d row %d: 2^%.1f from -s m 2^(64 - %d)" % (m, i, _log2(d), (i + 1) * Bg))
            assert d < 2.0 ** 43, (c, i, _log2(d))
        ep = oracle.external_product(ct, oracle.trgsw_to_dft(trgsw, 1, l), l, Bg)
        d = _dist(oracle, oracle.trlwe_phase(ep, s1), msg * U64(m))
        print("bit %d: external product 2^%.1f from m x message" % (m, _log2(d)))
        assert d < 2.0 ** 57, (c, _log2(d))


def test_trace_symbols_and_argument_checks(native_lib):
    """The library exports the four entry points and the host face, the binding its functions; every refusal returns MOSFHET_HIP_EINVAL with a message naming the
    argument -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); count == 0 is OK.  What a call reads off its key set
    (the ring, a set too short for entry0) is checked by the function the calls check with, mosfhet_hip_trace_plan."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_tlwe_trace_pack_batch", "mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch", "mosfhet_hip_trgsw_from_gadget_batch", "mosfhet_hip_trace_plan",
                 "mosfhet_tlwe_trace_pack"):
        assert hasattr(native_lib, name), name
    for name in ("tlwe_trace_pack", "trlwe_rlwe_priv_keyswitch", "trgsw_from_gadget"):
        assert hasattr(engine.Engine, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    for name in ("mosfhet_hip_tlwe_trace_pack_batch", "mosfhet_hip_trlwe_rlwe_priv_keyswitch_batch"):
        f = getattr(native_lib, name)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert f(None, fake, 0, fake, fake, 1, None) == EINVAL and "ctx" in err()
        assert f(fake, None, 0, fake, fake, 1, None) == EINVAL and "tks" in err()
        assert f(fake, fake, 0, fake, fake, -1, None) == EINVAL and "count = -1" in err()
        assert f(fake, fake, -1, fake, fake, 1, None) == EINVAL and "entry0 = -1" in err()
        assert f(fake, fake, -2, fake, fake, 0, None) == EINVAL and "entry0 = -2" in err()       # ... before count == 0 is accepted
        assert f(fake, fake, 0, fake, fake, 0, None) == 0                                          # count == 0: nothing to do, no handle read
        assert f(fake, fake, 5, None, None, 0, None) == 0
        assert f(fake, fake, 0, None, fake, 1, None) == EINVAL and "null buffer" in err()
        assert f(fake, fake, 0, fake, None, 1, None) == EINVAL and "null buffer" in err()
    g = native_lib.mosfhet_hip_trgsw_from_gadget_batch
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert g(None, fake, 0, fake, fake, 2, 1, None) == EINVAL and "ctx" in err()
    assert g(fake, None, 0, fake, fake, 2, 1, None) == EINVAL and "tks" in err()
    assert g(fake, fake, 0, fake, fake, 2, -1, None) == EINVAL and "count = -1" in err()
    assert g(fake, fake, -1, fake, fake, 2, 1, None) == EINVAL and "entry0 = -1" in err()
    assert g(fake, fake, 0, fake, fake, 0, 1, None) == EINVAL and "l = 0" in err()
    assert g(fake, fake, 0, fake, fake, 7, 1, None) == EINVAL and "l = 7" in err()
    assert g(fake, fake, 0, fake, fake, 7, 0, None) == EINVAL and "l = 7" in err()
    assert g(fake, fake, 0, fake, fake, 6, 0, None) == 0
    assert g(fake, fake, 0, None, fake, 2, 1, None) == EINVAL and "null buffer" in err()
    p = native_lib.mosfhet_hip_trace_plan
    p.argtypes = [C.c_int] * 8 + [C.c_void_p]
    plan = (C.c_longlong * 6)()
    assert p(0, 1024, 4, 9, 10, 0, 0, 1, None) == EINVAL and "plan" in err()
    assert p(3, 1024, 4, 9, 10, 0, 0, 1, plan) == EINVAL and "kind = 3" in err()
    for kind in (0, 1, 2):
        assert p(kind, 512, 4, 9, 12, 0, 2, 1, plan) == EINVAL and "N = 512" in err()
        assert p(kind, 1000, 4, 9, 12, 0, 2, 1, plan) == EINVAL and "N = 1000" in err()
        assert p(kind, 8192, 4, 9, 14, 0, 2, 1, plan) == EINVAL and "N = 8192" in err()
        assert p(kind, 1024, 0, 9, 12, 0, 2, 1, plan) == EINVAL and "t = 0" in err()
        assert p(kind, 1024, 8, 8, 12, 0, 2, 1, plan) == EINVAL and "base_bit = 8" in err()
        assert p(kind, 1024, 4, 9, 12, 0, 2, -1, plan) == EINVAL and "count = -1" in err()
        assert p(kind, 1024, 4, 9, 12, -1, 2, 1, plan) == EINVAL and "entry0 = -1" in err()
        assert p(kind, 1024, 4, 9, 0, 0, 2, 1, plan) == EINVAL and "holds 0 entries" in err()
    # a set too short: the trace reads log2 N entries from entry0 on, the private switch and the gadget conversion two
    for N, steps in ((1024, 10), (2048, 11), (4096, 12)):
        assert p(0, N, 4, 9, steps - 1, 0, 0, 1, plan) == EINVAL and "holds %d entries" % (steps - 1) in err() and "entry0 + %d" % steps in err()
        assert p(0, N, 4, 9, steps + 1, 2, 0, 1, plan) == EINVAL and "entry0 = 2" in err()
        assert p(0, N, 4, 9, steps + 2, 2, 0, 5, plan) == 0 and list(plan) == [steps, 5, N // 16, steps * 4, steps * 2, steps * 4 * N * 16]
    for kind in (1, 2):
        assert p(kind, 1024, 4, 9, 1, 0, 2, 1, plan) == EINVAL and "holds 1 entries" in err()
        assert p(kind, 1024, 4, 9, 12, 11, 2, 1, plan) == EINVAL and "entry0 = 11" in err()
        assert p(kind, 1024, 4, 9, 12, 10, 2, 3, plan) == 0 and plan[0] == 2 and plan[1] == (3 if kind == 1 else 6)
    assert p(2, 1024, 4, 9, 12, 10, 0, 1, plan) == EINVAL and "l = 0" in err()
    assert p(2, 1024, 4, 9, 12, 10, 7, 1, plan) == EINVAL and "l = 7" in err()
    assert p(2, 1024, 4, 9, 12, 10, 6, 2 ** 31 - 1, plan) == EINVAL and "one launch" in err()
    assert p(0, 1024, 4, 9, 12, 0, 0, 0, plan) == 0 and plan[1] == 0                              # count == 0: no team
    assert engine.trace_plan("trgsw_from_gadget", 2048, 4, 9, 2, 0, l=4, count=3) == dict(entries_read=2, teams=12, threads=128, forwards=12, inverses=4, key_bytes=2 * 4 * 2048 * 16)
    with pytest.raises(engine.MosfhetHipError, match="holds 10 entries"):
        engine.trace_plan("trace_pack", 2048, 4, 9, 10)


def test_trace_kernels_of_the_build(native_lib):
    """tools/kernel_table.py lists one instantiation per ring of trace_conversions_kernel (the three calls name their work at run time), all without scratch;
    tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    mine = sorted((r for r in kernel_table.table() if r["name"].startswith("trace_conversions_kernel")), key=lambda r: r["lds"])
    for r in mine:
        print("%-70s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    assert len(mine) == 3 and "1024" in mine[0]["name"] and "2048" in mine[1]["name"] and "4096" in mine[2]["name"], [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0, r
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    assert ", 0 violations" in report, report


def _compile_c(tmp_path):
    exe = str(tmp_path / "trace_conversions")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trace_conversions.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_trace_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trace_conversions.c compiles against include/mosfhet.h and links against the built library (its device part: test_trace_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _tks(eng, D, base_bit):
    if "tks" not in D or D["tks"].engine is not eng:
        D["tks"] = eng.load_trlwe_ks_keys(D["rows"], base_bit)
    return D["tks"]


def _run_trace(eng, tks, cts, entry0=0):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.tlwe_trace_pack(tks, ma.to_device(cts, eng.device), entry0))


def _same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), "%s: %d words differ, samples %s" % (what, (got != want).sum(), sorted(set(np.nonzero(got != want)[0]))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [(2, 8), (3, 10), (4, 9)])
def test_trace_bit_exact_1024(eng, oracle, tb):
    """N = 1024: batches of 1, 3 and 67 samples equal the helper on every word, with entry0 = 0 and with entry0 = 2 on the same set (log2 N + 2 entries: the helper
    then composes entries 2 .. 11 in the same way).  Sample i of the batch of 67 equals the same sample alone."""
    t, bb = tb
    N = 1024
    D = _case(oracle, N, t, bb, 67, 2.0 ** -45)
    tks = _tks(eng, D, bb)
    for entry0 in (0, 2):
        want = _want_trace(oracle, D, t, bb, N, entry0)
        whole = _run_trace(eng, tks, D["cts"], entry0)
        _same(whole, want, "count 67, entry0 %d" % entry0)
        for count in (1, 3):
            _same(_run_trace(eng, tks, D["cts"][:count], entry0), want[:count], "count %d, entry0 %d" % (count, entry0))
    whole = _run_trace(eng, tks, D["cts"])
    for i in (0, 1, 33, 65, 66):
        _same(_run_trace(eng, tks, D["cts"][i:i + 1]), whole[i:i + 1], "sample %d alone" % i)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2048, 4, 9, 2), (4096, 2, 8, 1)])
def test_trace_bit_exact_wide_rings(eng, oracle, shape):
    """N = 2048, count 2 (11 steps, 128 threads) and N = 4096, count 1 (12 steps, 256 threads): == the helper."""
    N, t, bb, count = shape
    D = _case(oracle, N, t, bb, count, 2.0 ** -50)
    _same(_run_trace(eng, _tks(eng, D, bb), D["cts"]), _want_trace(oracle, D, t, bb, N), "N %d" % N)


@pytest.mark.gpu
def test_trace_edge_rows_sentinel_and_input(eng, oracle):
    """One batch at N = 1024 (t 4, base_bit 9): a zero mask -- compared with the exact words a = 0, b = N in.b X^0, not only with the helper --; in.b = 0; mask words
    all 0 / 2^63 / 2^64 - 1 and words on both sides of every digit boundary of the key's (t, base_bit); a mask that is non-zero only at index 1 and only at index
    N - 1 (the reversal and the sign of the embedding).  The output buffer is one sample longer and sentinel-filled: the tail stays untouched; the input is unchanged."""
    import torch
    import mosfhet_amd as ma
    import trace_reference as R
    N, t, bb = 1024, 4, 9
    D = _case(oracle, N, t, bb, 67, 2.0 ** -45)
    tks = _tks(eng, D, bb)
    cts = D["cts"][:8].copy()
    cts[0, :N] = 0
    cts[1, N] = 0
    cts[2, :N] = U64(1) << U64(63)
    cts[3, :N] = U64(0xFFFFFFFFFFFFFFFF)
    edges = R.digit_boundary_words(t, bb)
    cts[4, :N] = edges[np.arange(N) % len(edges)]
    cts[5, :N] = 0
    cts[5, 1] = U64(0x3141592653589793)
    cts[6, :N] = 0
    cts[6, N - 1] = U64(0x2718281828459045)
    cts[7, :N] = 0
    cts[7, N] = 0
    d_in = ma.to_device(cts, eng.device)
    before = d_in.clone()
    sentinel = 0x5EA75EA75EA75EA7
    d_out = torch.full((9, 2, N), sentinel, dtype=torch.int64, device=eng.device)
    eng.tlwe_trace_pack(tks, d_in, 0, out=d_out[:8])
    torch.cuda.synchronize(eng.device)
    got = ma.to_numpy(d_out)
    assert (got[8] == U64(sentinel)).all(), "the call wrote past its last sample"
    assert torch.equal(d_in, before), "the call changed its input"
    want = R.trace_pack_batch(oracle, cts, D["dft"][:R.log2n(N)], t, bb, N)
    _same(got[:8], want, "edge rows")
    with np.errstate(over="ignore"):
        assert (got[0, 0] == 0).all() and got[0, 1, 0] == cts[0, N] * U64(N) and (got[0, 1, 1:] == 0).all()
    assert (got[7] == 0).all()
    # the embedding alone (what the first step permutes): a[N - 1] = -in.a[1], a[1] = -in.a[N - 1]
    e5, e6 = R.embed(cts[5], N), R.embed(cts[6], N)
    with np.errstate(over="ignore"):
        assert e5[0, N - 1] == U64(0) - cts[5, 1] and e6[0, 1] == U64(0) - cts[6, N - 1]


@pytest.mark.gpu
def test_trace_against_the_device_composition(eng, oracle):
    """The fused call equals today's device composition on the same key set: the embedding, then log2 N rounds of mosfhet_hip_trlwe_eval_automorphism_entry_batch
    (gen = N / 2^j + 1, entry j) and a word-wise add.  N = 1024 (t 4, base_bit 9), 67 samples; N = 2048, 2 samples."""
    import mosfhet_amd as ma
    import trace_reference as R
    for N, t, bb, count, sigma in ((1024, 4, 9, 67, 2.0 ** -45), (2048, 4, 9, 2, 2.0 ** -50)):
        D = _case(oracle, N, t, bb, count, sigma)
        tks = _tks(eng, D, bb)
        acc = ma.to_device(np.stack([R.embed(c, N) for c in D["cts"]]), eng.device)
        for j, gen in enumerate(R.trace_gens(N)):
            acc = acc + eng.trlwe_eval_automorphism_entry(tks, j, acc, gen)
        _same(_run_trace(eng, tks, D["cts"]), ma.to_numpy(acc), "N %d against the composition" % N)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TRACE_SHAPES)
def test_trace_decrypts(eng, oracle, shape):
    """The shapes of test_trace_helper_decrypts on the device: the phase is N m at coefficient 0 and 0 elsewhere within the helper's own error (computed here and
    printed: 2^40.7 at N = 1024, 2^42.0 at N = 2048 as measured) plus two bits, and within 2^58."""
    N, t, bb, sigma = shape
    D = _case(oracle, N, t, bb, 3, sigma)
    got, want = _run_trace(eng, _tks(eng, D, bb), D["cts"]), _want_trace(oracle, D, t, bb, N)
    s1 = D["s"].reshape(1, N)
    for c in range(3):
        exp = np.zeros(N, dtype=U64)
        with np.errstate(over="ignore"):
            exp[0] = D["msgs"][c] * U64(N)
        helper = _dist(oracle, oracle.trlwe_phase(want[c], s1), exp)
        d = _dist(oracle, oracle.trlwe_phase(got[c], s1), exp)
        print("N %d sample %d: device 2^%.1f, helper 2^%.1f from N m" % (N, c, _log2(d), _log2(helper)))
        assert d <= 4 * max(helper, 1.0) and d <= 2.0 ** 58, (c, _log2(d), _log2(helper))


def _priv_inputs(oracle, D, N, count, sigma, seed=None):
    """count TRLWE samples under D's key; with a seed, from a generator of the case's own (see _gadget_case)"""
    key = ("priv", id(D), count, seed)
    if key not in _CACHE:
        s1, rng = D["s"].reshape(1, N), D["rng"] if seed is None else oracle.Rng(seed)
        _CACHE[key] = np.stack([oracle.trlwe_sample(rng, rng.words(N) & U64(0xF000000000000000), s1, sigma) for _ in range(count)])
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 4, 9, 5), (1024, 3, 10, 5), (2048, 4, 9, 2)])
def test_rlwe_priv_keyswitch_bit_exact(eng, oracle, shape):
    """The private switch equals the helper (-(trlwe_keyswitch((in.b, 0), K1)) + trlwe_keyswitch((in.a, 0), K0)) on every word: N = 1024, count 5, t = 4 and 3;
    N = 2048, count 2; once more with d_out = d_in, which gives the same words; the input of the first call is unchanged."""
    import mosfhet_amd as ma
    import trace_reference as R
    N, t, bb, count = shape
    D = _case(oracle, N, t, bb, 67 if N == 1024 else 2, 2.0 ** -45 if N == 1024 else 2.0 ** -50)
    tks, e0 = _tks(eng, D, bb), R.log2n(N)
    ins = _priv_inputs(oracle, D, N, count, 2.0 ** -45)
    want = np.stack([R.rlwe_priv_keyswitch(oracle, c, D["dft"][e0:], t, bb) for c in ins])
    d_in = ma.to_device(ins, eng.device)
    _same(ma.to_numpy(eng.trlwe_rlwe_priv_keyswitch(tks, d_in, e0)), want, "N %d t %d" % (N, t))
    assert (ma.to_numpy(d_in) == ins).all()
    eng.trlwe_rlwe_priv_keyswitch(tks, d_in, e0, out=d_in)
    _same(ma.to_numpy(d_in), want, "N %d t %d in place" % (N, t))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 2, 8, 3, 2.0 ** -45), (2048, 4, 8, 1, 2.0 ** -50)])
def test_trgsw_from_gadget(eng, oracle, shape):
    """N = 1024, l = 2, count 3 and N = 2048, l = 4, count 1 (key t 4, base_bit 9).  The selectors compare == as doubles with mosfhet_hip_torus_to_dft_batch of
    (the words of the private switch, the gadget rows); the private-switch words equal the helper.  Then the selector goes through mosfhet_hip_cmux_batch as a key
    handle (a view of the DFT rows; mosfhet_hip_bsk_create_from_device, which takes the same rows in the torus domain, gives the same words) and both selector
    values, 0 and 1, decrypt to the chosen input within 2^57 (half a slot of 1/16 less two bits)."""
    import torch
    import mosfhet_amd as ma
    import trace_reference as R
    N, l, Bg, count, sigma = shape
    t, bb = 4, 9
    D = _case(oracle, N, t, bb, 67 if N == 1024 else 2, sigma)
    G = _gadget_case(oracle, D, N, l, Bg, count, sigma)
    tks, e0 = _tks(eng, D, bb), R.log2n(N)
    d_g = ma.to_device(G["gadget"], eng.device)
    sel = eng.trgsw_from_gadget(tks, d_g, e0)
    assert sel.shape == (count, 2 * l, 2, N) and sel.dtype == torch.float64
    switched = eng.trlwe_rlwe_priv_keyswitch(tks, d_g.view(count * l, 2, N), e0).view(count, l, 2, N)
    _same(ma.to_numpy(switched), np.stack([R.trgsw_from_gadget(oracle, g, D["dft"][e0:], t, bb)[:l] for g in G["gadget"]]), "the private switch of the gadget rows")
    words = torch.cat([switched, d_g], dim=1).contiguous()                       # [count][2l][2][N], the TRGSW in the torus domain
    want = eng.torus_to_dft(words.view(-1, N)).view(count, 2 * l, 2, N)
    torch.cuda.synchronize(eng.device)
    assert torch.equal(sel, want), "%d doubles differ" % int((sel != want).sum())
    s1 = D["s"].reshape(1, N)
    msgs = [D["rng"].words(N) & U64(0xF000000000000000) for _ in range(2)]
    in0, in1 = [ma.to_device(oracle.trlwe_sample(D["rng"], m, s1, sigma)[None], eng.device) for m in msgs]
    seen = set()
    for c, m in enumerate(G["bits"]):
        view = eng.bootstrap_key_view(sel[c:c + 1], 1, l, Bg)
        out = eng.cmux(view, 0, in0, in1)
        made = eng.load_bootstrap_key_device(words[c:c + 1], 1, l, Bg)
        assert torch.equal(out, eng.cmux(made, 0, in0, in1)), "the view and the key made of the torus words select differently"
        d = _dist(oracle, oracle.trlwe_phase(ma.to_numpy(out)[0], s1), msgs[m])
        print("N %d selector %d (bit %d): 2^%.1f from input %d" % (N, c, m, _log2(d), m))
        assert d < 2.0 ** 57, (c, m, _log2(d))
        view.free()
        made.free()
        seen.add(m)
    if count > 1:
        assert seen == {0, 1}


@pytest.mark.gpu
def test_trace_refusals_on_the_device(eng, oracle):
    """A set too short for entry0, d_out overlapping d_in, a shifted overlap of the private switch and a key of another context are refused with MOSFHET_HIP_EINVAL;
    a refused call writes nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, t, bb = 1024, 4, 9
    D = _case(oracle, N, t, bb, 67, 2.0 ** -45)
    tks = _tks(eng, D, bb)
    d_in = ma.to_device(D["cts"][:2], eng.device)
    out = torch.full((2, 2, N), 7, dtype=torch.int64, device=eng.device)
    with pytest.raises(engine.MosfhetHipError, match="holds 12 entries"):
        eng.tlwe_trace_pack(tks, d_in, 3, out=out)
    with pytest.raises(engine.MosfhetHipError, match="holds 12 entries"):
        eng.trlwe_rlwe_priv_keyswitch(tks, out, 11, out=out)
    with pytest.raises(engine.MosfhetHipError, match="l = 7"):
        eng.trgsw_from_gadget(tks, torch.zeros(1, 7, 2, N, dtype=torch.int64, device=eng.device), 10)
    buf = torch.zeros(2 * (N + 1) + 2 * 2 * N, dtype=torch.int64, device=eng.device)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.tlwe_trace_pack(tks, buf[:2 * (N + 1)].view(2, N + 1), 0, out=buf[N:N + 4 * N].view(2, 2, N))
    with pytest.raises(engine.MosfhetHipError, match="overlaps d_in"):
        eng.trlwe_rlwe_priv_keyswitch(tks, buf[:4 * N].view(2, 2, N), 10, out=buf[N:5 * N].view(2, 2, N))
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.tlwe_trace_pack(tks, d_in, 0, out=out)
    finally:
        other.close()
    torch.cuda.synchronize(eng.device)
    assert (out == 7).all() and (buf == 0).all(), "a refused call wrote to its output"


@pytest.mark.gpu
def test_trace_host_face(native_lib, tmp_path):
    """tests/c/trace_conversions.c: mosfhet_tlwe_trace_pack of 5 samples on host structs equals five single trlwe_packing1_keyswitch_CDKS21 calls word for word, the
    phases are N m within 2^58; trlwe_RLWE_priv_keyswitch and trgsw_from_gadget select through an external product."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trace_conversions ok" in r.stdout, r.stdout


# ---------------------------------------------------------------- value edges, uncovered instantiations, run contexts ----------------------------------------------------------------
EXTREME_KEY_SHAPES = [(4, 9), (2, 8)]


def _ks_offset(t, base_bit):
    """2^(63 - t base_bit) + sum_i 2^(63 - i base_bit): the rounding offset of the key switch's decomposition (trace_kernels.h: `off`)"""
    return (1 << (63 - t * base_bit)) + sum(1 << (63 - i * base_bit) for i in range(t))


def _ks_target(t, base_bit, field):
    """the torus word whose t digits all come out of the base_bit-bit slot value `field`: 0 -> every digit -2^(base_bit-1), 2^base_bit - 1 -> every digit 2^(base_bit-1) - 1"""
    return (sum(field << (64 - (i + 1) * base_bit) for i in range(t)) - _ks_offset(t, base_bit)) % 2 ** 64


def _extreme_case(oracle, t, base_bit):
    """N = 1024.  A key set of log2 N + 2 entries whose rows are all -2^63, all 2^63 - 1 and the two alternating by coefficient, in turn, with entry log2 N - 1 -- the
    trace's last step -- all zero.  Masks: words whose digits are all at the bottom / all at the top (the offset construction with the key switch's offset), such
    words with the signs the embedding and the first permutation (gen = N + 1: coefficient i times (-1)^i) take off again, so that the FIRST STEP decomposes exactly
    them; tests/trace_reference.py::digit_boundary_words; all 2^64 - 1.  The same words as TRLWE samples for the private switch, and paired into gadgets of l = 2."""
    import trace_reference as R
    key = ("extreme", t, base_bit)
    if key in _CACHE:
        return _CACHE[key]
    N = 1024
    steps = R.log2n(N)
    lo, hi = U64(1 << 63), U64((1 << 63) - 1)
    rows = np.empty((steps + 2, t, 2, N), dtype=U64)
    for e in range(steps + 2):
        rows[e] = (lo, hi, lo)[e % 3]
        if e % 3 == 2:
            rows[e, :, :, ::2] = hi
    rows[steps - 1] = 0
    bottom, top = _ks_target(t, base_bit, 0), _ks_target(t, base_bit, (1 << base_bit) - 1)
    edges = R.digit_boundary_words(t, base_bit)
    masks = np.empty((7, N), dtype=U64)
    masks[0], masks[1] = U64(bottom), U64(top)
    masks[2] = U64(bottom)
    masks[2, ::2] = U64(top)
    for k, word in ((3, bottom), (4, top)):            # in.a[0] = w, in.a[i] = w for odd i and -w for even i: the first step's digit words are all w
        masks[k] = U64(word)
        masks[k, 2::2] = U64((-word) % 2 ** 64)
    masks[5] = edges[np.arange(N) % len(edges)]
    masks[6] = U64(0xFFFFFFFFFFFFFFFF)
    rng = np.random.default_rng(0xE7 + t)
    cts = np.concatenate([masks, rng.integers(0, 2 ** 64, size=(7, 1), dtype=U64)], axis=1)
    trlwe = np.stack([np.stack([masks[k], masks[(k + 1) % 7]]) for k in (0, 1, 2, 5, 6, 3)])       # [6][2][N]
    _CACHE[key] = dict(rows=rows, dft=oracle.ks_to_dft(rows), cts=cts, trlwe=trlwe, gadget=trlwe.reshape(3, 2, 2, N), bottom=bottom, top=top)
    return _CACHE[key]


@pytest.mark.parametrize("tb", EXTREME_KEY_SHAPES)
def test_extreme_masks_decompose_to_extreme_digits(oracle, tb):
    """oracle.poly_decompose_i on the masks of the extreme-key case: the target words give every one of the t digits -2^(base_bit-1) resp. 2^(base_bit-1) - 1; the
    signed masks give exactly those words after the embedding and the first step's permutation, i.e. the trace's first step decomposes extreme digits only.  The
    helper runs on the key rows of +-2^63, and with the zero entry its last step is (a, b + b(X^gen)) exactly: the switch of the permuted sample subtracts nothing."""
    import trace_reference as R
    t, bb = tb
    N = 1024
    E = _extreme_case(oracle, t, bb)
    lo, hi = -(1 << (bb - 1)), (1 << (bb - 1)) - 1
    for k, want in ((0, lo), (1, hi), (3, lo), (4, hi)):
        first = np.ascontiguousarray(E["cts"][k, :N]) if k < 2 else oracle.poly_permute(np.ascontiguousarray(R.embed(E["cts"][k], N)[0]), N + 1)
        for i in range(t):
            assert (oracle.poly_decompose_i(first, bb, t, i).view(np.int64) == want).all(), (tb, k, i)
    print("t %d base_bit %d: largest |key double| 2^%.1f, the sums reach t N 2^(base_bit-1) 2^63 = 2^%.1f" % (t, bb, _log2(np.abs(E["dft"]).max()), np.log2(t * N) + bb - 1 + 63))
    steps = R.log2n(N)
    acc = R.embed(E["cts"][3], N)
    for j, gen in enumerate(R.trace_gens(N)[:-1]):
        acc = R.trace_step(oracle, acc, gen, E["dft"][j], t, bb)
    last = R.trace_step(oracle, acc, R.trace_gens(N)[-1], E["dft"][steps - 1], t, bb)
    gen = R.trace_gens(N)[-1]
    with np.errstate(over="ignore"):      # the switch of (a, b)(X^gen) with a zero entry is (0, b(X^gen)): the mask stays, the body takes its own permutation
        exact = np.stack([acc[0], acc[1] + oracle.poly_permute(np.ascontiguousarray(acc[1]), gen)])
    assert (last == exact).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tb", EXTREME_KEY_SHAPES)
def test_extreme_key_rows(eng, oracle, tb):
    """N = 1024, key rows of -2^63 / 2^63 - 1 / alternating and one zero entry, masks with every digit at the bottom or the top, at the digit boundaries and all
    2^64 - 1 (_extreme_case): the trace equals tests/trace_reference.py::trace_pack_batch on oracle.ks_to_dft of the same rows, the private switch equals
    rlwe_priv_keyswitch on them (entries log2 N, log2 N + 1, and entries log2 N - 1, log2 N whose first is the zero entry), trgsw_from_gadget at l = 2 equals the
    doubles of torus_to_dft of (private-switch words, gadget rows).  The last step without the oracle's key switch: it uses the zero entry and subtracts nothing
    (the switch of the permuted sample with it is (0, b(X^gen))), so the device's result is (a, b + b(X^gen)) of the accumulator in front of it, word for word.
    That accumulator is still the oracle's: R.trace_step, key switch included, builds it over the log2 N - 1 earlier steps; only the last step is oracle-free."""
    import torch
    import mosfhet_amd as ma
    import trace_reference as R
    t, bb = tb
    N = 1024
    E = _extreme_case(oracle, t, bb)
    steps = R.log2n(N)
    print("t %d base_bit %d: largest |key double| 2^%.1f" % (t, bb, _log2(np.abs(E["dft"]).max())))
    tks = eng.load_trlwe_ks_keys(E["rows"], bb)
    try:
        got = _run_trace(eng, tks, E["cts"])
        _same(got, R.trace_pack_batch(oracle, E["cts"], E["dft"][:steps], t, bb, N), "trace, t %d" % t)
        gen = R.trace_gens(N)[-1]
        for c in range(len(E["cts"])):
            acc = R.embed(E["cts"][c], N)
            for j, g in enumerate(R.trace_gens(N)[:-1]):
                acc = R.trace_step(oracle, acc, g, E["dft"][j], t, bb)
            with np.errstate(over="ignore"):
                exact = np.stack([acc[0], acc[1] + oracle.poly_permute(np.ascontiguousarray(acc[1]), gen)])
            assert (got[c] == exact).all(), "sample %d: the step on the zero entry is not (a, b + b(X^%d))" % (c, gen)
        d_in = ma.to_device(E["trlwe"], eng.device)
        for e0 in (steps, steps - 1):
            want = np.stack([R.rlwe_priv_keyswitch(oracle, c, E["dft"][e0:e0 + 2], t, bb) for c in E["trlwe"]])
            _same(ma.to_numpy(eng.trlwe_rlwe_priv_keyswitch(tks, d_in, e0)), want, "private switch, t %d, entry0 %d" % (t, e0))
        d_g = ma.to_device(E["gadget"], eng.device)
        sel = eng.trgsw_from_gadget(tks, d_g, steps)
        switched = eng.trlwe_rlwe_priv_keyswitch(tks, d_g.view(6, 2, N), steps).view(3, 2, 2, N)
        want = eng.torus_to_dft(torch.cat([switched, d_g], dim=1).contiguous().view(-1, N)).view(3, 4, 2, N)
        torch.cuda.synchronize(eng.device)
        assert torch.equal(sel, want), "%d doubles differ" % int((sel != want).sum())
    finally:
        tks.free()


def _gadget_against_the_two_calls(eng, oracle, D, tks, gadget, N, l, t, bb, what):
    """trgsw_from_gadget == torus_to_dft of (the private switch's words, the gadget rows) as doubles; the private switch's words == the helper"""
    import torch
    import mosfhet_amd as ma
    import trace_reference as R
    count, e0 = len(gadget), R.log2n(N)
    d_g = ma.to_device(gadget, eng.device)
    sel = eng.trgsw_from_gadget(tks, d_g, e0)
    assert sel.shape == (count, 2 * l, 2, N) and sel.dtype == torch.float64
    switched = eng.trlwe_rlwe_priv_keyswitch(tks, d_g.view(count * l, 2, N), e0).view(count, l, 2, N)
    _same(ma.to_numpy(switched), np.stack([R.trgsw_from_gadget(oracle, g, D["dft"][e0:], t, bb)[:l] for g in gadget]), what + ": the private switch of the gadget rows")
    want = eng.torus_to_dft(torch.cat([switched, d_g], dim=1).contiguous().view(-1, N)).view(count, 2 * l, 2, N)
    torch.cuda.synchronize(eng.device)
    assert torch.equal(sel, want), "%s: %d doubles differ" % (what, int((sel != want).sum()))
    return sel


@pytest.mark.gpu
def test_private_switch_and_gadget_at_4096(eng, oracle):
    """N = 4096 (t 2, base_bit 8, count 1; 256 threads a team), where the kernel is instantiated and only the trace ran: the private switch equals the helper on
    every word, and trgsw_from_gadget at l = 2 equals the doubles of torus_to_dft of (private-switch words, gadget rows).  Words and doubles only."""
    import mosfhet_amd as ma
    import trace_reference as R
    N, t, bb = 4096, 2, 8
    D = _case(oracle, N, t, bb, 1, 2.0 ** -50)
    tks, e0 = _tks(eng, D, bb), R.log2n(N)
    ins = _priv_inputs(oracle, D, N, 1, 2.0 ** -50, seed=0x4096A)
    want = np.stack([R.rlwe_priv_keyswitch(oracle, c, D["dft"][e0:], t, bb) for c in ins])
    _same(ma.to_numpy(eng.trlwe_rlwe_priv_keyswitch(tks, ma.to_device(ins, eng.device), e0)), want, "N 4096")
    G = _gadget_case(oracle, D, N, 2, 8, 1, 2.0 ** -50, seed=0x4096B)
    _gadget_against_the_two_calls(eng, oracle, D, tks, G["gadget"], N, 2, t, bb, "N 4096, l 2")


@pytest.mark.gpu
@pytest.mark.parametrize("l", [1, 6])
def test_trgsw_from_gadget_shortest_and_longest(eng, oracle, l):
    """l = 1 and l = 6, the ends of the 1 .. 6 the call accepts (it ran at 2 and 4): N = 1024, count 2, key t 4, base_bit 9, gadget Bg_bit 8.  Words and doubles only."""
    N, t, bb = 1024, 4, 9
    D = _case(oracle, N, t, bb, 67, 2.0 ** -45)
    G = _gadget_case(oracle, D, N, l, 8, 2, 2.0 ** -45, seed=0x6AD0 + l)
    _gadget_against_the_two_calls(eng, oracle, D, _tks(eng, D, bb), G["gadget"], N, l, t, bb, "l %d" % l)


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["trace", "private switch", "gadget"])
def test_trace_calls_are_captured_in_a_graph(eng, oracle, call):
    """Each of the three calls (N = 1024, t 4, base_bit 9), captured on one side stream after an eager call of that shape, replayed twice on different inputs copied
    into the captured buffer: each replay == the eager words resp. doubles, which equal the helper -- no hidden allocation, synchronisation or state left between
    replays.  For the gadget call the eager doubles are held to torus_to_dft of (private-switch words, gadget rows), the words to the helper
    (_gadget_against_the_two_calls).  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    import trace_reference as R
    N, t, bb = 1024, 4, 9
    D = _case(oracle, N, t, bb, 67, 2.0 ** -45)
    tks, e0 = _tks(eng, D, bb), R.log2n(N)
    if call == "trace":
        ins = [D["cts"][:3], D["cts"][3:6]]
        run = lambda x, out=None: eng.tlwe_trace_pack(tks, x, 0, out=out)
        want = [_want_trace(oracle, D, t, bb, N)[:3], _want_trace(oracle, D, t, bb, N)[3:6]]
    elif call == "private switch":
        both = _priv_inputs(oracle, D, N, 4, 2.0 ** -45, seed=0x6AA1)
        ins = [both[:2], both[2:4]]
        run = lambda x, out=None: eng.trlwe_rlwe_priv_keyswitch(tks, x, e0, out=out)
        want = [np.stack([R.rlwe_priv_keyswitch(oracle, c, D["dft"][e0:], t, bb) for c in x]) for x in ins]
    else:
        g = _gadget_case(oracle, D, N, 2, 8, 3, 2.0 ** -45, seed=0x6AA2)["gadget"]
        ins = [g[:1], g[1:2]]
        run = lambda x, out=None: eng.trgsw_from_gadget(tks, x, e0, out=out)
        want = None
    xs = [ma.to_device(np.ascontiguousarray(x), eng.device) for x in ins]
    eager = [run(x).clone() for x in xs]
    torch.cuda.synchronize()
    if want is not None:
        for r in range(2):
            _same(ma.to_numpy(eager[r]), want[r], "%s, eager, inputs %d" % (call, r))
    else:                           # the eager doubles == torus_to_dft of (private-switch words == the helper, gadget rows)
        for r in range(2):
            assert torch.equal(eager[r], _gadget_against_the_two_calls(eng, oracle, D, tks, ins[r], N, 2, t, bb, "gadget, eager, inputs %d" % r))
        assert not torch.equal(eager[0], eager[1])
    d_in, d_out = xs[0].clone(), torch.empty_like(eager[0])
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run(d_in, out=d_out)
    for r in (1, 0):
        d_in.copy_(xs[r])
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d_out, eager[r]), "%s: replay on inputs %d differs from the plain call" % (call, r)
    del g


@pytest.mark.gpu
def test_two_host_threads_run_the_trace(eng, oracle):
    """Two host threads, each on a stream of its own, run the trace five times concurrently -- one at N = 1024 (3 samples), one at N = 2048 (2 samples): every result
    equals the helper's words."""
    import threading
    import torch
    import mosfhet_amd as ma
    jobs = []
    for N, t, bb, count, sigma in ((1024, 4, 9, 67, 2.0 ** -45), (2048, 4, 9, 2, 2.0 ** -50)):
        D = _case(oracle, N, t, bb, count, sigma)
        n = min(count, 3)
        jobs.append((_tks(eng, D, bb), ma.to_device(D["cts"][:n], eng.device), _want_trace(oracle, D, t, bb, N)[:n]))
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            tks, d_in, want = jobs[k]
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    bad[k] += int(not (ma.to_numpy(eng.tlwe_trace_pack(tks, d_in, 0)) == want).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad
