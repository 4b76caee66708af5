"""Packed TRLWE samples opened at an offset and a stride on the device (include/mosfhet_hip.h: mosfhet_hip_trlwe_unpack_strided_batch,
mosfhet_hip_trlwe_unpack_strided_keyswitch_batch, mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch, mosfhet_hip_trlwe_unpack_strided_plan,
mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch; mosfhet_amd/csrc/capi_unpack.inc, capi_polylinear.inc, unpack_kernels.h;
include/mosfhet_compat.h: mosfhet_trlwe_unpack_strided, mosfhet_trlwe_unpack_strided_keyswitch).

A geometry (per, first, stride) on a ring N: sample o per + j of a call is trlwe_extract_tlwe(in[o], first + j stride).  Expected words come from
tests/unpacking_strided_reference.py -- rows first + stride * arange(.) of unpacking_reference.unpack --, held here to the project's oracle and to the reference's
own function; the key switch of its rows goes through oracle.tlwe_keyswitch.  Everything is integer work: every comparison of device words is == on all words.
The forms, keys and inputs of tests/test_trlwe_unpack.py (FUSED, BOOT and its helpers) are reused.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_trlwe_unpack import BOOT, FUSED, HALF_SLOT_16, MARGIN_BITS, SENTINEL, _boot_case, _device_key, _log2, _packed, _switch_key, _switched  # noqa: E402

EINVAL = -1
_CACHE = {}
U64 = np.uint64

# (N, per, first, stride, total) of the bit-exact test
SHAPES = [(256, 16, 0, 16, 16), (256, 5, 3, 50, 17), (256, 1, 255, 1, 3), (256, 1, 0, 256, 2), (1024, 16, 63, 64, 17), (2048, 2048, 0, 1, 2049), (4096, 3, 1, 2047, 4)]
# (per, first, stride) of the fused key switch at N = 256: each ends at coefficient 255
GEOMETRIES = [(4, 66, 63), (67, 57, 3), (128, 1, 2)]
# the bootstrap composition: the 70 values of BOOT at coefficients 24 + 25 j of two inputs (per 40), other values between them
BOOT_FIRST, BOOT_STRIDE = 24, 25
# the round trip with the trace: N = 1024, 16 samples, log_per 4 -> per 16, first 0, stride 64; t 4, base_bit 9, noise 2^-45 (tests/test_trace_pack_many.py)
TRACE = dict(N=1024, t=4, base_bit=9, sigma=2.0 ** -45, L=4, total=16)
TRACE_BOUND = 2.0 ** 58           # the reference's bound for the trace (test/tests.c:850), the bound of test_many_decrypts
HALF_SLOT_TRACE = 2.0 ** 59       # messages mu / (16 N): the phases N m_j lie on multiples of 2^60


def _rows(oracle, N, total, per, first, stride, seed=0):
    """the helper's batch for _packed(N, ceil(total / per), seed), cached"""
    import unpacking_strided_reference as S
    key = ("rows", N, total, per, first, stride, seed)
    if key not in _CACHE:
        _CACHE[key] = S.unpack_batch(_packed(oracle, N, -(-total // per), seed), total, per, first, stride)
    return _CACHE[key]


def _boot_strided(oracle):
    """BOOT's keys, table and messages (tests/test_trlwe_unpack.py) with the 70 values at coefficients 24 + 25 j of two inputs; every other coefficient carries a
    value nobody opens.  Made once and left unchanged."""
    if "boot" not in _CACHE:
        B, D = BOOT, _boot_case(oracle)
        N, total, per = B["N"], B["total"], B["per"]
        rng = oracle.Rng(0x57A1DE)
        outputs = -(-total // per)
        packed = np.empty((outputs, 2, N), dtype=U64)
        for o in range(outputs):
            m = (rng.words(N) % U64(16)) << U64(59)
            have = min(per, total - o * per)
            m[BOOT_FIRST + BOOT_STRIDE * np.arange(have)] = D["msgs"][o * per:o * per + have] << U64(59)
            packed[o] = oracle.trlwe_sample(rng, m, D["s_ring"].reshape(1, N), B["sigma"])
        _CACHE["boot"] = packed
    return _CACHE["boot"]


def _trace_case(oracle):
    """the key of tests/test_trace_pack_many.py's decryption test at N = 1024 (the same generator calls in the same order: t 4, base_bit 9, noise 2^-45) and 16
    samples with messages mu_j / (16 N)"""
    import trace_reference as R
    if "trace" not in _CACHE:
        T = TRACE
        N, t, bb = T["N"], T["t"], T["base_bit"]
        rng = oracle.Rng(0x3A27 + 131 * N + 17 * t + bb)
        s = oracle.gen_binary_key(rng, N)
        rows = np.concatenate([R.gen_trace_keys(oracle, rng, s, t, bb, T["sigma"]), R.gen_gadget_keys(oracle, rng, s, t, bb, T["sigma"])])
        msgs = ((np.arange(T["total"], dtype=U64) * U64(7) + U64(3)) % U64(16)) << U64(60 - R.log2n(N))
        cts = np.stack([oracle.tlwe_sample(rng, m, s, T["sigma"]) for m in msgs])
        _CACHE["trace"] = dict(s=s, rows=rows, msgs=msgs, cts=cts)
    return _CACHE["trace"]


def _trace_worst(oracle, opened, D):
    """the largest distance of the opened samples' phases from N m_j"""
    N = TRACE["N"]
    with np.errstate(over="ignore"):
        want = D["msgs"] * U64(N)
    return max(float(oracle.torus_dist(U64(oracle.tlwe_phase(np.ascontiguousarray(opened[j]), D["s"])), want[j])) for j in range(len(opened)))


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_strided_helper_against_the_oracle(oracle):
    """unpacking_strided_reference.unpack_batch == oracle.trlwe_extract_tlwe(in[o], first + j stride) on every sample of a ragged batch: N = 256, per 5, first 3,
    stride 50, total 17 (four inputs, the last opened to 2)."""
    import unpacking_strided_reference as S
    N, per, first, stride, total = 256, 5, 3, 50, 17
    P, got = _packed(oracle, N, 4), _rows(oracle, N, total, per, first, stride)
    assert got.shape == (total, N + 1)
    for c in range(total):
        assert (got[c] == oracle.trlwe_extract_tlwe(P[c // per], first + (c % per) * stride)).all(), c
    assert S.unpack_batch(P, 0, per, first, stride).shape == (0, N + 1)


@pytest.mark.parametrize("backend", ["avx512", "ffnt"])
def test_strided_helper_against_the_reference(oracle, backend):
    """... == the reference's own trlwe_extract_tlwe (both builds of oracle/_ref, through ctypes) on every sample of the same ragged batch."""
    from oracle import reflib
    if not reflib.available(backend):
        pytest.skip("oracle/_ref/libmosfhet_ref_%s.so is absent (or this CPU lacks AVX-512)" % backend)
    ref = reflib.get(backend)
    if not ref.has("ref_trlwe_extract_tlwe"):
        pytest.skip("the reference build does not export trlwe_extract_tlwe")
    N, per, first, stride, total = 256, 5, 3, 50, 17
    P, got = _packed(oracle, N, 4), _rows(oracle, N, total, per, first, stride)
    for c in range(total):
        assert (got[c] == ref.trlwe_extract_tlwe(P[c // per], first + (c % per) * stride)).all(), (backend, c)


def _abi(native_lib):
    f = native_lib.mosfhet_hip_trlwe_unpack_strided_batch
    f.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]
    g = native_lib.mosfhet_hip_trlwe_unpack_strided_keyswitch_batch
    g.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
    h = native_lib.mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch
    h.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    p = native_lib.mosfhet_hip_trlwe_unpack_strided_plan
    p.argtypes = [C.c_int] * 10 + [C.c_void_p]
    q = native_lib.mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch
    q.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    return f, g, h, p, q


# (per, first, stride, what the message names) refused on a ring of N = 256
REFUSED_256 = [(1, -1, 1, "first = -1"), (1, 256, 1, "first = 256"), (2, 0, 0, "stride = 0"), (2, 0, -5, "stride = -5"), (2, 0, 256, "stride = 256"),
               (3, 2, 127, "stride = 127"), (2, 0, 2 ** 31 - 1, "stride = 2147483647"), (2 ** 31 - 1, 0, 2 ** 31 - 1, "per = 2147483647"), (257, 0, 1, "per = 257"),
               (0, 0, 1, "per = 0")]


def test_strided_symbols_and_argument_checks(native_lib):
    """The library exports the five entry points and the host face, the binding its functions.  Every refusal that needs no device returns MOSFHET_HIP_EINVAL with a
    message naming the argument -- on fake pointers, before any handle is read and before any HIP call: first = -1 and first = N; stride = 0; a last coefficient of N
    (N - 1 is accepted); stride = 2^31 - 1 with per = 2, evaluated in 64 bits, not wrapped; per > N.  total == 0 is OK, after the scalar checks."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_trlwe_unpack_strided_batch", "mosfhet_hip_trlwe_unpack_strided_keyswitch_batch",
                 "mosfhet_hip_unpack_strided_keyswitch_functional_bootstrap_batch", "mosfhet_hip_trlwe_unpack_strided_plan",
                 "mosfhet_hip_trlwe_linear_unpack_keyswitch_functional_bootstrap_batch", "mosfhet_trlwe_unpack_strided", "mosfhet_trlwe_unpack_strided_keyswitch"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine, "trlwe_unpack_strided_plan")
    for name in ("trlwe_unpack_strided", "trlwe_unpack_strided_keyswitch", "unpack_strided_keyswitch_functional_bootstrap", "trlwe_linear_unpack_keyswitch_functional_bootstrap"):
        assert hasattr(engine.Engine, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f, g, h, p, q = _abi(native_lib)
    assert f(None, fake, fake, 256, 1, 1, 0, 1, None) == EINVAL and "ctx" in err()
    for per, first, stride, what in REFUSED_256:
        assert f(fake, fake, fake, 256, 1, per, first, stride, None) == EINVAL and what in err(), (per, first, stride, err())
        assert f(fake, fake, fake, 256, 0, per, first, stride, None) == EINVAL and what in err(), (per, first, stride, err())      # total == 0 comes after the ranges
    assert f(fake, fake, fake, 256, 1, 2, 0, 256, None) == EINVAL and "= 256 is past N - 1 = 255" in err(), err()      # a last coefficient of N
    assert f(fake, fake, fake, 256, 1, 2, 0, 2 ** 31 - 1, None) == EINVAL and "= 2147483647 is past N - 1" in err(), err()      # 64 bits: not wrapped
    assert f(fake, fake, fake, 4096, 1, 3, 2 ** 31 - 1, 2 ** 31 - 1, None) == EINVAL and "first = 2147483647" in err(), err()
    for N in (128, 8192, 1000, 0, -256):
        assert f(fake, fake, fake, N, 1, 1, 0, 1, None) == EINVAL and "N = %d" % N in err(), N
    assert f(fake, fake, fake, 256, -1, 1, 0, 1, None) == EINVAL and "total = -1" in err()
    assert f(fake, None, fake, 256, 1, 1, 0, 1, None) == EINVAL and "null buffer" in err()
    # accepted geometries: the last coefficient N - 1 in every way, stride = N with per = 1 (total == 0: nothing is read)
    for N, per, first, stride in ((256, 2, 0, 255), (256, 3, 1, 127), (256, 1, 255, 1), (256, 1, 0, 256), (256, 1, 0, 2 ** 31 - 1), (256, 256, 0, 1), (4096, 3, 1, 2047),
                                  (1024, 16, 63, 64)):
        assert f(fake, None, None, N, 0, per, first, stride, None) == 0, (N, per, first, stride, err())
    # the calls that take the ring from the key hold the scalars to the largest ring before the key is read (and to the key's ring after it: on the device)
    assert g(None, fake, fake, fake, 1, 1, 0, 1, None) == EINVAL and "ctx" in err()
    assert g(fake, None, fake, fake, 1, 1, 0, 1, None) == EINVAL and "ksk" in err()
    assert h(None, fake, fake, fake, fake, 1, fake, 1, 1, 0, 1, 4, 1, None) == EINVAL and "ctx" in err()
    assert h(fake, None, fake, fake, fake, 1, fake, 1, 1, 0, 1, 4, 1, None) == EINVAL and "null key" in err()
    assert h(fake, fake, None, fake, fake, 1, fake, 1, 1, 0, 1, 4, 1, None) == EINVAL and "null key" in err()
    assert q(None, fake, fake, fake, fake, fake, 1, fake, 1, 0, 1, 1, 4, 1, None) == EINVAL and "ctx" in err()
    assert q(fake, None, fake, fake, fake, fake, 1, fake, 1, 0, 1, 1, 4, 1, None) == EINVAL and "lin" in err()
    assert q(fake, fake, None, fake, fake, fake, 1, fake, 1, 0, 1, 1, 4, 1, None) == EINVAL and "ksk" in err()
    assert q(fake, fake, fake, None, fake, fake, 1, fake, 1, 0, 1, 1, 4, 1, None) == EINVAL and "bsk" in err()
    for per, first, stride, what in ((1, -1, 1, "first = -1"), (1, 4096, 1, "first = 4096"), (2, 0, 0, "stride = 0"), (2, 0, 4096, "stride = 4096"),
                                     (2, 0, 2 ** 31 - 1, "stride = 2147483647"), (4097, 0, 1, "per = 4097"), (0, 0, 1, "per = 0")):
        assert g(fake, fake, fake, fake, 1, per, first, stride, None) == EINVAL and what in err(), (per, first, stride, err())
        assert g(fake, fake, fake, fake, 0, per, first, stride, None) == EINVAL and what in err(), (per, first, stride, err())
        assert h(fake, fake, fake, fake, fake, 1, fake, 1, per, first, stride, 4, 1, None) == EINVAL and what in err(), (per, first, stride, err())
        assert q(fake, fake, fake, fake, fake, fake, 1, fake, per, first, stride, 1, 4, 1, None) == EINVAL and what in err(), (per, first, stride, err())
    assert g(fake, fake, fake, fake, -1, 1, 0, 1, None) == EINVAL and "total = -1" in err()
    assert h(fake, fake, fake, fake, fake, 1, fake, -2, 1, 0, 1, 4, 1, None) == EINVAL and "total = -2" in err()
    assert q(fake, fake, fake, fake, fake, fake, 1, fake, 1, 0, 1, -1, 4, 1, None) == EINVAL and "count = -1" in err()
    assert g(fake, fake, fake, fake, 0, 3, 1, 2047, None) == 0
    assert q(fake, fake, fake, fake, fake, fake, 1, fake, 4, 0, 256, 0, 4, 1, None) == 0
    # the calls without a geometry keep their checks: per <= N is the range check of (first 0, stride 1)
    u = native_lib.mosfhet_hip_trlwe_unpack_batch
    u.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert u(fake, fake, fake, 256, 1, 257, None) == EINVAL and "per = 257" in err()
    assert u(fake, None, None, 256, 0, 256, None) == 0


def test_strided_plan_equals_the_plain_plan(native_lib):
    """mosfhet_hip_trlwe_unpack_strided_plan == mosfhet_hip_trlwe_unpack_plan at the same (total, per) on a grid of shapes, at three settings of set_ks_words and
    for several accepted geometries per shape: no field depends on first or stride.  It makes the refusals of the calls, with the same words."""
    from mosfhet_amd import engine
    P, S = engine.trlwe_unpack_plan, engine.trlwe_unpack_strided_plan
    checked = 0
    try:
        for setting in (-1, 0, 100):
            engine.set_ks_words(setting)
            for N, n_out in ((256, 16), (1024, 585), (2048, 632)):
                for t, bb in ((2, 2), (3, 4), (1, 8)):
                    for compressed in (False, True):
                        for total in (1, 16, 17, 70, 257, 300, 8192, 8193, 3 * 8192):
                            for per, first, stride in ((min(N, 67), 0, 1), (16, 0, N // 16), (5, 3, 50), (3, 1, (N - 2) // 2), (1, N - 1, 1), (1, 0, N)):
                                plain = P(N, n_out, t, bb, total, per, compressed)
                                assert S(N, n_out, t, bb, total, per, first, stride, compressed) == plain, (setting, N, n_out, t, bb, compressed, total, per, first, stride)
                                checked += 1
                    assert S(N, 0, 0, 0, 2049, 16, 7, (N - 8) // 15) == P(N, total=2049, per=16)        # n_out = 0: the unpack call alone
    finally:
        engine.set_ks_words(-1)
    assert checked > 2000
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    p = _abi(native_lib)[3]
    plan = (C.c_longlong * 8)()
    assert p(256, 16, 2, 2, 0, 10, 5, 0, 1, 256, None) == EINVAL and "plan" in err()
    for per, first, stride, what in REFUSED_256:
        assert p(256, 16, 2, 2, 0, 10, per, first, stride, 256, plan) == EINVAL and what in err(), (per, first, stride, err())
    for N in (128, 8192, 1000):
        assert p(N, 0, 0, 0, 0, 10, 5, 0, 1, 256, plan) == EINVAL and "N = %d" % N in err()
    assert p(1024, 16, 2, 9, 0, 10, 5, 0, 1, 256, plan) == EINVAL and "base_bit = 9" in err()
    assert p(1024, 16, 2, 2, 0, 10, 5, 3, 50, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(256, 16, 2, 2, 0, 10, 2, 0, 255, 256, plan) == 0 and plan[0] == 5
    with pytest.raises(engine.MosfhetHipError, match="stride = 2147483647"):
        S(256, total=2, per=2, first=0, stride=2 ** 31 - 1)
    with pytest.raises(engine.MosfhetHipError, match="fit a C int"):
        S(256, total=2, per=2, first=0, stride=2 ** 32 + 1)


def test_strided_kernels_of_the_build(native_lib):
    """The geometry enters as run-time arguments: tools/kernel_table.py lists trlwe_unpack_kernel and the packed entries kernel once each, at most 256 VGPRs, without
    scratch; the library holds exactly 329 kernels; tools/check_lds_barriers.py finds nothing on a build of its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    import check_lds_barriers
    rows = kernel_table.table()
    for name in ("trlwe_unpack_kernel", "ks_words_entries_packed_kernel"):
        mine = [r for r in rows if r["name"].startswith(name)]
        for r in mine:
            print("%-60s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
        assert len(mine) == 1, (name, mine)
        assert mine[0]["vgpr"] <= 256 and mine[0]["scratch"] == 0, mine
    print("%d kernels" % len(rows))
    assert len(rows) == 329, len(rows)
    assert check_lds_barriers.build_and_check() == []


def _compile_c(tmp_path):
    exe = str(tmp_path / "trlwe_unpack_strided")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_unpack_strided.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_strided_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trlwe_unpack_strided.c compiles with -Wall -Werror against include/mosfhet.h and links against the built library (its device part:
    test_strided_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


def test_the_strided_composition_decrypts_on_the_cpu(oracle):
    """The condition of test_strided_bootstrap_decrypts, from the references alone: the helper at coefficients 24 + 25 j, then oracle.tlwe_keyswitch, then
    oracle.functional_bootstrap on the 70 values of BOOT (N = 1024, n = 24, l = 2, Bg_bit = 8, switch t = 4, base_bit = 4, all noises 2^-40, 16 slots; table entries on
    multiples of 1/16, inputs in slots of 1/32 as in tests/test_trlwe_unpack.py) decrypts every value to its table entry; the phases lie within half a slot (2^59)
    with a margin of at least 2 bits.  Measured: 2^54.2 (printed again by every run)."""
    import unpacking_strided_reference as S
    B, D = BOOT, _boot_case(oracle)
    rows = S.unpack_batch(_boot_strided(oracle), B["total"], B["per"], BOOT_FIRST, BOOT_STRIDE)
    worst_in = max(oracle.torus_dist(U64(oracle.tlwe_phase(rows[c], D["s_ring"])), D["msgs"][c] << U64(59)) for c in range(B["total"]))
    worst = 0.0
    for c in range(B["total"]):
        sw = oracle.tlwe_keyswitch(rows[c], D["ksk"], B["n"], B["t"], B["base_bit"])
        out = oracle.functional_bootstrap(D["tv"], sw, D["bk_dft"], B["l"], B["Bg_bit"], B["slots"])
        worst = max(worst, float(oracle.torus_dist(U64(oracle.tlwe_phase(out, D["s_ring"])), D["expect"][c])))
    print("the samples at 24 + 25 j: 2^%.1f from their slots; the composition: 2^%.1f from the table entries (half a slot: 2^59)" % (_log2(worst_in), _log2(worst)))
    assert worst < HALF_SLOT_16 / 2 ** MARGIN_BITS, _log2(worst)


def test_the_trace_round_trip_on_the_cpu(oracle):
    """The condition of test_trace_round_trip, from the references alone: 16 samples with messages mu_j / (16 N) through trace_many_reference.pack_many (N = 1024,
    log_per 4, t 4, base_bit 9, noise 2^-45: the key of tests/test_trace_pack_many.py), then the helper with per 16, first 0, stride 64: sample j has phase N m_j, a
    multiple of 2^60, within half a slot (2^59) with a margin of at least 2 bits -- inside the reference's bound for the trace, 2^58.  Measured: 2^42.8 (printed
    again by every run)."""
    import trace_many_reference as RM
    import unpacking_strided_reference as S
    T, D = TRACE, _trace_case(oracle)
    N = T["N"]
    packed = RM.pack_many(oracle, D["cts"], T["L"], oracle.ks_to_dft(D["rows"])[:10], T["t"], T["base_bit"], N)
    assert packed.shape == (1, 2, N)
    opened = S.unpack_batch(packed, T["total"], 1 << T["L"], 0, N >> T["L"])
    worst = _trace_worst(oracle, opened, D)
    print("trace-packed and opened at stride 64: 2^%.1f from N m_j (half a slot: 2^59)" % _log2(worst))
    assert worst < HALF_SLOT_TRACE / 2 ** MARGIN_BITS and worst <= TRACE_BOUND, _log2(worst)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _unpack_into_sentinel(eng, packed, total, per, first, stride):
    """the call into a buffer one row longer than total, pre-filled with a sentinel: (the batch, the row past it)"""
    import torch
    import mosfhet_amd as ma
    N = packed.shape[2]
    buf = torch.full((total + 1, N + 1), int(SENTINEL.view(np.int64)), dtype=torch.int64, device=eng.device)
    eng.trlwe_unpack_strided(ma.to_device(packed, eng.device), total, per, first, stride, out=buf[:total])
    got = ma.to_numpy(buf)
    return got[:total], got[total]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d-%d-%d" % s for s in SHAPES])
def test_strided_bit_exact(eng, oracle, shape):
    """== the helper on every word: the 16 slots of a trace-packed sample at the smallest ring; a ragged batch of four inputs; a sample at the last coefficient (no
    negated word); stride = N with per = 1; 17 samples at first 63, stride 64 of N = 1024; (0, 1) at N = 2048, which also == the call without a geometry on the
    device; the last coefficient N - 1 at N = 4096.  The row past `total` keeps its sentinel."""
    import mosfhet_amd as ma
    N, per, first, stride, total = shape
    packed = _packed(oracle, N, -(-total // per))
    got, past = _unpack_into_sentinel(eng, packed, total, per, first, stride)
    want = _rows(oracle, N, total, per, first, stride)
    assert got.shape == want.shape and (got == want).all(), "%s: %d words differ, rows %s" % (shape, (got != want).sum(), sorted(set(np.nonzero(got != want)[0]))[:8])
    assert (past == SENTINEL).all(), "%s: the row past total was written" % (shape,)
    if (first, stride) == (0, 1):
        assert (ma.to_numpy(eng.trlwe_unpack(ma.to_device(packed, eng.device), total, per)) == got).all()
    if (N, per, first) == (256, 1, 255):
        assert (got[:, :N] == packed[:3, 0, ::-1]).all()          # a[255 - i]: nothing wraps, nothing is negated


@pytest.mark.gpu
def test_strided_extreme_masks(eng, oracle):
    """Inputs whose mask words are all 0, all 2^63 and all 2^64 - 1, and a random one (N = 256, per 4, first 66, stride 63): == the helper; the negated wrap of 0 and of
    2^63 is itself, so those samples hold one value throughout."""
    import unpacking_strided_reference as S
    N, per, first, stride = 256, 4, 66, 63
    P = _packed(oracle, N, 4, seed=1).copy()
    P[0, 0], P[1, 0], P[2, 0] = 0, U64(1) << U64(63), U64(0xFFFFFFFFFFFFFFFF)
    got, past = _unpack_into_sentinel(eng, P, 4 * per, per, first, stride)
    assert (got == S.unpack_batch(P, 4 * per, per, first, stride)).all() and (past == SENTINEL).all()
    assert (got[:per, :N] == 0).all() and (got[per:2 * per, :N] == U64(1) << U64(63)).all()
    ones = got[2 * per:3 * per, :N]
    assert set(np.unique(ones)) == {U64(1), U64(0xFFFFFFFFFFFFFFFF)} and (ones[0, :first + 1] == U64(0xFFFFFFFFFFFFFFFF)).all() and (ones[0, first + 1:] == 1).all()


FUSED_CASES = [(c, g) for c in FUSED for g in GEOMETRIES]
FUSED_IDS = ["%s-per%d" % (n, g[0]) for n in ("small", "words-70", "words-300", "words-two-pieces", "tiles256", "tiles512") for g in GEOMETRIES]


@pytest.mark.gpu
@pytest.mark.parametrize("case,geometry", FUSED_CASES, ids=FUSED_IDS)
def test_strided_keyswitch_equals_unpack_then_keyswitch(eng, oracle, case, geometry):
    """N = 256, n_out = 16: trlwe_unpack_strided_keyswitch == trlwe_unpack_strided followed by tlwe_keyswitch on the device (all rows), and == oracle.tlwe_keyswitch of
    the helper's rows (all rows; for the batch of 8192 + 70 the first 80 and the rows from 8100 on, around the piece boundary, which lies inside an input at per 67),
    in every form of tests/test_trlwe_unpack.py's FUSED list -- each asserted through the strided plan -- and at three geometries that end at coefficient 255."""
    import mosfhet_amd as ma
    import unpacking_strided_reference as S
    from mosfhet_amd import engine
    form, setting, t, bb, total, _ = case
    per, first, stride = geometry
    N, n_out = 256, 16
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    packed = _packed(oracle, N, -(-total // per), seed=2)
    d_in = ma.to_device(packed, eng.device)
    try:
        engine.set_ks_words(setting)
        plan = engine.trlwe_unpack_strided_plan(N, n_out, t, bb, total, per, first, stride)
        assert plan["form"] == form and plan["pieces"] == -(-total // 8192), plan
        fused = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride))
        unpacked = eng.trlwe_unpack_strided(d_in, total, per, first, stride)
        two_calls = ma.to_numpy(eng.tlwe_keyswitch(dksk, unpacked))
    finally:
        engine.set_ks_words(-1)
    assert fused.shape == (total, n_out + 1)
    bad = np.nonzero((fused != two_calls).any(axis=1))[0]
    assert bad.size == 0, "%s %s: %d samples differ from unpack + tlwe_keyswitch, first %s" % (form, geometry, bad.size, bad[:8])
    check = list(range(total)) if total < 1000 else list(range(80)) + list(range(8100, total))
    opened = {o: S.unpack(packed[o], min(per, total - o * per), first, stride) for o in sorted({c // per for c in check})}
    rows = np.stack([opened[c // per][c % per] for c in check])
    assert (ma.to_numpy(unpacked)[check] == rows).all()
    assert (fused[check] == _switched(oracle, K, rows, n_out, t, bb)).all(), "%s %s: differs from the oracle's key switch of the helper's rows" % (form, geometry)


@pytest.mark.gpu
def test_strided_keyswitch_with_a_seed_compressed_key(eng, oracle):
    """A seed-compressed key and its stored twin (the same seed, the same noise secret): the strided fused call gives the same words with both, at 200 samples (tiles of
    256) and at 9 (the direct kernels), and they equal trlwe_unpack_strided followed by tlwe_keyswitch (N = 256, per 67, first 57, stride 3)."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, n_out, t, bb, per, first, stride = 256, 16, 2, 2, 67, 57, 3
    K = _switch_key(oracle, N, n_out, t, bb)
    eng.set_keygen_secret(b"the twins share one noise stream")
    stored = eng.generate_keyswitch_key(K["s_out"], K["s_in"], t, bb, 2.0 ** -40, 0xC0FFEE)
    eng.set_keygen_secret(b"the twins share one noise stream")
    packed_key = eng.generate_keyswitch_key(K["s_out"], K["s_in"], t, bb, 2.0 ** -40, 0xC0FFEE, compressed=True)
    try:
        for total, form in ((200, "tiles_256"), (9, "small")):
            assert engine.trlwe_unpack_strided_plan(N, n_out, t, bb, total, per, first, stride, compressed=True)["form"] == form
            d_in = ma.to_device(_packed(oracle, N, -(-total // per), seed=2), eng.device)
            a = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(packed_key, d_in, total, per, first, stride))
            b = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(stored, d_in, total, per, first, stride))
            rows = eng.trlwe_unpack_strided(d_in, total, per, first, stride)
            assert (ma.to_numpy(rows) == _rows(oracle, N, total, per, first, stride, seed=2)).all()
            c = ma.to_numpy(eng.tlwe_keyswitch(stored, rows))
            assert (a == b).all() and (b == c).all(), total
    finally:
        stored.free()
        packed_key.free()


def _boot_keys(eng, oracle):
    D = _boot_case(oracle)
    if "bsk" not in D or D["bsk"].engine is not eng:
        D["bsk"] = eng.load_bootstrap_key(D["bk"], 1, BOOT["l"], BOOT["Bg_bit"])
        D["dksk"] = eng.load_keyswitch_key(D["ksk"], BOOT["base_bit"])
    return D


@pytest.mark.gpu
def test_strided_bootstrap_equals_the_two_calls(eng, oracle):
    """unpack_strided_keyswitch_functional_bootstrap == trlwe_unpack_strided_keyswitch followed by functional_bootstrap[_wo_extract] (BOOT: N = 1024, n = 24, 70 values
    at coefficients 24 + 25 j, 40 per input), with extract 1 and 0 and with one test vector and one per value."""
    import mosfhet_amd as ma
    B, D = BOOT, _boot_keys(eng, oracle)
    N, total, per = B["N"], B["total"], B["per"]
    d_in = ma.to_device(_boot_strided(oracle), eng.device)
    tvs = np.stack([oracle.trlwe_torus_packing(np.roll(D["lut"], c), 1, N) for c in range(total)])
    switched = eng.trlwe_unpack_strided_keyswitch(D["dksk"], d_in, total, per, BOOT_FIRST, BOOT_STRIDE)
    for d_tv in (ma.to_device(D["tv"][None], eng.device), ma.to_device(tvs, eng.device)):
        for extract in (True, False):
            one = ma.to_numpy(eng.unpack_strided_keyswitch_functional_bootstrap(D["dksk"], D["bsk"], d_tv, d_in, total, per, BOOT_FIRST, BOOT_STRIDE, B["slots"], extract))
            boot = eng.functional_bootstrap if extract else eng.functional_bootstrap_wo_extract
            two = ma.to_numpy(boot(D["bsk"], d_tv, switched, B["slots"]))
            assert one.shape == two.shape and (one == two).all(), (d_tv.shape[0], extract)


@pytest.mark.gpu
def test_strided_bootstrap_decrypts(eng, oracle):
    """The inputs of test_the_strided_composition_decrypts_on_the_cpu through unpack_strided_keyswitch_functional_bootstrap: every one of the 70 values at coefficients
    24 + 25 j decrypts to its table entry within half a slot (2^59)."""
    import mosfhet_amd as ma
    B, D = BOOT, _boot_keys(eng, oracle)
    total, per = B["total"], B["per"]
    out = eng.unpack_strided_keyswitch_functional_bootstrap(D["dksk"], D["bsk"], ma.to_device(D["tv"][None], eng.device), ma.to_device(_boot_strided(oracle), eng.device),
                                                            total, per, BOOT_FIRST, BOOT_STRIDE, B["slots"])
    words = ma.to_numpy(out)
    d = max(float(oracle.torus_dist(U64(oracle.tlwe_phase(words[c], D["s_ring"])), D["expect"][c])) for c in range(total))
    print("the values at 24 + 25 j through the bootstrap: 2^%.1f from the table entries (half a slot: 2^59)" % _log2(d))
    assert d < HALF_SLOT_16, _log2(d)


@pytest.mark.gpu
def test_trace_round_trip(eng, oracle):
    """N = 1024: 16 LWE samples through tlwe_trace_pack_many (log_per 4: sample j at coefficient 64 j), then trlwe_unpack_strided (per 16, first 0, stride 64): == the
    helper applied to the packed sample, and the phase of sample j is N m_j within 2^58, the bound of tests/test_trace_pack_many.py's decryption test, on its keys."""
    import mosfhet_amd as ma
    import unpacking_strided_reference as S
    T, D = TRACE, _trace_case(oracle)
    N, n = T["N"], 1 << T["L"]
    tks = eng.load_trlwe_ks_keys(D["rows"], T["base_bit"])
    try:
        packed = eng.tlwe_trace_pack_many(tks, ma.to_device(D["cts"], eng.device), T["L"])
        assert tuple(packed.shape) == (1, 2, N)
        opened = ma.to_numpy(eng.trlwe_unpack_strided(packed, T["total"], n, 0, N // n))
    finally:
        tks.free()
    assert (opened == S.unpack_batch(ma.to_numpy(packed), T["total"], n, 0, N // n)).all()
    worst = _trace_worst(oracle, opened, D)
    print("trace-packed and opened at stride 64 on the device: 2^%.1f from N m_j" % _log2(worst))
    assert worst <= TRACE_BOUND, _log2(worst)


def _set1(eng, oracle):
    """the SET_1 key fixtures of tests/test_trlwe_linear.py (N = 1024), with device handles of this module's engine"""
    if "set1" not in _CACHE or _CACHE["set1"]["bsk"].engine is not eng:
        from mosfhet_amd import host
        from test_gpu_parity import _keyset
        K = _keyset("set1", eng, oracle)
        P = K["P"]
        if "ksk" not in K:
            K["ksk"] = host.gen_tlwe_ks_key(K["lk"], K["out_key"], P["t"], P["base_bit"])
        _CACHE["set1"] = dict(P=P, dksk=eng.load_keyswitch_key(K["ksk"], P["base_bit"]), bsk=eng.load_bootstrap_key(K["bk"], 1, P["l"], P["Bg_bit"]))
    return _CACHE["set1"]


@pytest.mark.gpu
def test_linear_unpack_bootstrap_equals_the_two_calls(eng, oracle):
    """N = 1024, (rows_out, rows_in, count) = (2, 3, 2), SET_1 keys, per 4, first 0, stride 256: trlwe_linear_unpack_keyswitch_functional_bootstrap == trlwe_linear
    followed by unpack_strided_keyswitch_functional_bootstrap on its 4 results, word for word, with extract 1 and 0 and with one test vector and one per sample; a
    handle of another ring and a geometry past the ring are refused."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine, host
    K = _set1(eng, oracle)
    dksk, bsk = K["dksk"], K["bsk"]
    N, rows_out, rows_in, count, per, first, stride = 1024, 2, 3, 2, 4, 0, 256
    assert K["P"]["N"] == N
    rng = np.random.default_rng(0x57A1D)
    x = rng.integers(0, 2 ** 64, size=(count, rows_in, 2, N), dtype=np.uint64)
    W = rng.integers(-128, 128, size=(rows_out, rows_in, N), dtype=np.int64)
    bias = rng.integers(0, 2 ** 64, size=(rows_out, N), dtype=np.uint64)
    samples = count * rows_out * per
    tvs = np.stack([host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, N) for _ in range(samples)])
    lin = eng.polylinear_create_dense(W, bias)
    d_x = ma.to_device(x, eng.device)
    try:
        d_y = eng.trlwe_linear(lin, d_x).view(count * rows_out, 2, N)
        for tv in (tvs[:1], tvs):
            d_tv = ma.to_device(tv, eng.device)
            for extract in (True, False):
                want = ma.to_numpy(eng.unpack_strided_keyswitch_functional_bootstrap(dksk, bsk, d_tv, d_y, samples, per, first, stride, 4, extract))
                got = ma.to_numpy(eng.trlwe_linear_unpack_keyswitch_functional_bootstrap(lin, dksk, bsk, d_tv, d_x, per, first, stride, 4, extract))
                assert got.shape == want.shape and got.shape[0] == samples and (got == want).all(), (len(tv), extract)
        with pytest.raises(engine.MosfhetHipError, match="stride = 342"):
            eng.trlwe_linear_unpack_keyswitch_functional_bootstrap(lin, dksk, bsk, ma.to_device(tvs[:1], eng.device), d_x, per, first, 342, 4)
    finally:
        lin.close()
    lin2 = eng.polylinear_create_dense(rng.integers(-128, 128, size=(1, 1, 2048), dtype=np.int64))
    try:
        with pytest.raises(engine.MosfhetHipError, match="ring"):
            eng.trlwe_linear_unpack_keyswitch_functional_bootstrap(lin2, dksk, bsk, ma.to_device(tvs[:1], eng.device),
                                                                   ma.to_device(rng.integers(0, 2 ** 64, size=(1, 1, 2, 2048), dtype=np.uint64), eng.device), per, first, stride, 4)
    finally:
        lin2.close()


@pytest.mark.gpu
def test_strided_stale_pool_and_total_0(eng, oracle):
    """The direct form unpacks into the calling thread's pool: a call of 9 samples (per 4, first 66, stride 63) that follows a call of 16 samples at another geometry,
    whose rows still lie in the pool, == the oracle's key switch of the helper's rows; so does a word-lane call that follows a larger one.  total = 0 returns OK and
    writes nothing, in all three calls."""
    import torch
    import mosfhet_amd as ma
    import unpacking_strided_reference as S
    N, n_out, t, bb = 256, 16, 2, 2
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    packed = _packed(oracle, N, 5, seed=2)
    d_in = ma.to_device(packed, eng.device)
    eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 16, 16, 0, 16)
    got = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 9, 4, 66, 63))
    assert (got == _switched(oracle, K, S.unpack_batch(packed, 9, 4, 66, 63), n_out, t, bb)).all()
    eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 300, 67, 57, 3)
    got = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 70, 16, 15, 16))
    assert (got == _switched(oracle, K, S.unpack_batch(packed, 70, 16, 15, 16), n_out, t, bb)).all()
    out = torch.full((4, N + 1), 5, dtype=torch.int64, device=eng.device)
    assert eng.trlwe_unpack_strided(d_in, 0, 4, 66, 63, out=out[:0]).shape[0] == 0
    assert eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 0, 4, 66, 63, out=out.view(-1)[:0].view(0, n_out + 1)).shape[0] == 0
    torch.cuda.synchronize(eng.device)
    assert (out == 5).all()


@pytest.mark.gpu
def test_strided_keyswitch_is_captured_in_a_graph(eng, oracle):
    """trlwe_unpack_strided (from its first call) and trlwe_unpack_strided_keyswitch at 70 samples (after one eager call of that size), captured on one side stream and
    replayed twice on different inputs: each replay == the eager words.  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    N, n_out, t, bb, total, per, first, stride = 256, 16, 2, 2, 70, 67, 57, 3
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    xs = [ma.to_device(_packed(oracle, N, 2, seed=s), eng.device) for s in (2, 3)]
    want_rows = [_rows(oracle, N, total, per, first, stride, seed=s) for s in (2, 3)]
    eager = [ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, x, total, per, first, stride)) for x in xs]
    assert (eager[0] == _switched(oracle, K, want_rows[0], n_out, t, bb)).all()
    side = torch.cuda.Stream(device=eng.device)
    d_in, d_rows, d_out = xs[0].clone(), eng.empty(total, N + 1), eng.empty(total, n_out + 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.trlwe_unpack_strided(d_in, total, per, first, stride, out=d_rows)
        eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride, out=d_out)
    for r in (1, 0):
        d_in.copy_(xs[r])
        d_rows.zero_()
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_rows) == want_rows[r]).all(), "replay on inputs %d: the unpacked rows differ from the helper" % r
        assert (ma.to_numpy(d_out) == eager[r]).all(), "replay on inputs %d differs from the plain call" % r
    del g


@pytest.mark.gpu
def test_strided_refusals_on_the_device(eng, oracle):
    """On real handles: a geometry past the key's ring (accepted on a larger ring, so only the key can refuse it), d_out overlapping d_in, a packing key, a key of
    another ring (the binding's check and the library's) and a key of another context are refused with MOSFHET_HIP_EINVAL, each leaving d_out untouched."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, n_out, t, bb, total, per, first, stride = 256, 16, 2, 2, 70, 67, 57, 3
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    in_w, out_w = 2 * 2 * N, total * (n_out + 1)
    buf = torch.full((in_w + out_w,), 5, dtype=torch.int64, device=eng.device)
    buf[:in_w] = ma.to_device(_packed(oracle, N, 2, seed=2), eng.device).view(-1)
    before = buf.clone()
    d_in, d_out = buf[:in_w].view(2, 2, N), buf[in_w:].view(total, n_out + 1)
    with pytest.raises(engine.MosfhetHipError, match="stride = 4"):
        eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, 4, out=d_out)
    with pytest.raises(engine.MosfhetHipError, match="first = 256"):
        eng.trlwe_unpack_strided_keyswitch(dksk, d_in, 2, 1, 256, 1, out=d_out[:2])
    odd = eng.load_keyswitch_key(np.zeros((300, t, 3, n_out + 1), dtype=np.uint64), bb)
    with pytest.raises(engine.MosfhetHipError, match="n_in = 300"):
        eng.trlwe_unpack_strided_keyswitch(odd, buf[:2 * 2 * 300].view(2, 2, 300), 4, 2, 0, 2, out=d_out[:4])
    odd.free()
    with pytest.raises(engine.MosfhetHipError, match="n_in = 256"):
        eng.trlwe_unpack_strided_keyswitch(dksk, buf[:1024].view(1, 2, 512), 2, 2, 0, 2, out=d_out[:2])
    table = eng.load_packing1_key(np.zeros((N, 1, 3, 2, 1024), dtype=np.uint64), bb)
    with pytest.raises(engine.MosfhetHipError, match="packing"):
        eng.trlwe_unpack_strided_keyswitch(table, d_in, total, per, first, stride, out=d_out)
    table.free()
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride, out=buf[:out_w].view(total, n_out + 1))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride, out=buf[in_w - 1:in_w - 1 + out_w].view(total, n_out + 1))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_unpack_strided(d_in, 2, 1, 255, 1, out=buf[2 * N - 1:2 * N - 1 + 2 * (N + 1)].view(2, N + 1))
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride, out=d_out)
    finally:
        other.close()
    torch.cuda.synchronize(eng.device)
    assert (buf == before).all(), "a refused call wrote to its output"
    got = ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride, out=d_out))          # adjacent buffers: fine
    assert (got == _switched(oracle, K, _rows(oracle, N, total, per, first, stride, seed=2), n_out, t, bb)).all()


@pytest.mark.gpu
def test_two_host_threads_strided(eng, oracle):
    """Two host threads, each on a stream of its own and with a pool of its own, run the strided fused key switch five times concurrently -- one at 70 samples (the
    word-lane form), one at 9 (the direct kernels, through the pool) -- at different geometries: every result == the oracle's key switch of the helper's rows."""
    import threading
    import torch
    import mosfhet_amd as ma
    N, n_out, t, bb = 256, 16, 2, 2
    K = _switch_key(oracle, N, n_out, t, bb)
    dksk = _device_key(eng, K, bb)
    jobs = []
    for total, per, first, stride in ((70, 67, 57, 3), (9, 4, 66, 63)):
        d_in = ma.to_device(_packed(oracle, N, -(-total // per), seed=2), eng.device)
        jobs.append((d_in, total, per, first, stride, _switched(oracle, K, _rows(oracle, N, total, per, first, stride, seed=2), n_out, t, bb)))
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            d_in, total, per, first, stride, want = jobs[k]
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    bad[k] += int(not (ma.to_numpy(eng.trlwe_unpack_strided_keyswitch(dksk, d_in, total, per, first, stride)) == want).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad


@pytest.mark.gpu
def test_strided_host_face(native_lib, tmp_path):
    """tests/c/trlwe_unpack_strided.c: mosfhet_trlwe_unpack_strided and mosfhet_trlwe_unpack_strided_keyswitch on host structs equal the C-ABI calls and the drop-in
    layer's loop of trlwe_extract_tlwe (+ tlwe_keyswitch) word for word, and every sample decrypts (N = 1024, n = 24, 70 samples at coefficients 24 + 25 j)."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_unpack_strided ok" in r.stdout, r.stdout
