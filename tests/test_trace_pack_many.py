"""Many LWE samples packed into one TRLWE sample by the trace, on the device (include/mosfhet_hip.h: mosfhet_hip_tlwe_trace_pack_many_batch,
mosfhet_hip_tlwe_trace_pack_many_plan; mosfhet_amd/csrc/capi_trace.inc, trace_kernels.h; include/mosfhet_compat.h: mosfhet_tlwe_trace_pack_many).

Expected words come from tests/trace_many_reference.py, which composes the oracle primitives of tests/trace_reference.py (poly_permute, trlwe_keyswitch) and the exact
negacyclic shift in the order of the definition.  Every comparison of device words with the helper is == on all words.
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
TRLWE_1024 = 2 * 1024 * 8        # bytes of one TRLWE sample at N = 1024
COUNT = {1024: 2049, 2048: 2048, 4096: 2}     # samples of a ring's case: enough for two full-depth outputs and one more sample at N = 1024, one at N = 2048


def _log2(x):
    return float(np.log2(max(float(x), 1.0)))


def _dist(oracle, a, b):
    return float(oracle.torus_dist(np.ascontiguousarray(a), np.ascontiguousarray(b)).max())


def _case(oracle, N, t, base_bit, count, sigma):
    """Key, key rows and samples of one shape, made once and left unchanged: dict(s, rows [log2 N + 2][t][2][N] torus words -- the log2 N trace keys and two more entries,
    so that entry0 = 2 has a set long enough --, dft = their transforms, msgs = mu_j / (16 N) with distinct mu_j mod 16 for neighbours, cts [count][N + 1] under s as
    the extracted ring key)"""
    import trace_reference as R
    key = (N, t, base_bit, count, sigma)
    if key not in _CACHE:
        rng = oracle.Rng(0x3A27 + 131 * N + 17 * t + base_bit)
        s = oracle.gen_binary_key(rng, N)
        rows = np.concatenate([R.gen_trace_keys(oracle, rng, s, t, base_bit, sigma), R.gen_gadget_keys(oracle, rng, s, t, base_bit, sigma)])
        msgs = ((np.arange(count, dtype=U64) * U64(7) + U64(3)) % U64(16)) << U64(60 - R.log2n(N))
        cts = np.stack([oracle.tlwe_sample(rng, m, s, sigma) for m in msgs])
        _CACHE[key] = dict(s=s, rows=rows, dft=oracle.ks_to_dft(rows), msgs=msgs, cts=cts)
    return _CACHE[key]


def _want(oracle, D, t, base_bit, N, L, total, entry0=0):
    """the helper's words for the first `total` samples of the case, computed once"""
    import trace_many_reference as RM
    import trace_reference as R
    key = ("want", id(D), L, total, entry0)
    if key not in _CACHE:
        _CACHE[key] = RM.pack_many(oracle, D["cts"][:total], L, D["dft"][entry0:entry0 + R.log2n(N)], t, base_bit, N)
    return _CACHE[key]


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_helper_at_log_per_0_is_the_trace(oracle):
    """L = 0: the helper's tail is the whole trace in the same order, == tests/trace_reference.py::trace_pack on every word (N = 1024, t 4 / base_bit 9 and t 2 / 8)."""
    import trace_many_reference as RM
    import trace_reference as R
    N = 1024
    for t, bb in ((4, 9), (2, 8)):
        D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
        got = RM.pack_many(oracle, D["cts"][:3], 0, D["dft"][:10], t, bb, N)
        assert got.shape == (3, 2, N) and (got == R.trace_pack_batch(oracle, D["cts"][:3], D["dft"][:10], t, bb, N)).all()


def test_helper_merge_is_eval_automorphism(oracle):
    """Each merge of the helper == U + oracle.trlwe_eval_automorphism(V, 2^lvl + 1, key[log2 N - lvl]) bit for bit, at every level of a full-depth tree walked along
    its first branch (N = 1024; t 4 / base_bit 9 and t 2 / 8): the merge is the composition the device's existing automorphism call computes, as
    test_trace_step_is_eval_automorphism shows for the trace step.  The shift is checked against the polynomial product with X^s."""
    import trace_many_reference as RM
    import trace_reference as R
    N = 1024
    rng = np.random.default_rng(5)
    p = rng.integers(0, 2 ** 64, size=N, dtype=U64)
    for s in (0, 1, 256, 512, 1023):
        mono = np.zeros(N, dtype=U64)
        mono[s] = 1
        assert (RM.shift(p, s) == oracle.poly_naive_mul(mono, p)).all(), s
    for t, bb in ((4, 9), (2, 8)):
        D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
        E, P1 = R.embed(D["cts"][0], N), R.embed(D["cts"][1], N)
        for lvl in range(1, 11):
            res, U, V = RM.merge(oracle, E, P1, lvl, D["dft"], t, bb, N)
            with np.errstate(over="ignore"):
                other = U + oracle.trlwe_eval_automorphism(V, (1 << lvl) + 1, np.ascontiguousarray(D["dft"][10 - lvl]), t, bb)
            assert (res == other).all(), (t, bb, lvl)
            E, P1 = res, R.embed(D["cts"][2 + lvl % 7], N)        # (any second operand: only the words are compared)


DECRYPT_SHAPES = [(1024, 2.0 ** -45, 1), (1024, 2.0 ** -45, 3), (1024, 2.0 ** -45, 10), (2048, 2.0 ** -50, 2)]


@pytest.mark.parametrize("shape", DECRYPT_SHAPES)
def test_helper_decrypts(oracle, shape):
    """t 4, base_bit 9; 2n + 1 samples with messages mu_j / (16 N) (n + 3 at L = 10): the helper's outputs have phase N m_j at coefficient j N / n and 0 elsewhere within
    2^58, the reference's bound for the trace (test/tests.c:850).  Measured on other keys: 2^38.8 .. 2^43.3 (the figure of this file's keys is printed).  Zero masks
    give a = 0, b[j N / n] = N in[j].b and 0 elsewhere exactly: every digit is zero."""
    import trace_many_reference as RM
    N, sigma, L = shape
    t, bb, n = 4, 9, 1 << L
    total = n + 3 if L == 10 else 2 * n + 1
    D = _case(oracle, N, t, bb, COUNT[N], sigma)
    want = _want(oracle, D, t, bb, N, L, total)
    exp = RM.expected_phase(D["msgs"][:total], L, N)
    worst = max(_dist(oracle, oracle.trlwe_phase(want[o], D["s"].reshape(1, N)), exp[o]) for o in range(len(want)))
    print("N %d L %d: phase - expected = 2^%.1f" % (N, L, _log2(worst)))
    assert len(want) == -(-total // n) and worst <= 2.0 ** 58, _log2(worst)
    zero = np.zeros((min(n, 5), N + 1), dtype=U64)
    zero[:, N] = U64(0x0123456789ABCDEF) + np.arange(len(zero), dtype=U64)
    z = RM.pack_many(oracle, zero, L, D["dft"], t, bb, N)
    assert z.shape == (1, 2, N) and (z[0, 0] == 0).all() and (z[0, 1] == RM.expected_phase(zero[:, N], L, N)[0]).all()


def _many(native_lib):
    f = native_lib.mosfhet_hip_tlwe_trace_pack_many_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    p = native_lib.mosfhet_hip_tlwe_trace_pack_many_plan
    p.argtypes = [C.c_int] * 7 + [C.c_longlong, C.c_void_p]
    return f, p


def test_many_symbols_and_argument_checks(native_lib):
    """The library exports the two entry points and the host face, the binding its functions; every refusal returns MOSFHET_HIP_EINVAL with a message naming the argument
    -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); total == 0 is OK.  What a call reads off its key set (the ring,
    log_per against log2 N, a set too short for entry0, the workspace against one output) is checked by the function the call checks with,
    mosfhet_hip_tlwe_trace_pack_many_plan.  (A level whose teams do not fit one launch needs more samples than an int counts: the check stands, nothing reaches it.)"""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_tlwe_trace_pack_many_batch", "mosfhet_hip_tlwe_trace_pack_many_plan", "mosfhet_tlwe_trace_pack_many"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine.Engine, "tlwe_trace_pack_many") and hasattr(engine, "tlwe_trace_pack_many_plan")
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f, p = _many(native_lib)
    assert f(None, fake, 0, fake, fake, 1, 0, None) == EINVAL and "ctx" in err()
    assert f(fake, None, 0, fake, fake, 1, 0, None) == EINVAL and "tks" in err()
    assert f(fake, fake, 0, fake, fake, -1, 0, None) == EINVAL and "total = -1" in err()
    assert f(fake, fake, -1, fake, fake, 1, 0, None) == EINVAL and "entry0 = -1" in err()
    assert f(fake, fake, -2, fake, fake, 0, 0, None) == EINVAL and "entry0 = -2" in err()      # ... before total == 0 is accepted
    assert f(fake, fake, 0, fake, fake, 1, -1, None) == EINVAL and "log_per = -1" in err()
    assert f(fake, fake, 0, fake, fake, 0, 13, None) == EINVAL and "log_per = 13" in err()     # above log2 of the largest ring: refused without the handle
    assert f(fake, fake, 0, fake, fake, 0, 0, None) == 0                                        # total == 0: nothing to do, no handle read
    assert f(fake, fake, 5, None, None, 0, 12, None) == 0
    assert f(fake, fake, 0, None, fake, 1, 3, None) == EINVAL and "null buffer" in err()
    assert f(fake, fake, 0, fake, None, 1, 3, None) == EINVAL and "null buffer" in err()
    plan = (C.c_longlong * 8)()
    assert p(1024, 4, 9, 10, 0, 1, 0, 0, None) == EINVAL and "plan" in err()
    assert p(512, 4, 9, 10, 0, 1, 0, 0, plan) == EINVAL and "N = 512" in err()
    assert p(8192, 4, 9, 13, 0, 1, 0, 0, plan) == EINVAL and "N = 8192" in err()
    assert p(1024, 0, 9, 10, 0, 1, 0, 0, plan) == EINVAL and "t = 0" in err()
    assert p(1024, 8, 8, 10, 0, 1, 0, 0, plan) == EINVAL and "base_bit = 8" in err()
    assert p(1024, 4, 9, 10, 0, -1, 0, 0, plan) == EINVAL and "total = -1" in err()
    assert p(1024, 4, 9, 10, -1, 1, 0, 0, plan) == EINVAL and "entry0 = -1" in err()
    assert p(1024, 4, 9, 10, 0, 1, -1, 0, plan) == EINVAL and "log_per = -1" in err()
    assert p(1024, 4, 9, 10, 0, 1, 3, -1, plan) == EINVAL and "workspace_bytes = -1" in err()
    for N, steps in ((1024, 10), (2048, 11), (4096, 12)):
        assert p(N, 4, 9, steps, 0, 1, steps + 1, 0, plan) == EINVAL and "log_per = %d" % (steps + 1) in err()
        assert p(N, 4, 9, steps, 0, 1, steps, 0, plan) == 0 and plan[3] == N - 1 and plan[4] == 0
        for L in (0, 1, steps):          # every call reads all log2 N entries, whatever log_per
            assert p(N, 4, 9, steps - 1, 0, 1, L, 0, plan) == EINVAL and "holds %d entries" % (steps - 1) in err() and "entry0 + %d" % steps in err()
            assert p(N, 4, 9, steps + 1, 2, 1, L, 0, plan) == EINVAL and "entry0 = 2" in err()
            assert p(N, 4, 9, steps + 2, 2, 1, L, 0, plan) == 0
    assert p(1024, 4, 9, 0, 0, 1, 0, 0, plan) == EINVAL and "holds 0 entries" in err()
    assert p(1024, 4, 9, 10, 0, 1, 3, 6 * TRLWE_1024 - 1, plan) == EINVAL and "workspace" in err()      # one output's levels: n / 2 + n / 4 = 6 samples
    assert p(1024, 4, 9, 10, 0, 1, 3, 6 * TRLWE_1024, plan) == 0
    assert p(1024, 4, 9, 10, 0, 1, 1, 1, plan) == 0 and plan[7] == 0                                    # one level: nothing between the leaves and the output


def test_many_plan_values(native_lib):
    """The plan at N = 1024 (t 4, base_bit 9), log_per 0 / 3 / 10, total 1 / 9 / 2049 -- a short last output at 9 and 2049 -- at the default workspace and at a small
    one that forces a round split; log_per 1 and 2 for the pool's first sizes.  { outputs, launches per round, teams of a round's first launch, merges per output,
    tail steps, outputs per round, rounds, pool bytes per round }: the pool of one output is n / 2 samples of level 1 (L >= 2) and n / 4 of level 2 (L >= 3)."""
    from mosfhet_amd import engine
    _, p = _many(native_lib)
    plan = (C.c_longlong * 8)()
    P = lambda total, L, ws=0: (p(1024, 4, 9, 10, 0, total, L, ws, plan), list(plan))[1]
    for total in (1, 9, 2049):
        assert P(total, 0) == [total, 1, total, 0, 10, total, 1, 0]
    assert P(0, 0) == [0, 1, 0, 0, 10, 0, 0, 0] and P(0, 3)[:3] == [0, 3, 0]
    one3, one10 = 6 * TRLWE_1024, (512 + 256) * TRLWE_1024
    assert P(1, 3) == [1, 3, 4, 7, 7, 1, 1, one3]
    assert P(9, 3) == [2, 3, 8, 7, 7, 2, 1, 2 * one3]
    assert P(2049, 3) == [257, 3, 257 * 4, 7, 7, 257, 1, 257 * one3]
    assert P(2049, 3, 100 * one3 + 5) == [257, 3, 400, 7, 7, 100, 3, 100 * one3]
    assert P(9, 3, one3) == [2, 3, 4, 7, 7, 1, 2, one3]
    assert P(1, 10) == [1, 10, 512, 1023, 0, 1, 1, one10]
    assert P(9, 10) == [1, 10, 512, 1023, 0, 1, 1, one10]
    assert P(2049, 10) == [3, 10, 3 * 512, 1023, 0, 3, 1, 3 * one10]
    assert P(2049, 10, 2 * one10) == [3, 10, 2 * 512, 1023, 0, 2, 2, 2 * one10]
    assert P(2049, 10, one10) == [3, 10, 512, 1023, 0, 1, 3, one10]
    assert P(9, 1) == [5, 1, 5, 1, 9, 5, 1, 0]
    assert P(9, 2) == [3, 2, 6, 3, 8, 3, 1, 3 * 2 * TRLWE_1024]
    # the workspace setting is the one tlwe_pack has; 0 in the plan means the current setting
    engine.set_tlwe_pack_workspace(one10)
    try:
        assert P(2049, 10) == [3, 10, 512, 1023, 0, 1, 3, one10]
    finally:
        engine.set_tlwe_pack_workspace(0)
    assert P(2049, 10)[5] == 3
    assert engine.tlwe_trace_pack_many_plan(1024, 4, 9, 10, 9, 3) == dict(outputs=2, launches_per_round=3, teams=8, merge_steps=7, tail_steps=7, outputs_per_round=2, rounds=1,
                                                                           pool_bytes=2 * one3)
    with pytest.raises(engine.MosfhetHipError, match="log_per = 11"):
        engine.tlwe_trace_pack_many_plan(1024, 4, 9, 10, 9, 11)


def test_many_kernels_of_the_build(native_lib):
    """The merge is a run-time kind of trace_conversions_kernel, not a kernel: tools/kernel_table.py still lists that kernel once per ring, all without scratch, and
    fewer than 330 kernels in all; tools/check_lds_barriers.py found nothing on the build."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    mine = sorted((r for r in rows if r["name"].startswith("trace_conversions_kernel")), key=lambda r: r["lds"])
    for r in mine:
        print("%-70s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    assert len(mine) == 3 and "1024" in mine[0]["name"] and "2048" in mine[1]["name"] and "4096" in mine[2]["name"], [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0, r
    print("%d kernels in the library" % len(rows))
    assert len(rows) < 330, len(rows)
    with open(os.path.join(ROOT, "mosfhet_amd", "build", "lds_barrier_check.txt")) as fh:
        report = fh.read()
    assert ", 0 violations" in report, report


def _compile_c(tmp_path):
    exe = str(tmp_path / "trace_pack_many")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trace_pack_many.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_many_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trace_pack_many.c compiles against include/mosfhet.h and links against the built library (its device part: test_many_host_face)."""
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


def _run(eng, tks, cts, L, entry0=0):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.tlwe_trace_pack_many(tks, ma.to_device(np.ascontiguousarray(cts), eng.device), L, entry0))


def _same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), "%s: %d words differ, outputs %s" % (what, (got != want).sum(), sorted(set(np.nonzero(got != want)[0]))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [0, 1, 2, 3, 10])
@pytest.mark.parametrize("tb", [(2, 8), (3, 10), (4, 9)])
def test_many_bit_exact_1024(eng, oracle, tb, L):
    """N = 1024, n = 2^L: 2n + 1 samples (a last output of one sample), n samples (one full output) and 3 samples (fewer than n from L = 2 on) equal the helper on every
    word, with entry0 = 0 and with entry0 = 2 on the same set of log2 N + 2 entries (the helper then composes entries 2 .. 11 in the same way)."""
    t, bb = tb
    N, n = 1024, 1 << L
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
    tks = _tks(eng, D, bb)
    for entry0 in (0, 2):
        whole = _want(oracle, D, t, bb, N, L, 2 * n + 1, entry0)
        _same(_run(eng, tks, D["cts"][:2 * n + 1], L, entry0), whole, "L %d total %d entry0 %d" % (L, 2 * n + 1, entry0))
        _same(_run(eng, tks, D["cts"][:n], L, entry0), whole[:1], "L %d total %d entry0 %d" % (L, n, entry0))
        _same(_run(eng, tks, D["cts"][:3], L, entry0), _want(oracle, D, t, bb, N, L, 3, entry0), "L %d total 3 entry0 %d" % (L, entry0))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2048, 4, 9, 2, 8), (2048, 4, 9, 11, 2048), (4096, 2, 8, 1, 2)])
def test_many_bit_exact_wide_rings(eng, oracle, shape):
    """N = 2048 with log_per 2, total 8 and with log_per 11, total 2048 (the full-depth tree: no tail); N = 4096 with log_per 1, total 2: == the helper."""
    N, t, bb, L, total = shape
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -50)
    _same(_run(eng, _tks(eng, D, bb), D["cts"][:total], L), _want(oracle, D, t, bb, N, L, total), "N %d L %d" % (N, L))


@pytest.mark.gpu
def test_many_log_per_0_is_the_trace_call(eng, oracle):
    """log_per = 0 == tlwe_trace_pack on the same device buffer, word for word (N = 1024 t 4 base_bit 9, 67 samples, entry0 0 and 2; N = 2048, 2 samples)."""
    import torch
    import mosfhet_amd as ma
    for N, t, bb, count, sigma in ((1024, 4, 9, 67, 2.0 ** -45), (2048, 4, 9, 2, 2.0 ** -50)):
        D = _case(oracle, N, t, bb, COUNT[N], sigma)
        tks = _tks(eng, D, bb)
        d_in = ma.to_device(D["cts"][:count], eng.device)
        for entry0 in (0, 2) if N == 1024 else (0,):
            a, b = eng.tlwe_trace_pack_many(tks, d_in, 0, entry0), eng.tlwe_trace_pack(tks, d_in, entry0)
            torch.cuda.synchronize(eng.device)
            assert torch.equal(a, b), (N, entry0)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 3, 10])
def test_many_edge_rows_sentinel_and_input(eng, oracle, L):
    """N = 1024 (t 4, base_bit 9), two outputs and a third of one sample.  Output 0: zero masks -- compared with the exact words a = 0, b[j N / n] = N in[j].b, not only with
    the helper.  Output 1: a row with b = 0, mask words all 0 / 2^63 / 2^64 - 1 and words on both sides of every digit boundary (as far as n rows reach; the others keep
    their random masks).  Three more batches hold a single non-zero sample at j = 0, at j = n / 2 (the first shifted operand) and at j = n - 1, every b = 0 besides.
    The output buffer is one sample longer and sentinel-filled: the tail stays untouched; the input is unchanged."""
    import torch
    import mosfhet_amd as ma
    import trace_many_reference as RM
    import trace_reference as R
    N, t, bb, n = 1024, 4, 9, 1 << L
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
    tks = _tks(eng, D, bb)
    cts = D["cts"][:2 * n + 1].copy()
    cts[:n, :N] = 0
    edges = R.digit_boundary_words(t, bb)
    rows = [np.zeros(N, dtype=U64), np.full(N, U64(1) << U64(63)), np.full(N, U64(0xFFFFFFFFFFFFFFFF)), edges[np.arange(N) % len(edges)], edges[(np.arange(N) + 5) % len(edges)]]
    for k, row in enumerate(rows):
        cts[n + (k * (n - 1)) // (len(rows) - 1), :N] = row          # spread over the output: first, last and rows between
    cts[n + n // 2, N] = 0
    d_in = ma.to_device(cts, eng.device)
    before = d_in.clone()
    sentinel = 0x5EA75EA75EA75EA7
    d_out = torch.full((4, 2, N), sentinel, dtype=torch.int64, device=eng.device)
    eng.tlwe_trace_pack_many(tks, d_in, L, out=d_out[:3])
    torch.cuda.synchronize(eng.device)
    got = ma.to_numpy(d_out)
    assert (got[3] == U64(sentinel)).all(), "the call wrote past its last output"
    assert torch.equal(d_in, before), "the call changed its input"
    _same(got[:3], RM.pack_many(oracle, cts, L, D["dft"][:10], t, bb, N), "edge rows, L %d" % L)
    assert (got[0, 0] == 0).all() and (got[0, 1] == RM.expected_phase(cts[:n, N], L, N)[0]).all(), "zero masks: not the exact words"
    for j in (0, n // 2, n - 1):
        lone = np.zeros((n, N + 1), dtype=U64)
        lone[j] = D["cts"][7]
        _same(_run(eng, tks, lone, L), RM.pack_many(oracle, lone, L, D["dft"][:10], t, bb, N), "a single sample at j = %d, L %d" % (j, L))
    allb0 = D["cts"][:n].copy()
    allb0[:, N] = 0
    _same(_run(eng, tks, allb0, L), RM.pack_many(oracle, allb0, L, D["dft"][:10], t, bb, N), "all b = 0, L %d" % L)


@pytest.mark.gpu
def test_many_outputs_rounds_and_stale_pool(eng, oracle):
    """N = 1024 (t 4, base_bit 9), L = 3, 37 samples (5 outputs, the last of 5 samples).  Output o of the batch == its samples packed alone; a workspace that holds one
    output (5 rounds) and one that holds two (3 rounds, the last short) give the words of the default; so does a call that follows a call of another size and another
    log_per, whose levels still lie in the pool.  All == the helper."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, t, bb, L, total = 1024, 4, 9, 3, 37
    n = 1 << L
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
    tks = _tks(eng, D, bb)
    want = _want(oracle, D, t, bb, N, L, total)
    whole = _run(eng, tks, D["cts"][:total], L)
    _same(whole, want, "37 samples")
    for o in range(5):
        _same(_run(eng, tks, D["cts"][o * n:min(total, (o + 1) * n)], L), whole[o:o + 1], "output %d alone" % o)
    try:
        for outputs_per_round in (1, 2):
            engine.set_tlwe_pack_workspace(outputs_per_round * 6 * TRLWE_1024 + 8)
            assert engine.tlwe_trace_pack_many_plan(N, t, bb, 12, total, L)["rounds"] == -(-5 // outputs_per_round)
            _same(_run(eng, tks, D["cts"][:total], L), want, "%d outputs per round" % outputs_per_round)
    finally:
        engine.set_tlwe_pack_workspace(0)
    _run(eng, tks, D["cts"][100:100 + 600], 6)          # leaves other levels of another size in the pool
    _same(_run(eng, tks, D["cts"][:total], L), want, "after a call of another size")
    _same(_run(eng, tks, D["cts"][:3], 2), _want(oracle, D, t, bb, N, 2, 3), "L 2 after L 3")


@pytest.mark.gpu
def test_many_is_captured_in_a_graph(eng, oracle):
    """N = 1024 (t 4, base_bit 9), L = 3, 17 samples: captured on one side stream after an eager call of that size, replayed twice on different inputs copied into the
    captured buffer: each replay == the eager words, which equal the helper.  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    import trace_many_reference as RM
    N, t, bb, L, total = 1024, 4, 9, 3, 17
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
    tks = _tks(eng, D, bb)
    ins = [D["cts"][:total], D["cts"][40:40 + total]]
    xs = [ma.to_device(np.ascontiguousarray(x), eng.device) for x in ins]
    eager = [eng.tlwe_trace_pack_many(tks, x, L).clone() for x in xs]
    torch.cuda.synchronize()
    for r in range(2):
        _same(ma.to_numpy(eager[r]), RM.pack_many(oracle, ins[r], L, D["dft"][:10], t, bb, N), "eager, inputs %d" % r)
    d_in, d_out = xs[0].clone(), torch.empty_like(eager[0])
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.tlwe_trace_pack_many(tks, d_in, L, out=d_out)
    for r in (1, 0):
        d_in.copy_(xs[r])
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d_out, eager[r]), "replay on inputs %d differs from the plain call" % r
    del g


@pytest.mark.gpu
def test_two_host_threads_pack_many(eng, oracle):
    """Two host threads, each on a stream of its own and with a pool of its own, run the call five times concurrently -- one at N = 1024, L = 3, 17 samples, one at
    N = 2048, L = 2, 8 samples: every result equals the helper's words."""
    import threading
    import torch
    import mosfhet_amd as ma
    jobs = []
    for N, t, bb, count, sigma, L, total in ((1024, 4, 9, 2049, 2.0 ** -45, 3, 17), (2048, 4, 9, 2048, 2.0 ** -50, 2, 8)):
        D = _case(oracle, N, t, bb, COUNT[N], sigma)
        jobs.append((_tks(eng, D, bb), ma.to_device(D["cts"][:total], eng.device), L, _want(oracle, D, t, bb, N, L, total)))
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            tks, d_in, L, want = jobs[k]
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    bad[k] += int(not (ma.to_numpy(eng.tlwe_trace_pack_many(tks, d_in, L)) == want).all())
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
def test_many_refusals_on_the_device(eng, oracle):
    """A set too short for entry0, log_per above log2 N, d_out overlapping d_in, a workspace below one output's levels and a key of another context are refused with
    MOSFHET_HIP_EINVAL; a refused call writes nothing."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, t, bb = 1024, 4, 9
    D = _case(oracle, N, t, bb, COUNT[N], 2.0 ** -45)
    tks = _tks(eng, D, bb)
    d_in = ma.to_device(D["cts"][:8], eng.device)
    out = torch.full((1, 2, N), 7, dtype=torch.int64, device=eng.device)
    with pytest.raises(engine.MosfhetHipError, match="holds 12 entries"):
        eng.tlwe_trace_pack_many(tks, d_in, 3, 3, out=out)
    with pytest.raises(engine.MosfhetHipError, match="log_per = 11"):
        eng.tlwe_trace_pack_many(tks, d_in, 11, out=out)
    buf = torch.zeros(8 * (N + 1) + 2 * N, dtype=torch.int64, device=eng.device)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.tlwe_trace_pack_many(tks, buf[:8 * (N + 1)].view(8, N + 1), 3, out=buf[7 * (N + 1):7 * (N + 1) + 2 * N].view(1, 2, N))
    engine.set_tlwe_pack_workspace(6 * TRLWE_1024 - 8)
    try:
        with pytest.raises(engine.MosfhetHipError, match="workspace"):
            eng.tlwe_trace_pack_many(tks, d_in, 3, out=out)
    finally:
        engine.set_tlwe_pack_workspace(0)
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.tlwe_trace_pack_many(tks, d_in, 3, out=out)
    finally:
        other.close()
    torch.cuda.synchronize(eng.device)
    assert (out == 7).all() and (buf == 0).all(), "a refused call wrote to its output"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DECRYPT_SHAPES)
def test_many_decrypts(eng, oracle, shape):
    """The shapes of test_helper_decrypts on the device: the phase of every output is N m_j at coefficient j N / n and 0 elsewhere within the helper's own error (computed
    here and printed) plus two bits, and within 2^58."""
    import trace_many_reference as RM
    N, sigma, L = shape
    t, bb, n = 4, 9, 1 << L
    total = n + 3 if L == 10 else 2 * n + 1
    D = _case(oracle, N, t, bb, COUNT[N], sigma)
    got, want = _run(eng, _tks(eng, D, bb), D["cts"][:total], L), _want(oracle, D, t, bb, N, L, total)
    exp = RM.expected_phase(D["msgs"][:total], L, N)
    s1 = D["s"].reshape(1, N)
    for o in range(len(want)):
        helper = _dist(oracle, oracle.trlwe_phase(want[o], s1), exp[o])
        d = _dist(oracle, oracle.trlwe_phase(got[o], s1), exp[o])
        print("N %d L %d output %d: device 2^%.1f, helper 2^%.1f from the expected phase" % (N, L, o, _log2(d), _log2(helper)))
        assert d <= 4 * max(helper, 1.0) and d <= 2.0 ** 58, (o, _log2(d), _log2(helper))


@pytest.mark.gpu
def test_many_host_face(native_lib, tmp_path):
    """tests/c/trace_pack_many.c: mosfhet_tlwe_trace_pack_many of 9 samples on host structs (log_per 2) decrypts to N m_j at j N / 4 within 2^58, equals the flat device
    call word for word, and gives mosfhet_tlwe_trace_pack's words at log_per 0."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trace_pack_many ok" in r.stdout, r.stdout
