"""Encrypted polynomial-weight linear layers on packed TRLWE samples (include/mosfhet_hip.h: mosfhet_hip_gswlinear_*, mosfhet_hip_trlwe_gsw_linear_batch,
mosfhet_hip_trlwe_gsw_linear_extract_batch, mosfhet_hip_trlwe_gsw_linear_plan; mosfhet_amd/csrc/capi_gswlinear.inc, gsw_digits_body and gsw_sum_body in trace_kernels.h;
include/mosfhet_compat.h: mosfhet_trlwe_gsw_linear, mosfhet_trlwe_gsw_linear_extract).

Expected words come from tests/trlwe_gsw_linear_reference.py: the contract restated from the oracle's primitives (poly_decompose_i, torus_to_dft, dft_mul_addto,
dft_to_torus, trlwe_extract_tlwe, trgsw_to_dft).  Every device comparison is == on all words.  The two decryption bounds are half a message slot (2^59 for four-bit
values in slots of 2^60) and, for the weight made by the gadget conversion, the 2^57 tests/test_trace_conversions.py holds that conversion to."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trlwe_gsw_linear_reference import csr_of_dense, dot_layout, extracted, restatement, trgsw_of_polynomial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U64 = np.uint64
_CACHE = {}
GADGETS = [(1024, 2, 8), (2048, 4, 9), (1024, 1, 23), (4096, 1, 22), (1024, 6, 7)]


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("N,l,Bg_bit", GADGETS)
def test_restatement_against_the_external_product(oracle, N, l, Bg_bit):
    """A single entry and no bias: the restatement == oracle.external_product (reference product order) on every word, uniform torus words in sample and TRGSW rows.
    The code under test plays no part."""
    rng = np.random.default_rng([0x65A, N, l, Bg_bit])
    c = rng.integers(0, 2 ** 64, size=(2, N), dtype=U64)
    g = rng.integers(0, 2 ** 64, size=(2 * l, 2, N), dtype=U64)
    with oracle.product_order("reference"):
        want = oracle.external_product(c, oracle.trgsw_to_dft(g, 1, l), l, Bg_bit)
    got = restatement(oracle, [0, 1], [0], g[None], None, c[None, None], l, Bg_bit)[0, 0]
    assert (got == want).all(), (got != want).sum()


def test_gswlinear_symbols_and_argument_checks(native_lib):
    """The library exports the new entry points and the binding its functions; every refusal that needs no device returns MOSFHET_HIP_EINVAL with a message naming the
    argument -- on fake pointers, before any handle is read and before any HIP call (this runs without a GPU); count == 0 is OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_gswlinear_create_dense", "mosfhet_hip_gswlinear_create_sparse", "mosfhet_hip_gswlinear_create_from_selectors", "mosfhet_hip_gswlinear_destroy",
                 "mosfhet_hip_gswlinear_info", "mosfhet_hip_gswlinear_clone", "mosfhet_hip_trlwe_gsw_linear_batch", "mosfhet_hip_trlwe_gsw_linear_extract_batch",
                 "mosfhet_hip_trlwe_gsw_linear_plan", "mosfhet_trlwe_gsw_linear", "mosfhet_trlwe_gsw_linear_extract"):
        assert hasattr(native_lib, name), name
    assert hasattr(engine, "trlwe_gsw_linear_plan")
    for name in ("gswlinear_create_dense", "gswlinear_create_sparse", "gswlinear_create_from_selectors", "clone_gswlinear", "trlwe_gsw_linear", "trlwe_gsw_linear_extract"):
        assert hasattr(engine.Engine, name), name
    for name in ("info", "close"):
        assert hasattr(engine.GswLinearMap, name), name
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below ends on its scalar arguments
    f = native_lib.mosfhet_hip_trlwe_gsw_linear_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    assert f(None, fake, fake, fake, 1, None) == EINVAL and "ctx" in err()
    assert f(fake, None, fake, fake, 1, None) == EINVAL and "lin" in err()
    assert f(fake, fake, fake, fake, -1, None) == EINVAL and "count = -1" in err()
    assert f(fake, fake, None, fake, 1, None) == EINVAL and "null buffer" in err()
    assert f(fake, fake, fake, None, 1, None) == EINVAL and "null buffer" in err()
    assert f(fake, fake, fake, fake, 0, None) == 0                              # count == 0: nothing to do, no handle read
    assert f(fake, fake, None, None, 0, None) == 0
    x = native_lib.mosfhet_hip_trlwe_gsw_linear_extract_batch
    x.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert x(None, fake, fake, fake, 0, 1, None) == EINVAL and "ctx" in err()
    assert x(fake, None, fake, fake, 0, 1, None) == EINVAL and "lin" in err()
    assert x(fake, fake, fake, fake, 0, -2, None) == EINVAL and "count = -2" in err()
    assert x(fake, fake, fake, fake, -1, 1, None) == EINVAL and "idx = -1" in err()
    assert x(fake, fake, fake, fake, -1, 0, None) == EINVAL and "idx = -1" in err()       # ... before count == 0 returns
    assert x(fake, fake, None, fake, 0, 1, None) == EINVAL and "null buffer" in err()
    assert x(fake, fake, fake, fake, 0, 0, None) == 0
    d = native_lib.mosfhet_hip_gswlinear_create_dense
    d.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5
    out = C.c_void_p()
    assert d(None, C.byref(out), fake, None, 2, 2, 1024, 2, 8) == EINVAL and "ctx" in err()
    assert d(fake, None, fake, None, 2, 2, 1024, 2, 8) == EINVAL and "out" in err()
    assert d(fake, C.byref(out), fake, None, 0, 2, 1024, 2, 8) == EINVAL and "rows_out = 0" in err()
    assert d(fake, C.byref(out), fake, None, 2, -1, 1024, 2, 8) == EINVAL and "rows_in = -1" in err()
    assert d(fake, C.byref(out), fake, None, 2, 2, 512, 2, 8) == EINVAL and "N = 512" in err()
    assert d(fake, C.byref(out), None, None, 2, 2, 1024, 2, 8) == EINVAL and "h_W" in err()
    for l, Bg_bit in ((0, 8), (7, 8), (2, 0), (2, 32), (1, 40), (4, 16), (6, 11), (3, 22)):       # l outside 1 .. 6, Bg_bit outside 1 .. 31, l Bg_bit >= 64
        assert d(fake, C.byref(out), fake, None, 2, 2, 1024, l, Bg_bit) == EINVAL and ("gadget" in err() or "l = " in err()), (l, Bg_bit, err())
    s = native_lib.mosfhet_hip_gswlinear_create_sparse
    s.argtypes = [C.c_void_p] * 6 + [C.c_int] * 5
    ints = lambda *v: (C.c_int * len(v))(*v)
    assert s(None, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 1, 1024, 2, 8) == EINVAL and "ctx" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 0, 1, 1024, 2, 8) == EINVAL and "rows_out = 0" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 0, 1024, 2, 8) == EINVAL and "rows_in = 0" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 1, 3000, 2, 8) == EINVAL and "N = 3000" in err()
    assert s(fake, C.byref(out), ints(0, 1), ints(0), fake, None, 1, 1, 1024, 2, 32) == EINVAL and "gadget" in err()
    assert s(fake, C.byref(out), None, ints(0), fake, None, 1, 1, 1024, 2, 8) == EINVAL and "h_row_ptr" in err()
    assert s(fake, C.byref(out), ints(1, 2), ints(0, 0), fake, None, 1, 1, 1024, 2, 8) == EINVAL and "row_ptr[0] = 1" in err()
    assert s(fake, C.byref(out), ints(0, 2, 1), ints(0, 0), fake, None, 2, 1, 1024, 2, 8) == EINVAL and "row_ptr[2] = 1" in err()     # not monotone
    assert s(fake, C.byref(out), ints(0, 2), ints(0, 3), fake, None, 1, 3, 1024, 2, 8) == EINVAL and "col[1] = 3" in err()          # out of range
    assert s(fake, C.byref(out), ints(0, 2), ints(0, -1), fake, None, 1, 3, 1024, 2, 8) == EINVAL and "col[1] = -1" in err()
    assert s(fake, C.byref(out), ints(0, 2), None, fake, None, 1, 3, 1024, 2, 8) == EINVAL and "h_col" in err()
    assert s(fake, C.byref(out), ints(0, 2), ints(0, 1), None, None, 1, 3, 1024, 2, 8) == EINVAL and "h_W" in err()
    v = native_lib.mosfhet_hip_gswlinear_create_from_selectors
    v.argtypes = [C.c_void_p] * 6 + [C.c_int] * 5
    assert v(None, C.byref(out), fake, ints(0, 1), ints(0), None, 1, 1, 1024, 2, 8) == EINVAL and "ctx" in err()
    assert v(fake, C.byref(out), None, ints(0, 1), ints(0), None, 1, 1, 1024, 2, 8) == EINVAL and "d_sel_dft" in err()
    assert v(fake, C.byref(out), fake, None, ints(0), None, 1, 1, 1024, 2, 8) == EINVAL and "h_row_ptr" in err()
    assert v(fake, C.byref(out), fake, ints(0, 1), ints(1), None, 1, 1, 1024, 2, 8) == EINVAL and "col[0] = 1" in err()
    assert v(fake, C.byref(out), fake, ints(0, 1), ints(0), None, 1, 1, 1024, 7, 8) == EINVAL and "l = 7" in err()
    assert out.value is None                                                                                                # nothing was created
    i = native_lib.mosfhet_hip_gswlinear_info
    i.argtypes = [C.c_void_p, C.c_void_p]
    assert i(None, (C.c_longlong * 8)()) == EINVAL and "lin" in err()
    assert i(fake, None) == EINVAL and "info" in err()
    c = native_lib.mosfhet_hip_gswlinear_clone
    c.argtypes = [C.c_void_p] * 3
    assert c(None, fake, C.byref(out)) == EINVAL and "ctx_other" in err()
    assert c(fake, None, C.byref(out)) == EINVAL and "lin" in err()
    assert c(fake, fake, None) == EINVAL and "out" in err()
    assert native_lib.mosfhet_hip_gswlinear_destroy(None) == 0
    p = native_lib.mosfhet_hip_trlwe_gsw_linear_plan
    p.argtypes = [C.c_int] * 4 + [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    plan = (C.c_longlong * 8)()
    assert p(1024, 2, 2, 2, -1, 1, 0, 256, 0, None) == EINVAL and "plan" in err()
    assert p(512, 2, 2, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "N = 512" in err()
    assert p(1024, 0, 2, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "l = 0" in err()
    assert p(1024, 7, 2, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "l = 7" in err()
    assert p(1024, 2, 0, 2, -1, 1, 0, 256, 0, plan) == EINVAL and "rows_out = 0" in err()
    assert p(1024, 2, 2, 0, -1, 1, 0, 256, 0, plan) == EINVAL and "rows_in = 0" in err()
    assert p(1024, 2, 2, 2, -2, 1, 0, 256, 0, plan) == EINVAL and "nnz = -2" in err()
    assert p(1024, 2, 2, 2, -1, -1, 0, 256, 0, plan) == EINVAL and "count = -1" in err()
    assert p(1024, 2, 2, 2, -1, 1, 2, 256, 0, plan) == EINVAL and "extract = 2" in err()
    assert p(1024, 2, 2, 2, -1, 1, 0, 0, 0, plan) == EINVAL and "cus = 0" in err()
    assert p(1024, 2, 2, 2, -1, 1, 0, 256, -5, plan) == EINVAL and "workspace_bytes = -5" in err()
    assert p(1024, 2, 2, 2, -1, 1, 0, 256, 2 * 4 * 1024 * 8 - 1, plan) == EINVAL and "workspace" in err()           # below one batch element
    assert p(1024, 1, 2 ** 20, 1, 5, 2 ** 12, 0, 256, 2 ** 40, plan) == EINVAL and "do not fit one launch" in err()   # 2^32 teams in the one round
    assert p(1024, 2, 2, 2, -1, 0, 0, 256, 0, plan) == 0 and plan[0] == 0 and plan[2] == 0                         # count == 0: no round
    assert p(1024, 2, 2, 2, -1, 1, 1, 256, 0, plan) == 0


def test_gswlinear_plan_values():
    """mosfhet_hip_trlwe_gsw_linear_plan at fixed shapes: one team per (batch element, output row); the pool holds rows_in * 2l digit transforms per batch element; a
    workspace of exactly one batch element gives count rounds of rows_out teams; dense against sparse differ in the bytes a team reads only; neither extract nor cus
    changes anything; the transform counts are count rows_in 2l forward and count rows_out 2 inverse."""
    from mosfhet_amd import engine
    N, l = 1024, 2
    one = 4 * 2 * l * N * 8
    row, dig = 2 * l * 2 * N * 8, 2 * l * N * 8
    p = engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64)
    assert p == dict(teams=1024, per_round=64, rounds=1, pool_bytes=64 * one, forwards=64 * 4 * 2 * l, inverses=2048, weight_bytes=4 * row, digit_bytes=4 * dig), p
    assert engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, extract=True, cus=64) == p
    q = engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, workspace_bytes=one)
    assert q == dict(p, teams=16, per_round=1, rounds=64, pool_bytes=one), q
    q = engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, workspace_bytes=5 * one + 17)
    assert (q["per_round"], q["rounds"], q["teams"], q["pool_bytes"]) == (5, 13, 80, 5 * one), q
    with pytest.raises(engine.MosfhetHipError, match="one batch element"):
        engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, workspace_bytes=one - 1)
    s = engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, nnz=24)           # 1.5 entries per row: the mean row, rounded up
    assert s == dict(p, weight_bytes=2 * row, digit_bytes=2 * dig), s
    assert engine.trlwe_gsw_linear_plan(N, l, 16, 4, 64, nnz=64) == p     # the dense entries as a sparse handle
    e = engine.trlwe_gsw_linear_plan(N, l, 3, 4, 7, nnz=0)
    assert (e["teams"], e["forwards"], e["inverses"], e["weight_bytes"], e["digit_bytes"]) == (21, 7 * 4 * 4, 42, 0, 0), e
    big = engine.trlwe_gsw_linear_plan(4096, 1, 2, 3, 5)
    assert big == dict(teams=10, per_round=5, rounds=1, pool_bytes=5 * 3 * 2 * 4096 * 8, forwards=30, inverses=20, weight_bytes=3 * 2 * 2 * 4096 * 8,
                       digit_bytes=3 * 2 * 4096 * 8), big
    six = engine.trlwe_gsw_linear_plan(2048, 6, 1, 1, 1)
    assert (six["forwards"], six["pool_bytes"], six["weight_bytes"]) == (12, 12 * 2048 * 8, 12 * 2 * 2048 * 8), six


def test_gswlinear_kernels_of_the_build(native_lib):
    """The new bodies are run-time kinds of trace_conversions_kernel: that kernel is still listed once per ring, without scratch; the library holds exactly 329 kernels;
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
    exe = str(tmp_path / "trlwe_gsw_linear")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "trlwe_gsw_linear.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_gswlinear_c_program_compiles_and_links(native_lib, tmp_path):
    """tests/c/trlwe_gsw_linear.c compiles with -Wall -Werror against include/mosfhet.h and links against the built library (its device part:
    test_gswlinear_host_face)."""
    assert os.path.exists(_compile_c(tmp_path))


def _inner_product_case(oracle, N, l, Bg_bit, sigma, seed, rows_out=2, rows_in=2, count=1, per=32):
    """`per` four-bit values per sample at coefficients 0 .. per - 1 in slots of 2^60 under a ring key, weights in [-8, 8) laid out as mosfhet_polylinear_dot_layout
    lays them out, each weight polynomial encrypted as a TRGSW sample"""
    rng = oracle.Rng(seed)
    s = oracle.gen_binary_key(rng, N).reshape(1, N)
    nrng = np.random.default_rng(seed)
    vals = nrng.integers(0, 16, size=(count, rows_in, per))
    w = nrng.integers(-8, 8, size=(rows_out, rows_in, per), dtype=np.int64)
    x = np.empty((count, rows_in, 2, N), dtype=U64)
    for b in range(count):
        for i in range(rows_in):
            m = np.zeros(N, dtype=U64)
            m[:per] = vals[b, i].astype(U64) << U64(60)
            x[b, i] = oracle.trlwe_sample(rng, m, s, sigma)
    W = np.stack([np.stack([trgsw_of_polynomial(oracle, rng, dot_layout(w[j, i], N), s, l, Bg_bit, sigma) for i in range(rows_in)]) for j in range(rows_out)])
    return dict(s=s, x=x, W=W, want=np.einsum("jic,bic->bj", w, vals) % 16)


def _worst_phase_distance(oracle, D, out):
    worst = 0.0
    for b in range(out.shape[0]):
        for j in range(out.shape[1]):
            ph = oracle.trlwe_phase(np.ascontiguousarray(out[b, j]), D["s"])[0]
            worst = max(worst, float(oracle.torus_dist(ph, U64(int(D["want"][b, j]) << 60))))
    return worst


def test_inner_products_decrypt_on_the_restatement(oracle):
    """N = 2048, l = 4, Bg_bit = 9, sigma = 2^-44, rows_in = 2: 32 four-bit values per sample, weights in [-8, 8) encrypted as TRGSW samples; coefficient 0 of the
    restatement decrypts to sum w x within half a slot, 2^59 (the issue measured 2^36.3 as the worst of three seeds).  The code under test plays no part."""
    D = _inner_product_case(oracle, 2048, 4, 9, 2.0 ** -44, 0x1A7E)
    out = restatement(oracle, *csr_of_dense(D["W"]), None, D["x"], 4, 9)
    worst = _worst_phase_distance(oracle, D, out)
    print("inner products of 64 four-bit values with encrypted weights in [-8, 8): worst distance from sum w x 2^%.1f (half a slot: 2^59)" % np.log2(max(worst, 1.0)))
    assert worst < 2.0 ** 59


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def _case(oracle, N, l, Bg_bit, rows_out, rows_in, count):
    """uniform torus words in inputs, TRGSW rows and bias, and the restatement's words for the TRLWE mode with and without bias; made once per shape and left unchanged"""
    key = ("case", N, l, Bg_bit, rows_out, rows_in, count)
    if key not in _CACHE:
        rng = np.random.default_rng([0x65A11, N, l, Bg_bit, rows_out, rows_in, count])
        x = rng.integers(0, 2 ** 64, size=(count, rows_in, 2, N), dtype=U64)
        W = rng.integers(0, 2 ** 64, size=(rows_out, rows_in, 2 * l, 2, N), dtype=U64)
        bias = rng.integers(0, 2 ** 64, size=(rows_out, N), dtype=U64)
        csr = csr_of_dense(W)
        plain = restatement(oracle, *csr, None, x, l, Bg_bit)
        biased = plain.copy()
        biased[:, :, 1] += bias[None]
        _CACHE[key] = dict(x=x, W=W, bias=bias, csr=csr, plain=plain, biased=biased)
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


SHAPES = [(1024, 2, 8, 1, 1, 1), (1024, 2, 8, 2, 3, 2), (1024, 2, 8, 3, 2, 5), (1024, 1, 23, 2, 2, 2), (1024, 6, 7, 2, 2, 2), (2048, 4, 9, 2, 2, 2), (4096, 1, 22, 1, 2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg_bit,rows_out,rows_in,count", SHAPES)
def test_gswlinear_dense_bit_exact(eng, oracle, N, l, Bg_bit, rows_out, rows_in, count):
    """Dense handles, with and without bias: the TRLWE mode and the extract mode at idx 0, 1, N / 2, N - 1 == the restatement on every word; the bias lands on
    component b only (the restatement with a bias is the one without plus the bias on b: checked on the CPU for the first shape)."""
    import mosfhet_amd as ma
    D = _case(oracle, N, l, Bg_bit, rows_out, rows_in, count)
    if (rows_out, rows_in, count) == (1, 1, 1):
        assert (restatement(oracle, *D["csr"], D["bias"], D["x"], l, Bg_bit) == D["biased"]).all()
    d_x = _dev(eng, D["x"])
    for bias, want in ((None, D["plain"]), (D["bias"], D["biased"])):
        lin = eng.gswlinear_create_dense(D["W"], Bg_bit, bias)
        info = lin.info()
        assert (info["rows_out"], info["rows_in"], info["nnz"], info["N"], info["l"], info["Bg_bit"], info["form"]) == (rows_out, rows_in, -1, N, l, Bg_bit, "dense"), info
        assert info["nbytes"] >= D["W"].size * 8
        got = ma.to_numpy(eng.trlwe_gsw_linear(lin, d_x))
        assert got.shape == want.shape and (got == want).all(), "TRLWE mode, bias %s: %d words differ" % (bias is not None, (got != want).sum())
        for idx in (0, 1, N // 2, N - 1):
            got = ma.to_numpy(eng.trlwe_gsw_linear_extract(lin, d_x, idx))
            ext = extracted(oracle, want, idx)
            assert got.shape == ext.shape and (got == ext).all(), "extract at %d, bias %s: %d words differ" % (idx, bias is not None, (got != ext).sum())
        lin.close()


@pytest.mark.gpu
def test_gswlinear_sparse_and_selectors(eng, oracle):
    """N = 1024, (2, 8), rows_in = 3, count = 2: an empty row gives (0, bias); a repeated column adds, in the stored order; unsorted columns; no entry at all; and the
    same ordered entries give the same words dense, sparse and from selectors (the device transform of the same rows through mosfhet_hip_torus_to_dft_batch)."""
    import mosfhet_amd as ma
    N, l, Bg, rows_in, count = 1024, 2, 8, 3, 2
    rng = np.random.default_rng(0x5BA25E)
    x = rng.integers(0, 2 ** 64, size=(count, rows_in, 2, N), dtype=U64)
    rows = [[], [2, 2, 0, 2], [2, 0, 1], [1], []]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    W = rng.integers(0, 2 ** 64, size=(len(col), 2 * l, 2, N), dtype=U64)
    bias = rng.integers(0, 2 ** 64, size=(len(rows), N), dtype=U64)
    d_x = _dev(eng, x)
    d_sel = eng.torus_to_dft(_dev(eng, W).view(-1, N)).view(len(col), 2 * l, 2, N)
    for b in (None, bias):
        want = restatement(oracle, ptr, col, W, b, x, l, Bg)
        for form, lin in (("sparse", eng.gswlinear_create_sparse(ptr, col, W, rows_in, N, l, Bg, b)),
                          ("selectors", eng.gswlinear_create_from_selectors(d_sel, ptr, col, rows_in, Bg, b))):
            info = lin.info()
            assert (info["rows_out"], info["rows_in"], info["nnz"], info["N"], info["l"], info["Bg_bit"], info["form"]) == (len(rows), rows_in, len(col), N, l, Bg, form), info
            got = ma.to_numpy(eng.trlwe_gsw_linear(lin, d_x))
            assert (got == want).all(), "%s, bias %s: %d words differ, rows %s" % (form, b is not None, (got != want).sum(), sorted(set(np.nonzero(got != want)[1])))
            for j in (0, 4):
                assert (got[:, j, 0] == 0).all() and (got[:, j, 1] == (0 if b is None else b[j][None])).all(), "an empty row is (0, bias)"
            got = ma.to_numpy(eng.trlwe_gsw_linear_extract(lin, d_x, 7))
            assert (got == extracted(oracle, want, 7)).all(), form
            lin.close()
    empty = eng.gswlinear_create_sparse([0, 0], [], np.zeros((0, 2 * l, 2, N), dtype=U64), rows_in, N, l, Bg)     # no entry at all
    assert (ma.to_numpy(eng.trlwe_gsw_linear(empty, d_x)) == 0).all()
    empty.close()
    D = _case(oracle, N, l, Bg, 2, 3, 2)
    d_x = _dev(eng, D["x"])
    d_sel = eng.torus_to_dft(_dev(eng, D["W"]).view(-1, N)).view(6, 2 * l, 2, N)
    handles = [eng.gswlinear_create_dense(D["W"], Bg, D["bias"]), eng.gswlinear_create_sparse(*D["csr"], 3, N, l, Bg, D["bias"]),
               eng.gswlinear_create_from_selectors(d_sel, D["csr"][0], D["csr"][1], 3, Bg, D["bias"])]
    for lin in handles:
        assert (ma.to_numpy(eng.trlwe_gsw_linear(lin, d_x)) == D["biased"]).all(), "the %s handle of the dense entries differs from the restatement" % lin.info()["form"]
        lin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg_bit", [(1024, 2, 8), (1024, 6, 7), (2048, 4, 9)])
def test_gswlinear_value_edges(eng, oracle, N, l, Bg_bit):
    """Input words and TRGSW row words drawn from {0, 1, 2^63 - 1, 2^63, 2^64 - 1}, with one component all 2^63 - 1 and one all 2^63: the offset carries out of the top
    (2^63 - 1 rounds up to the digits (-Bg / 2, 0, ..)); these words alone never give the digit Bg / 2 - 1, so two more are planted -- every digit at Bg / 2 - 1, and
    every digit at -Bg / 2 -- and every level is seen to reach both ends (checked on the oracle's digits).  The general rounding still gives the restatement's words,
    TRLWE mode and extract mode."""
    import mosfhet_amd as ma
    words = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)
    rng = np.random.default_rng([0xED6E, N, l])
    x = words[rng.integers(0, len(words), size=(2, 2, 2, N))]
    x[1, 1, 0] = U64(2 ** 63 - 1)
    x[1, 1, 1] = U64(2 ** 63)
    x[1, 0, 0, ::2] = U64(2 ** 64 - 1)
    half = 1 << (Bg_bit - 1)
    x[0, 0, 0, 3] = x[0, 1, 1, N - 1] = U64(sum((half - 1) << (64 - (i + 1) * Bg_bit) for i in range(l)))
    x[0, 0, 1, 5] = x[0, 1, 0, 0] = U64(sum((-half) << (64 - (i + 1) * Bg_bit) for i in range(l)) % 2 ** 64)
    W = words[rng.integers(0, len(words), size=(2, 2, 2 * l, 2, N))]
    W[1, 1] = U64(2 ** 63)                                       # every coefficient at the edge
    bias = words[rng.integers(0, len(words), size=(2, N))]
    for i in range(l):
        digits = np.concatenate([oracle.poly_decompose_i(np.ascontiguousarray(p), Bg_bit, l, i).view(np.int64) for p in x.reshape(-1, N)])
        assert digits.min() == -half and digits.max() == half - 1, (i, digits.min(), digits.max())
    want = restatement(oracle, *csr_of_dense(W), bias, x, l, Bg_bit)
    lin = eng.gswlinear_create_dense(W, Bg_bit, bias)
    got = ma.to_numpy(eng.trlwe_gsw_linear(lin, _dev(eng, x)))
    assert (got == want).all(), "N = %d: %d words differ" % (N, (got != want).sum())
    got = ma.to_numpy(eng.trlwe_gsw_linear_extract(lin, _dev(eng, x), N - 1))
    assert (got == extracted(oracle, want, N - 1)).all(), N
    lin.close()


@pytest.mark.gpu
def test_gswlinear_run_contexts(eng, oracle):
    """(3, 2, 5) at N = 1024: a larger call on other inputs first (the pool holds its digit transforms: garbage for this one); sentinel words behind d_out stay, both
    modes; with the workspace set to one batch element the call runs count rounds and gives the same words; a position in the batch changes nothing; count == 0."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg, rows_out, rows_in, count = 1024, 2, 8, 3, 2, 5
    D = _case(oracle, N, l, Bg, rows_out, rows_in, count)
    lin = eng.gswlinear_create_dense(D["W"], Bg, D["bias"])
    d_x = _dev(eng, D["x"])
    junk = _dev(eng, np.random.default_rng(1).integers(0, 2 ** 64, size=(count + 2, rows_in, 2, N), dtype=U64))
    eng.trlwe_gsw_linear(lin, junk)
    SENT = -0x0123456789ABCDEF
    for idx, words, want in ((None, 2 * N, D["biased"]), (3, N + 1, extracted(oracle, D["biased"], 3))):
        buf = torch.full((count * rows_out * words + 64,), SENT, dtype=torch.int64, device=eng.device)
        out = buf[:count * rows_out * words].view(count, rows_out, *((2, N) if idx is None else (N + 1,)))
        if idx is None:
            eng.trlwe_gsw_linear(lin, d_x, out=out)
        else:
            eng.trlwe_gsw_linear_extract(lin, d_x, idx, out=out)
        assert (ma.to_numpy(out) == want).all() and (buf[count * rows_out * words:] == SENT).all(), idx
    one = rows_in * 2 * l * N * 8
    assert engine.trlwe_gsw_linear_plan(N, l, rows_out, rows_in, count, workspace_bytes=one)["rounds"] == count
    engine.set_tlwe_pack_workspace(one)
    try:
        assert (ma.to_numpy(eng.trlwe_gsw_linear(lin, d_x)) == D["biased"]).all(), "one batch element per round"
        assert (ma.to_numpy(eng.trlwe_gsw_linear_extract(lin, d_x, N - 1)) == extracted(oracle, D["biased"], N - 1)).all()
        engine.set_tlwe_pack_workspace(one - 8)
        with pytest.raises(engine.MosfhetHipError, match="one batch element"):
            eng.trlwe_gsw_linear(lin, d_x)
    finally:
        engine.set_tlwe_pack_workspace(0)
    back = np.ascontiguousarray(D["x"][::-1])
    assert (ma.to_numpy(eng.trlwe_gsw_linear(lin, _dev(eng, back))) == D["biased"][::-1]).all(), "a sample's position in the batch"
    assert (ma.to_numpy(eng.trlwe_gsw_linear(lin, d_x[:0])).size == 0)                 # count == 0
    assert (ma.to_numpy(eng.trlwe_gsw_linear_extract(lin, d_x[:0], 5)).size == 0)
    lin.close()


@pytest.mark.gpu
def test_gswlinear_calls_are_captured_in_a_graph(eng, oracle):
    """Both calls captured on one side stream after an eager call of the same size, replayed on fresh inputs: the replayed words == the plain call's -- no hidden
    allocation or synchronisation.  One stream, no parallel branches."""
    import torch
    import mosfhet_amd as ma
    N, l, Bg = 1024, 2, 8
    D = _case(oracle, N, l, Bg, 2, 3, 2)
    lin = eng.gswlinear_create_dense(D["W"], Bg, D["bias"])
    xs = [_dev(eng, D["x"]), _dev(eng, np.ascontiguousarray(D["x"][::-1]))]
    calls = [("trlwe", lambda i, o: eng.trlwe_gsw_linear(lin, i, out=o), (2, 2, 2, N)), ("extract", lambda i, o: eng.trlwe_gsw_linear_extract(lin, i, 9, out=o), (2, 2, N + 1))]
    side = torch.cuda.Stream(device=eng.device)
    for name, call, shape in calls:
        eager = [ma.to_numpy(call(x, eng.empty(*shape))) for x in xs]
        assert (eager[0] == (D["biased"] if name == "trlwe" else extracted(oracle, D["biased"], 9))).all()
        d_in, d_out = xs[0].clone(), eng.empty(*shape)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(d_in, d_out)
        for r in (1, 0):
            d_in.copy_(xs[r])
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert (ma.to_numpy(d_out) == eager[r]).all(), "%s: replay on inputs %d differs from the plain call" % (name, r)
        del g
    lin.close()


@pytest.mark.gpu
def test_two_host_threads_gswlinear(eng, oracle):
    """Two host threads, each on a stream of its own and with a pool of its own, run the call five times concurrently on one shared handle per shape -- (3, 2, 5) at
    N = 1024 and (2, 2, 2) at N = 2048: every result equals the restatement."""
    import threading
    import torch
    import mosfhet_amd as ma
    jobs = []
    for shape in ((1024, 2, 8, 3, 2, 5), (2048, 4, 9, 2, 2, 2)):
        D = _case(oracle, *shape)
        jobs.append((eng.gswlinear_create_dense(D["W"], shape[2], D["bias"]), _dev(eng, D["x"]), D["biased"]))
    torch.cuda.synchronize()
    bad, errors = [0, 0], []

    def worker(k):
        try:
            lin, d_in, want = jobs[k]
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(5):
                    bad[k] += int(not (ma.to_numpy(eng.trlwe_gsw_linear(lin, d_in)) == want).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert bad == [0, 0], bad
    for lin, _, _ in jobs:
        lin.close()


@pytest.mark.gpu
def test_gswlinear_refusals_on_the_device(eng, oracle):
    """idx = N, d_out overlapping d_in (the same buffer, and a partial overlap) and a handle made for another context are refused with MOSFHET_HIP_EINVAL, and nothing
    is written; the handle's clone for that context works there."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    N, l, Bg = 1024, 2, 8
    D = _case(oracle, N, l, Bg, 2, 3, 2)
    lin = eng.gswlinear_create_dense(D["W"], Bg, D["bias"])
    in_w, out_w = 2 * 3 * 2 * N, 2 * 2 * 2 * N
    buf = torch.zeros(in_w + out_w, dtype=torch.int64, device=eng.device)
    buf[:in_w] = _dev(eng, D["x"]).view(-1)
    before = buf.clone()
    d_in = buf[:in_w].view(2, 3, 2, N)
    with pytest.raises(engine.MosfhetHipError, match="idx = 1024"):
        eng.trlwe_gsw_linear_extract(lin, d_in, N)
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_gsw_linear(lin, d_in, out=buf[:out_w].view(2, 2, 2, N))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_gsw_linear(lin, d_in, out=buf[in_w - 1:in_w - 1 + out_w].view(2, 2, 2, N))
    with pytest.raises(engine.MosfhetHipError, match="d_out overlaps d_in"):
        eng.trlwe_gsw_linear_extract(lin, d_in, 0, out=buf[in_w - 1:in_w - 1 + 4 * (N + 1)].view(2, 2, N + 1))
    other = ma.Engine(0)
    try:
        with pytest.raises(engine.MosfhetHipError, match="another context"):
            other.trlwe_gsw_linear(lin, d_in, out=buf[in_w:].view(2, 2, 2, N))
        torch.cuda.synchronize(eng.device)
        assert (buf == before).all(), "a refused call wrote to its output"
        mine = other.clone_gswlinear(lin)
        assert mine.info() == lin.info()
        assert (ma.to_numpy(other.trlwe_gsw_linear(mine, d_in)) == D["biased"]).all()
        mine.close()
    finally:
        other.close()
    got = eng.trlwe_gsw_linear(lin, d_in, out=buf[in_w:].view(2, 2, 2, N))              # adjacent: fine
    assert (ma.to_numpy(got) == D["biased"]).all()
    lin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg_bit", [(1024, 2, 8), (2048, 4, 9)])
def test_single_entry_equals_the_external_product_call(eng, oracle, N, l, Bg_bit):
    """A layer of one entry and no bias == mosfhet_hip_external_product_batch on the same TRGSW (loaded as a one-entry key, product order "reference"), word for word,
    over a batch of 3."""
    import mosfhet_amd as ma
    rng = np.random.default_rng([0xE47, N])
    g = rng.integers(0, 2 ** 64, size=(1, 2 * l, 2, N), dtype=U64)
    x = rng.integers(0, 2 ** 64, size=(3, 2, N), dtype=U64)
    bsk = eng.load_bootstrap_key(g, 1, l, Bg_bit)
    bsk.set_product_order("reference")
    want = ma.to_numpy(eng.external_product(bsk, 0, _dev(eng, x)))
    lin = eng.gswlinear_create_dense(g[None], Bg_bit)
    got = ma.to_numpy(eng.trlwe_gsw_linear(lin, _dev(eng, x[:, None])))[:, 0]
    assert (got == want).all(), (got != want).sum()
    lin.close()
    bsk.free()


@pytest.mark.gpu
def test_weight_from_the_gadget_conversion_decrypts(eng, oracle):
    """N = 2048, l = 4, Bg_bit = 9 (the lvl2 gadget), key-switch key t = 4, base_bit = 9, sigma = 2^-50: gadget rows of mu = 2 - X^5, TRLWE(mu 2^(64 - (i + 1) Bg_bit)),
    become a TRGSW_DFT sample on the device through mosfhet_hip_trgsw_from_gadget_batch; the one-entry layer made from it maps a sample of four-bit messages to one whose
    phase is mu m within 2^57 on every coefficient."""
    import mosfhet_amd as ma
    import test_trace_conversions as T
    import trace_reference as R
    N, l, Bg, t, bb, sigma = 2048, 4, 9, 4, 9, 2.0 ** -50
    D = T._case(oracle, N, t, bb, 2, sigma)
    rng = oracle.Rng(0x6AD6E7)
    s1 = D["s"].reshape(1, N)
    mu = np.zeros(N, dtype=np.int64)
    mu[0], mu[5] = 2, -1
    gadget = np.stack([oracle.trlwe_sample(rng, mu.view(U64) << U64(64 - (i + 1) * Bg), s1, sigma) for i in range(l)])[None]
    m = (rng.words(N) % U64(16)) << U64(60)
    x = oracle.trlwe_sample(rng, m, s1, sigma)
    tks = eng.load_trlwe_ks_keys(D["rows"], bb)
    sel = eng.trgsw_from_gadget(tks, _dev(eng, gadget), R.log2n(N))
    lin = eng.gswlinear_create_from_selectors(sel, [0, 1], [0], 1, Bg)
    assert lin.info()["form"] == "selectors" and lin.info()["l"] == l
    out = ma.to_numpy(eng.trlwe_gsw_linear(lin, _dev(eng, x[None, None])))[0, 0]
    want = 2 * m - np.concatenate((-m[N - 5:], m[:N - 5]))            # mu m = 2 m - X^5 m mod (X^N + 1, 2^64)
    d = float(oracle.torus_dist(oracle.trlwe_phase(out, s1), want).max())
    print("weight from the gadget conversion: worst distance from mu m 2^%.1f (bound 2^57)" % np.log2(max(d, 1.0)))
    assert d < 2.0 ** 57
    lin.close()
    tks.free()


@pytest.mark.gpu
def test_gswlinear_on_the_device_decrypts(eng, oracle):
    """The inner products of test_inner_products_decrypt_on_the_restatement through the device call: the words equal the restatement's and coefficient 0 decrypts to
    sum w x within half a slot."""
    import mosfhet_amd as ma
    D = _inner_product_case(oracle, 2048, 4, 9, 2.0 ** -44, 0x1A7E)
    lin = eng.gswlinear_create_dense(D["W"], 9)
    out = ma.to_numpy(eng.trlwe_gsw_linear(lin, _dev(eng, D["x"])))
    lin.close()
    assert (out == restatement(oracle, *csr_of_dense(D["W"]), None, D["x"], 4, 9)).all()
    assert _worst_phase_distance(oracle, D, out) < 2.0 ** 59


@pytest.mark.gpu
def test_gswlinear_host_face(native_lib, tmp_path):
    """tests/c/trlwe_gsw_linear.c: at rows_in = 1 mosfhet_trlwe_gsw_linear on host structs equals the drop-in layer's trgsw_mul_trlwe_DFT + trlwe_from_DFT word for word;
    at rows_in = 2 it and mosfhet_trlwe_gsw_linear_extract decrypt to the inner products."""
    r = subprocess.run([_compile_c(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "trlwe_gsw_linear ok" in r.stdout, r.stdout[-3000:]
