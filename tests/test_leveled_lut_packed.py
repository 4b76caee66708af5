"""Leveled look-up-table evaluation with SEVERAL OUTPUTS PACKED INTO ONE TABLE (include/mosfhet_hip.h: mosfhet_hip_leveled_lut_packed_batch,
mosfhet_hip_lut_bits_packed_batch; mosfhet_amd/csrc/leveled_lut_kernels.h: lut_tables_finish_kernel with LutParams::pack_log).

An entry of a table occupies m = 2^pack_log adjacent coefficients.  The expected words of (input b, table tb) are the composition of
tests/test_leveled_lut.py::_composition with three changes -- log2 N - pack_log rotation steps at most, a[i] = int2torus(2N - 2^(i + pack_log)), and the stack of
oracle.trlwe_extract_tlwe(acc, t) for t < m as the result.  Every GPU comparison is == on all words; there is no tolerance anywhere.  The decryption bound
2^(64 - prec - 1) is a condition on the INPUTS that the oracle composition alone meets on the CPU (test_oracle_packed_composition_decrypts).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_leveled_lut import _assert_words, _map, _sel_dft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (N, l, Bg_bit, sigma, size, pack_log, tables, prec, inputs, encrypted tables, seed)
PSETS = {
    "P1": (1024, 3, 10, 2.0 ** -44, 5, 3, 1, 4, 5, False, 0x9A1),     # no tree, fewer than log2 N - p steps, table shorter than N
    "P2": (1024, 3, 10, 2.0 ** -44, 9, 2, 2, 4, 5, True, 0x9A2),      # level 0 only, 8 steps, two tables
    "P3": (2048, 4, 9, 2.0 ** -44, 8, 3, 1, 4, 5, False, 0x9A3),      # the S-box shape: one TRLWE at N = 2048, lvl2's gadget
    "P4": (1024, 2, 8, 2.0 ** -25, 12, 1, 3, 3, 5, False, 0x9A4),     # 3 tree levels (level 0 + 2 deeper), odd table count
    "P5": (1024, 3, 10, 2.0 ** -44, 10, 0, 2, 6, 3, False, 0x9A5),    # pack_log = 0
    "P6": (2048, 1, 23, 2.0 ** -52, 11, 2, 2, 4, 3, False, 0x9A6),    # the reference application's gadget, 2 levels
    "P7": (1024, 3, 10, 2.0 ** -44, 1, 9, 1, 4, 2, False, 0x9A7),     # the largest pack_log, one step, 512 extractions
}
_CACHE = {}


def _packed_composition(oracle, tabs, sel_dft, N, l, Bg, size, p):
    """test_leveled_lut._composition for entries of 2^p coefficients: [2^p][N + 1]"""
    log_N = N.bit_length() - 1
    rot = log_N - p
    T = tabs.copy()
    for i in range(max(0, size - rot)):
        half = 1 << (size - rot - i - 1)
        for j in range(half):
            T[j] = T[j] + oracle.external_product(T[j + half] - T[j], sel_dft[size - i - 1], l, Bg)
    steps = min(size, rot)
    a = np.zeros(steps, dtype=np.uint64)
    for i in range(steps):
        a[i] = ((2 * N - (1 << (i + p))) << (64 - (log_N + 1))) % 2 ** 64
    acc = oracle.blind_rotate(T[0], a, sel_dft[:steps], l, Bg)
    return np.stack([oracle.trlwe_extract_tlwe(acc, t) for t in range(1 << p)])


def _pcase(oracle, name):
    """key, tables, indices (2^size - 1 and 0 first: the extreme rotations), selectors and the oracle's outputs want[b][tb][t] of a set (cached for the module)"""
    if name in _CACHE:
        return _CACHE[name]
    N, l, Bg, sigma, size, p, tables, prec, inputs, encrypted, seed = PSETS[name]
    oracle.plan(N)       # by one thread, in front of the workers of _map
    log_N = N.bit_length() - 1
    r = oracle.Rng(seed)
    s = oracle.gen_binary_key(r, N).reshape(1, N)
    n_luts = max(1, (1 << (size + p)) >> log_N)
    # random behind a table shorter than N too: those coefficients are never selected, whatever they hold
    lut = (oracle.u64(r.words(tables * n_luts * N)) % np.uint64(1 << prec)).astype(np.uint64).reshape(tables, n_luts * N)
    msg = (lut << np.uint64(64 - prec)).reshape(tables, n_luts, N)
    tabs = np.zeros((tables, n_luts, 2, N), dtype=np.uint64)
    if encrypted:
        for tb in range(tables):
            for j in range(n_luts):
                tabs[tb, j] = oracle.trlwe_sample(r, msg[tb, j].copy(), s, sigma)
    else:
        tabs[:, :, 1, :] = msg
    rng = np.random.default_rng(seed)
    m = ([(1 << size) - 1, 0] + [int(rng.integers(0, 1 << size)) for _ in range(inputs - 2)])[:inputs]
    sel = np.stack([np.stack([oracle.trgsw_monomial_sample(r, (m[b] >> i) & 1, 0, s, l, Bg, sigma) for i in range(size)]) for b in range(inputs)])
    sel_dft = _map(lambda b: oracle.bk_to_dft(sel[b], 1, l), range(inputs))
    want = np.stack(_map(lambda u: _packed_composition(oracle, tabs[u % tables], sel_dft[u // tables], N, l, Bg, size, p), range(inputs * tables)))
    _CACHE[name] = dict(N=N, l=l, Bg=Bg, size=size, p=p, tables=tables, prec=prec, inputs=inputs, s=s, lut=lut, tabs=tabs, m=m, sel=sel,
                        want=want.reshape(inputs, tables, 1 << p, N + 1))
    return _CACHE[name]


def _worst_distance(oracle, T, outs):
    """largest torus distance of an output's phase from LUT_tb[m x_b + t], over all (input, table, t)"""
    worst, mm = 0.0, 1 << T["p"]
    for b in range(T["inputs"]):
        for tb in range(T["tables"]):
            for t in range(mm):
                want = int(T["lut"][tb][mm * T["m"][b] + t]) << (64 - T["prec"])
                worst = max(worst, float(oracle.torus_dist(oracle.tlwe_phase(outs[b, tb, t], T["s"][0]), want)))
    return worst


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_packed_symbols_and_argument_checks(native_lib):
    """The library exports the four entry points and the two host-struct calls; the packed calls refuse pack_log < 0 and > log2 N - 1, size + pack_log past the bound
    and everything the several-table call refuses with MOSFHET_HIP_EINVAL and a message naming the argument -- on fake pointers that are never dereferenced, before
    any HIP call (this runs without a GPU); count = 0 with good arguments returns OK."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_leveled_lut_packed_batch", "mosfhet_hip_leveled_lut_packed_plan", "mosfhet_hip_lut_bits_packed_batch", "mosfhet_hip_lut_bits_packed_plan",
                 "mosfhet_eval_LUTs_packed_inputs", "mosfhet_eval_LUTs_packed_bits"):
        assert hasattr(native_lib, name), name
    f = native_lib.mosfhet_hip_leveled_lut_packed_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)
    L = engine.LEVELED_LUT_MAX_LEVELS
    #              size  N    l  Bg  tables pack count
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, -1, 4, None) == -1 and "pack_log = -1" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, 10, 4, None) == -1 and "pack_log = 10" in err()
    assert f(fake, fake, fake, fake, 8, 2048, 3, 10, 1, 11, 4, None) == -1 and "pack_log = 11" in err()
    assert f(fake, fake, fake, fake, 10 + L - 2, 1024, 3, 10, 1, 3, 4, None) == -1 and "size = %d with pack_log = 3" % (10 + L - 2) in err()
    assert f(fake, fake, fake, fake, 11 + L, 2048, 3, 10, 1, 1, 4, None) == -1 and "size = %d with pack_log = 1" % (11 + L) in err()
    assert f(fake, fake, fake, fake, 10 + L + 1, 1024, 3, 10, 1, 0, 4, None) == -1 and "size = %d" % (10 + L + 1) in err()
    assert f(fake, fake, fake, fake, 0, 1024, 3, 10, 1, 3, 4, None) == -1 and "size = 0" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 0, 3, 4, None) == -1 and "tables = 0" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 65, 3, 4, None) == -1 and "tables = 65" in err()
    assert f(None, fake, fake, fake, 8, 1024, 3, 10, 1, 3, 4, None) == -1 and "ctx" in err()
    assert f(fake, fake, fake, fake, 8, 512, 3, 10, 1, 3, 4, None) == -1 and "N = 512" in err()
    assert f(fake, fake, fake, fake, 8, 4096, 3, 10, 1, 3, 4, None) == -1 and "N = 4096" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 4, 16, 1, 3, 4, None) == -1 and "l=4 Bg_bit=16" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 7, 8, 1, 3, 4, None) == -1 and "l = 7" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, 3, -1, None) == -1 and "count = -1" in err()
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, 10, 0, None) == -1 and "pack_log = 10" in err()      # count = 0 still checks the rest ...
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, 3, 0, None) == 0                                      # ... and is no error
    assert f(fake, fake, fake, fake, 8, 1024, 3, 10, 1, 0, 0, None) == 0
    plan = (C.c_longlong * 8)()
    g = native_lib.mosfhet_hip_leveled_lut_packed_plan
    assert g(1024, 3, 8, 1, 3, 4, 256, None) == -1 and "null plan" in err()
    assert g(4096, 1, 8, 1, 3, 4, 256, plan) == -1 and "N = 4096" in err()
    assert g(1024, 3, 8, 0, 3, 4, 256, plan) == -1 and "tables = 0" in err()
    assert g(1024, 3, 8, 1, -1, 4, 256, plan) == -1 and "pack_log = -1" in err()
    assert g(1024, 3, 8, 1, 10, 4, 256, plan) == -1 and "pack_log = 10" in err()
    assert g(2048, 3, 8, 1, 10, 4, 256, plan) == 0                                  # log2 N - 1 at N = 2048
    assert g(1024, 3, 10 + L, 1, 1, 4, 256, plan) == -1 and "pack_log = 1" in err()
    assert g(1024, 3, 8, 1, 3, 0, 256, plan) == -1 and "count = 0" in err()
    assert g(1024, 3, 8, 1, 3, -1, 256, plan) == -1 and "count = -1" in err()
    assert g(1024, 3, 8, 1, 3, 4, 0, plan) == -1 and "cus = 0" in err()
    # the bits variant: null handles and scalar ranges before any handle is read
    h = native_lib.mosfhet_hip_lut_bits_packed_batch
    h.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p]
    assert h(None, fake, fake, fake, None, fake, fake, fake, 8, 1, 3, 4, None) == -1 and "null ctx" in err()
    assert h(fake, None, fake, fake, None, fake, fake, fake, 8, 1, 3, 4, None) == -1 and "null bsk" in err()
    assert h(fake, fake, None, fake, None, fake, fake, fake, 8, 1, 3, 4, None) == -1 and "null kska" in err()
    assert h(fake, fake, fake, None, None, fake, fake, fake, 8, 1, 3, 4, None) == -1 and "null kskb" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 1, -1, 4, None) == -1 and "pack_log = -1" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 1, 11, 4, None) == -1 and "pack_log = 11" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 0, 1, 3, 4, None) == -1 and "size = 0" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 11 + L - 2, 1, 3, 4, None) == -1 and "size = %d with pack_log = 3" % (11 + L - 2) in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 0, 3, 4, None) == -1 and "tables = 0" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 65, 3, 4, None) == -1 and "tables = 65" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 1, 3, -1, None) == -1 and "count = -1" in err()
    assert h(fake, fake, fake, fake, None, fake, fake, fake, 8, 1, 3, 0, None) == 0
    plan12 = (C.c_longlong * 12)()
    k = native_lib.mosfhet_hip_lut_bits_packed_plan
    assert k(2048, 4, 8, 1, 3, 4, 256, None) == -1 and "null plan" in err()
    assert k(2048, 4, 8, 1, 11, 4, 256, plan12) == -1 and "pack_log = 11" in err()
    assert k(2048, 4, 8, 1, 3, -1, 256, plan12) == -1 and "count = -1" in err()
    assert k(2048, 4, 8, 1, 3, 4, 0, plan12) == -1 and "cus = 0" in err()


def test_packed_plan_sweep(native_lib):
    """mosfhet_hip_leveled_lut_packed_plan -- the function the launcher decides with -- over both rings, l in {1, 3, 6}, every (size, pack_log) inside the bound,
    1, 3 and 64 tables, small and large batches and a device of 256 and of 64 CUs: levels = max(0, size - (log2 N - p)), nodes = 2^(levels - 1), steps =
    min(size, log2 N - p), outputs = tables 2^p; the workspace arithmetic of the several-table plan at those nodes, chunk and pass maximal within the bound; pack_log
    = 0 gives exactly leveled_lut_tables_plan's six fields; nothing depends on the CU count; a lowered bound gives more passes or chunks, never a larger workspace.
    The bits plan prepends lut_bits_plan's four fields."""
    from mosfhet_amd import engine
    GiB = 1 << 30
    six = ("levels", "nodes", "chunk", "tables_per_pass", "workspace_bytes", "group")

    def check(N, l, size, tables, p_log, count, cus, bound):
        p = engine.leveled_lut_packed_plan(N, l, size, tables, p_log, count, cus)
        what = (cus, N, l, size, tables, p_log, count, bound, p)
        log_N = N.bit_length() - 1
        levels = max(0, size - (log_N - p_log))
        assert p["levels"] == levels and p["nodes"] == ((1 << (levels - 1)) if levels else 0), what
        assert p["steps"] == min(size, log_N - p_log) >= 1 and p["outputs"] == tables << p_log, what
        tp, chunk = p["tables_per_pass"], p["chunk"]
        assert 1 <= tp <= tables and 1 <= chunk <= count, what
        table, per_input = p["nodes"] * 2 * l * (N // 2) * 16, p["nodes"] * 2 * N * 8
        assert p["workspace_bytes"] == (tp * (table + chunk * per_input) if levels else 0) <= bound, what
        if levels:
            assert tp == tables or (tp + 1) * (table + chunk * per_input) > bound, what
            assert chunk == count or tp * (table + (chunk + 1) * per_input) > bound, what
        else:
            assert tp == tables and chunk == count, what
        assert 1 <= p["group"] <= tp, what
        assert p == engine.leveled_lut_packed_plan(N, l, size, tables, p_log, count, 256), what     # the CU count sizes grids only
        if p_log == 0:
            assert {k: p[k] for k in six} == engine.leveled_lut_tables_plan(N, l, size, tables, count, cus), what
        return p

    n = 0
    for cus in (256, 64):
        for N in (1024, 2048):
            log_N = N.bit_length() - 1
            for l in (1, 3, 6):
                for p_log in range(0, log_N):
                    for size in range(1, log_N + engine.LEVELED_LUT_MAX_LEVELS - p_log + 1):
                        for tables in (1, 3, 64):
                            for count in (1, 257, 4096):
                                check(N, l, size, tables, p_log, count, cus, GiB)
                                n += 1
                    with pytest.raises(engine.MosfhetHipError, match="pack_log = %d" % p_log):
                        engine.leveled_lut_packed_plan(N, l, log_N + engine.LEVELED_LUT_MAX_LEVELS - p_log + 1, 1, p_log, 1, cus)
    print("%d plans checked" % n)
    # P4's shape: 3 levels, 4 first-level nodes, 3 tables, 5 inputs
    try:
        table, per_input = 4 * 4 * 512 * 16, 4 * 2 * 1024 * 8
        p0 = engine.leveled_lut_packed_plan(1024, 2, 12, 3, 1, 5)
        assert p0 == dict(levels=3, nodes=4, chunk=5, tables_per_pass=3, workspace_bytes=3 * (table + 5 * per_input), group=p0["group"], steps=9, outputs=6)
        for bound in (3 * (table + 5 * per_input), 3 * (table + 5 * per_input) - 1, 3 * (table + 2 * per_input), 2 * (table + per_input), table + 2 * per_input,
                      table + per_input):
            engine.set_leveled_lut_workspace(bound)
            p = check(1024, 2, 12, 3, 1, 5, 256, bound)
            passes, chunks = -(-3 // p["tables_per_pass"]), -(-5 // p["chunk"])
            assert (passes > 1 or chunks > 1) == (bound < p0["workspace_bytes"]) and p["workspace_bytes"] <= p0["workspace_bytes"], (bound, p)
        assert (p["tables_per_pass"], p["chunk"]) == (1, 1)
        engine.set_leveled_lut_workspace(table + per_input - 1)                 # not even one table with one input: refused, not overrun
        with pytest.raises(engine.MosfhetHipError, match="workspace bound"):
            engine.leveled_lut_packed_plan(1024, 2, 12, 3, 1, 5)
        assert engine.leveled_lut_packed_plan(1024, 2, 9, 3, 1, 5)["workspace_bytes"] == 0      # no tree, no workspace
    finally:
        engine.set_leveled_lut_workspace(0)
    assert engine.leveled_lut_packed_plan(1024, 2, 12, 3, 1, 5) == p0
    # the bits plan: lut_bits_plan's four fields (the selector workspace is `size` selectors per input, whatever the packing), then the packed plan of a chunk
    for (N, l, size, tables, p_log, count) in ((2048, 4, 8, 1, 3, 1024), (2048, 4, 7, 1, 3, 3), (1024, 3, 12, 3, 1, 4096), (2048, 4, 8, 8, 0, 128)):
        b = engine.lut_bits_packed_plan(N, l, size, tables, p_log, count)
        u = engine.lut_bits_plan(N, l, size, 1, count)
        assert (b["chunk"], b["chunks"], b["selector_bytes"], b["cb_bits"]) == (u["chunk"], u["chunks"], u["selector_bytes"], u["cb_bits"]), (b, u)
        assert b["lut"] == engine.leveled_lut_packed_plan(N, l, size, tables, p_log, b["chunk"]), b
        assert b == engine.lut_bits_packed_plan(N, l, size, tables, p_log, count, 64)
    try:
        engine.set_lut_bits_workspace(2 * 8 * 2 * 4 * 2 * 2048 * 8 + 5)
        b = engine.lut_bits_packed_plan(2048, 4, 8, 1, 3, 5)
        assert (b["chunk"], b["chunks"], b["cb_bits"], b["lut"]["chunk"], b["lut"]["outputs"]) == (2, 3, 16, 2, 8), b
    finally:
        engine.set_lut_bits_workspace(0)


@pytest.mark.parametrize("name", list(PSETS))
def test_oracle_packed_composition_decrypts(oracle, name):
    """The condition on the inputs, proven on the CPU: the oracle composition alone decrypts every (input, table, t) of every set to LUT_tb[m x + t] within
    2^(64 - prec - 1); the inputs hold index 2^size - 1 and index 0."""
    T = _pcase(oracle, name)
    assert T["m"][0] == (1 << T["size"]) - 1 and T["m"][1] == 0
    worst = _worst_distance(oracle, T, T["want"])
    bound = 64 - T["prec"] - 1
    print("set %s: worst log2 torus_dist(phase, LUT_tb[m x + t]) = %.1f, bound %d, margin %.1f bits" % (name, np.log2(max(worst, 1.0)), bound,
                                                                                                       bound - np.log2(max(worst, 1.0))))
    assert worst < 2.0 ** bound, (name, np.log2(max(worst, 1.0)))


def test_packed_kernels_of_the_build(native_lib):
    """The packed call is new device code inside the kernels that exist: lut_tables_finish_kernel still once per ring, VGPR <= 256 and no scratch, fewer than 330
    kernels in all (329), and tools/check_lds_barriers.py as it stands finds nothing in any of its forms."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    import kernel_table
    assert sum(1 for f in chk.FORMS if "leveled LUT" in f[0]) >= 2, [f[0] for f in chk.FORMS]
    assert chk.build_and_check() == []        # the tool as it stands, every form
    rows = kernel_table.table()
    mine = sorted((r for r in rows if r["name"].startswith("lut_tables_finish_kernel")), key=lambda r: r["name"])
    assert [r["name"].replace("> >", ">>") for r in mine] == ["lut_tables_finish_kernel<Fft1024>", "lut_tables_finish_kernel<Fft2048T<false, false>>"], mine
    for r in mine:
        print("%-50s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
        assert r["vgpr"] <= 256 and r["scratch"] == 0, r
    print("%d kernels in the library" % len(rows))
    assert len(rows) == 329, len(rows)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _assert_all(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    _assert_words(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), what)


def _run(eng, T, sel=None, d_luts=None):
    import mosfhet_amd as ma
    sel = _sel_dft(eng, T["sel"]) if sel is None else sel
    d_luts = ma.to_device(T["tabs"], eng.device) if d_luts is None else d_luts
    return ma.to_numpy(eng.leveled_lut_packed(sel, d_luts, T["size"], T["l"], T["Bg"], T["p"]))


@pytest.mark.gpu
@pytest.mark.parametrize("group", [0, 64], ids=["default group", "largest group"])
@pytest.mark.parametrize("name", list(PSETS))
def test_packed_matches_the_oracle(eng, oracle, name, group):
    """P1 - P7 at the default grouping of the finish and at the largest the LDS holds: all count x tables x m x (N + 1) words equal the oracle's, every output
    decrypts to LUT_tb[m x + t], and the tables on the device are unchanged afterwards."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    T = _pcase(oracle, name)
    d_luts = ma.to_device(T["tabs"], eng.device)
    try:
        engine.set_leveled_lut_tables_group(group)
        got = _run(eng, T, d_luts=d_luts)
    finally:
        engine.set_leveled_lut_tables_group(0)
    assert got.shape == (T["inputs"], T["tables"], 1 << T["p"], T["N"] + 1)
    _assert_all(got, T["want"], "set %s, group %d" % (name, group))
    assert _worst_distance(oracle, T, got) < 2.0 ** (64 - T["prec"] - 1), "set %s: an output does not decrypt" % name
    assert (ma.to_numpy(d_luts) == T["tabs"]).all(), "the tables were modified"


@pytest.mark.gpu
def test_pack_log_0_is_the_several_table_call(eng, oracle):
    """P5 (pack_log = 0) equals leveled_lut_tables word for word, and one table of it through the packed call equals leveled_lut."""
    import mosfhet_amd as ma
    T = _pcase(oracle, "P5")
    sel = _sel_dft(eng, T["sel"])
    d_luts = ma.to_device(T["tabs"], eng.device)
    got = _run(eng, T, sel, d_luts)
    several = ma.to_numpy(eng.leveled_lut_tables(sel, d_luts, T["size"], T["l"], T["Bg"]))
    assert got.shape == (T["inputs"], T["tables"], 1, T["N"] + 1) and (got[:, :, 0] == several).all(), "pack_log = 0 differs from leveled_lut_tables"
    for tb in range(T["tables"]):
        alone = ma.to_numpy(eng.leveled_lut_packed(sel, d_luts[tb:tb + 1], T["size"], T["l"], T["Bg"], 0))
        one = ma.to_numpy(eng.leveled_lut(sel, d_luts[tb], T["size"], T["l"], T["Bg"]))
        assert (alone[:, 0, 0] == one).all(), "pack_log = 0, tables = 1 on table %d differs from leveled_lut" % tb


@pytest.mark.gpu
def test_packed_words_do_not_depend_on_the_shape(eng, oracle):
    """P4 (3 tree levels, 3 tables, 2 outputs per entry) at count 5 in one call, as 2 + 3, with the workspace bound lowered so that a pass holds one table and a chunk
    one or two inputs, and at 1, 2 and 64 tables per finishing workgroup: always the oracle's words."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    T = _pcase(oracle, "P4")
    N, l, size, p, tables = T["N"], T["l"], T["size"], T["p"], T["tables"]
    sel = _sel_dft(eng, T["sel"])
    d_luts = ma.to_device(T["tabs"], eng.device)
    _assert_all(_run(eng, T, sel, d_luts), T["want"], "P4, 5 inputs in one call")
    split = np.concatenate([_run(eng, T, sel[:2].contiguous(), d_luts), _run(eng, T, sel[2:].contiguous(), d_luts)])
    _assert_all(split, T["want"], "P4 as 2 + 3 inputs")
    q = eng.leveled_lut_packed_plan(N, l, size, tables, p, 5)
    table, per_input = q["nodes"] * 2 * l * (N // 2) * 16, q["nodes"] * 2 * N * 8
    assert (q["levels"], q["tables_per_pass"], q["chunk"]) == (3, 3, 5), q
    try:
        for bound, chunk in ((table + per_input, 1), (table + 2 * per_input, 2)):
            engine.set_leveled_lut_workspace(bound)
            q = eng.leveled_lut_packed_plan(N, l, size, tables, p, 5)
            assert (q["tables_per_pass"], q["chunk"]) == (1, chunk), q
            _assert_all(_run(eng, T, sel, d_luts), T["want"], "P4 in passes of one table and chunks of %d" % chunk)
        engine.set_leveled_lut_workspace(0)
        for group in (1, 2, 64):
            engine.set_leveled_lut_tables_group(group)
            assert eng.leveled_lut_packed_plan(N, l, size, tables, p, 5)["group"] == min(group, tables)
            _assert_all(_run(eng, T, sel, d_luts), T["want"], "P4 at group %d" % group)
    finally:
        engine.set_leveled_lut_workspace(0)
        engine.set_leveled_lut_tables_group(0)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reference", "by_component"])
def test_lut_bits_packed_is_the_three_calls(eng, oracle, order):
    """The key fixtures of tests/test_lut_bits.py's chunk-independence test (lvl2's ring and gadget, the cheap private and packing keys) at both set product orders:
    3 inputs x 4 bits, one table of 4 outputs per entry (tables * m == size): lut_bits_packed in chunks of 1, 2 + 1 and 3 inputs equals circuit_bootstrap_3_dft,
    leveled_lut_packed and tlwe_keyswitch on the whole batch, with and without the output key; the output is the next call's input."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    from test_gpu_parity import _keyset, _ksk_for
    K = _keyset("lvl2", eng, oracle)
    P = K["P"]
    N, l, Bg, n = P["N"], P["l"], P["Bg_bit"], P["n"]
    size, p, tables, count = 4, 2, 1, 3
    r = oracle.Rng(0xC105E)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"]), 2)
    ksk, _ = _ksk_for(K, eng)
    dksk = eng.load_keyswitch_key(ksk, P["base_bit"])
    key = eng.load_bootstrap_key(K["bk"], 1, l, Bg)
    key.set_product_order(order)
    rng = np.random.default_rng(0xC4A3)
    cts = rng.integers(0, 2 ** 64, size=(count, size, n + 1), dtype=np.uint64)
    tabs = rng.integers(0, 2 ** 64, size=(tables, 1, 2, N), dtype=np.uint64)                   # encrypted-looking table: every word takes part
    d_cts, d_luts = ma.to_device(cts, eng.device), ma.to_device(tabs, eng.device)
    sel = eng.circuit_bootstrap_3_dft(key, kska, pk, d_cts.view(count * size, n + 1)).reshape(count, size, 2 * l, 2, N)
    lut = eng.leveled_lut_packed(sel, d_luts, size, l, Bg, p)
    want_plain = ma.to_numpy(lut).reshape(count, tables << p, N + 1)
    want = ma.to_numpy(eng.tlwe_keyswitch(dksk, lut.view(count * (tables << p), N + 1))).reshape(count, tables << p, n + 1)
    per_input = size * 2 * l * 2 * N * 8
    try:
        for bound, chunk in ((per_input, 1), (2 * per_input + 5, 2), (0, 3)):
            engine.set_lut_bits_workspace(bound)
            q = eng.lut_bits_packed_plan(N, l, size, tables, p, count)
            assert (q["chunk"], q["chunks"], q["cb_bits"], q["lut"]["outputs"]) == (chunk, -(-count // chunk), chunk * size, size), (bound, q)
            got = eng.lut_bits_packed(key, kska, pk, d_luts, d_cts, p, ksk_out=dksk)
            assert tuple(got.shape) == tuple(d_cts.shape)
            assert (ma.to_numpy(got) == want).all(), "%s, %d inputs per chunk: differs from the three calls on the whole batch" % (order, chunk)
            plain = ma.to_numpy(eng.lut_bits_packed(key, kska, pk, d_luts, d_cts, p))
            assert (plain == want_plain).all(), "%s, %d inputs per chunk, no output key: differs from the two calls on the whole batch" % (order, chunk)
    finally:
        engine.set_lut_bits_workspace(0)
    assert (ma.to_numpy(d_luts) == tabs).all(), "the table was modified"
    for h in (kska, pk, dksk, key):
        h.free()


@pytest.mark.gpu
def test_lut_bits_packed_round_decrypts(eng, oracle):
    """One round at BASELINE.json configs[3]'s real keys (tests/test_lut_bits.py::_real_keys), 7 bits in, 8 bits out.  The condition, established with the call that
    existed before: lut_bits with the function as 8 one-bit tables decrypts every output bit within 2^61, half the message spacing of 1/4 that the circuit bootstrap
    takes (test_lut_bits_two_rounds_decrypt's bound); at most one input that misses it is dropped.  Then lut_bits_packed with the same function as ONE table of 8
    outputs per entry (pack_log 3: 1024 coefficients, shorter than N) decrypts every kept bit to the same value."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import host
    import test_lut_bits as TLB
    free, _ = torch.cuda.mem_get_info(eng.device)
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory (3 GB packing key), %.1f GiB free" % (free / 2 ** 30))
    had = "real" in TLB._CACHE
    R = TLB._real_keys(eng)
    try:
        P, key, kska, pk, dksk = R["P"], R["key"], R["kska"], R["pk"], R["dksk"]
        N, n, size, p, outs, count = P["N"], P["n"], 7, 3, 8, 3
        rng = np.random.default_rng(0x9AC)
        f = rng.integers(0, 2, size=(1 << size, outs), dtype=np.uint64)             # f(x) bit t = f[x][t]
        unpacked = np.zeros((outs, 1, 2, N), dtype=np.uint64)
        unpacked[:, 0, 1, :1 << size] = f.T << np.uint64(62)
        packed = np.zeros((1, 1, 2, N), dtype=np.uint64)
        packed[0, 0, 1, :outs << size] = f.reshape(-1) << np.uint64(62)             # output t of entry x at coefficient 8 x + t
        m = [(1 << size) - 1, 0, int(rng.integers(0, 1 << size))]
        host.seed(0x9AC)
        cts = host.tlwe_samples([host.double2torus(0.25 * ((m[b] >> i) & 1)) for b in range(count) for i in range(size)], R["lk"])
        d_in = ma.to_device(cts, eng.device).view(count, size, n + 1)
        lwe_s = np.ascontiguousarray(R["lk"].s, dtype=np.uint64)

        def distances(out):
            return np.array([[float(oracle.torus_dist(oracle.tlwe_phase(out[b, t], lwe_s), int(f[m[b]][t]) << 62)) for t in range(outs)] for b in range(count)])

        d_old = distances(ma.to_numpy(eng.lut_bits(key, kska, pk, ma.to_device(unpacked, eng.device), d_in, ksk_out=dksk)))
        print("lut_bits, 8 one-bit tables: worst log2 torus distance per input %s (bound 61)" % np.round(np.log2(np.maximum(d_old.max(axis=1), 1.0)), 1))
        kept = [b for b in range(count) if d_old[b].max() < 2.0 ** 61]
        assert len(kept) >= count - 1, "the inputs are unfit: the unpacked call itself misses the bound on %d of %d inputs" % (count - len(kept), count)
        got = eng.lut_bits_packed(key, kska, pk, ma.to_device(packed, eng.device), d_in, p, ksk_out=dksk)
        assert tuple(got.shape) == (count, outs, n + 1)
        d_new = distances(ma.to_numpy(got))
        print("lut_bits_packed, one table, pack_log 3: worst log2 torus distance per input %s" % np.round(np.log2(np.maximum(d_new.max(axis=1), 1.0)), 1))
        for b in kept:
            assert d_new[b].max() < 2.0 ** 61, "input %d: a bit of the packed call is 2^%.1f from f(m) (bound 2^61)" % (b, np.log2(d_new[b].max()))
    finally:
        if not had:      # the handles belong to this module's engine: the next module makes its own
            TLB._CACHE.pop("real", None)
            for h in (R["key"], R["kska"], R["pk"], R["dksk"]):
                h.free()


@pytest.mark.gpu
def test_eval_LUTs_packed_inputs_through_the_host_structs(native_lib, tmp_path):
    """tests/c/leveled_lut_packed.c: mosfhet_eval_LUTs_packed_inputs at P1's and P2's shapes through the host structs of include/mosfhet.h; every output decrypts to
    its table entry, equals the blind_rotate / trlwe_extract_tlwe loop written against the same header word for word, and the tables are left as they were."""
    exe = str(tmp_path / "leveled_lut_packed")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "leveled_lut_packed.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "leveled_lut_packed ok" in r.stdout, r.stdout[-3000:]
