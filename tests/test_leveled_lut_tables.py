"""Leveled look-up-table evaluation with SEVERAL shared tables over the same TRGSW-encrypted inputs (include/mosfhet_hip.h:
mosfhet_hip_leveled_lut_tables_batch; mosfhet_amd/csrc/leveled_lut_kernels.h: lut_tables_finish_kernel).

The expected words of (input b, table tb) are the oracle composition of tests/test_leveled_lut.py::_composition on table tb with sel_dft = oracle.bk_to_dft(sel[b], 1, l):
the same words mosfhet_hip_leveled_lut_batch gives for that table alone.  Every GPU comparison is == on all words; there is no tolerance anywhere.  The decryption
bound 2^(64 - prec - 1) is a condition on the INPUTS that the oracle composition alone meets on the CPU (test_oracle_composition_decrypts_every_table).

The parameter sets are those of test_leveled_lut.py (same N, l, Bg, sigma, size, selectors and key); each gets 8 tables of that set's precision (13 for set A's
shape test), trivial or encrypted as the set says.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_leveled_lut import SETS, _assert_words, _case, _composition, _map, _sel_dft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SETS = ["A", "A'", "C", "D", "E", "G"]
XCH_SLOTS = {1024: 576, 2048: 1152}        # negacyclic_fft.h: complex slots of one team's exchange buffer
_CACHE = {}


def _tcase(oracle, name, tables=8, inputs=None):
    """test_leveled_lut's case `name` (key, indices, selectors) with `tables` fresh tables and the oracle's outputs want[b][tb] for the first `inputs` inputs"""
    N, l, Bg, sigma, size, prec, n_inputs, encrypted, seed = SETS[name]
    oracle.plan(N)       # made here, by one thread: oracle.plan() is not safe to call first from the workers of _map (two plans, one freed while the other thread uses it)
    S = _case(oracle, name)
    inputs = n_inputs if inputs is None else inputs
    if (name, tables, inputs) in _CACHE:
        return _CACHE[(name, tables, inputs)]
    log_N = N.bit_length() - 1
    r = oracle.Rng(seed + 0x7AB)
    n_luts = max(1, (1 << size) >> log_N)
    lut = (oracle.u64(r.words(tables << max(size, log_N))) % np.uint64(1 << prec)).astype(np.uint64).reshape(tables, -1)
    msg = (lut << np.uint64(64 - prec)).reshape(tables, n_luts, N)
    tabs = np.zeros((tables, n_luts, 2, N), dtype=np.uint64)
    if encrypted:
        for tb in range(tables):
            for j in range(n_luts):
                tabs[tb, j] = oracle.trlwe_sample(r, msg[tb, j].copy(), S["s"], sigma)
    else:
        tabs[:, :, 1, :] = msg
    sel_dft = _map(lambda b: oracle.bk_to_dft(S["sel"][b], 1, l), range(inputs))
    want = np.stack(_map(lambda u: _composition(oracle, tabs[u % tables], sel_dft[u // tables], N, l, Bg, size), range(inputs * tables)))
    T = dict(S, lut=lut, tabs=tabs, want=want.reshape(inputs, tables, N + 1), tables=tables, inputs=inputs)
    _CACHE[(name, tables, inputs)] = T
    return T


def _worst_distance(oracle, T, outs):
    """largest torus distance of an output's phase from LUT_tb[m_b], over all (input, table)"""
    worst = 0.0
    for b in range(T["inputs"]):
        for tb in range(T["tables"]):
            d = float(oracle.torus_dist(oracle.tlwe_phase(outs[b, tb], T["s"][0]), int(T["lut"][tb][T["m"][b]]) << (64 - T["prec"])))
            worst = max(worst, d)
    return worst


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_tables_symbols_and_argument_checks(native_lib):
    """The library exports the new entry points, and mosfhet_hip_leveled_lut_tables_batch refuses tables = 0 and 65 and every bad argument of the one-table call
    with MOSFHET_HIP_EINVAL and a message naming the argument -- on fake pointers, before any HIP call (this runs without a GPU)."""
    from mosfhet_amd import engine
    for name in ("mosfhet_hip_leveled_lut_tables_batch", "mosfhet_hip_leveled_lut_tables_plan", "mosfhet_eval_LUTs_inputs"):
        assert hasattr(native_lib, name), name
    assert engine.LEVELED_LUT_MAX_TABLES == 64
    f = native_lib.mosfhet_hip_leveled_lut_tables_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    err = lambda: native_lib.mosfhet_hip_last_error().decode()
    fake = C.c_void_p(8)     # never dereferenced: every call below fails on its arguments
    bound = 10 + engine.LEVELED_LUT_MAX_LEVELS
    assert f(fake, fake, fake, fake, 13, 1024, 3, 10, 0, 4, None) == -1 and "tables = 0" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 3, 10, 65, 4, None) == -1 and "tables = 65" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 3, 10, -1, 4, None) == -1 and "tables = -1" in err()
    assert f(None, fake, fake, fake, 13, 1024, 3, 10, 8, 4, None) == -1 and "ctx" in err()
    assert f(fake, fake, fake, fake, 0, 1024, 3, 10, 8, 4, None) == -1 and "size = 0" in err()
    assert f(fake, fake, fake, fake, bound + 1, 1024, 3, 10, 8, 4, None) == -1 and "size = %d" % (bound + 1) in err()
    assert f(fake, fake, fake, fake, bound + 2, 2048, 3, 10, 8, 4, None) == -1 and "size = %d" % (bound + 2) in err()
    assert f(fake, fake, fake, fake, 13, 512, 3, 10, 8, 4, None) == -1 and "N = 512" in err()
    assert f(fake, fake, fake, fake, 13, 4096, 3, 10, 8, 4, None) == -1 and "N = 4096" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 4, 16, 8, 4, None) == -1 and "l=4 Bg_bit=16" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 7, 8, 8, 4, None) == -1 and "l = 7" in err()
    assert f(fake, fake, fake, fake, 13, 1024, 3, 10, 8, -1, None) == -1 and "count = -1" in err()
    assert f(fake, fake, fake, fake, 0, 1024, 3, 10, 8, 0, None) == -1 and "size = 0" in err()      # count = 0 still checks the rest ...
    plan = (C.c_longlong * 6)()
    g = native_lib.mosfhet_hip_leveled_lut_tables_plan
    assert g(1024, 3, 13, 8, 4, 256, None) == -1
    assert g(4096, 1, 13, 8, 4, 256, plan) == -1 and "N = 4096" in err()
    assert g(1024, 3, 13, 0, 4, 256, plan) == -1 and "tables = 0" in err()
    assert g(1024, 3, 13, 65, 4, 256, plan) == -1 and "tables = 65" in err()
    assert g(1024, 3, 13, 8, 0, 256, plan) == -1 and "count = 0" in err()
    assert g(1024, 3, 13, 8, 4, 0, plan) == -1 and "cus = 0" in err()
    assert native_lib.mosfhet_hip_set_leveled_lut_tables_group(-1) == -1 and "group = -1" in err()
    assert native_lib.mosfhet_hip_set_leveled_lut_tables_group(65) == -1 and "group = 65" in err()


def test_tables_plan_sweep(native_lib):
    """mosfhet_hip_leveled_lut_tables_plan -- the function the launcher decides with -- over both rings, l in {1, 3, 6}, every size up to the bound, 1 .. 64 tables,
    small and large batches and a device of 256 and of 64 CUs: levels and nodes of the one-table plan, passes x tables per pass cover the tables, chunks cover the
    inputs, workspace = tables per pass x (prepared rows + chunk x intermediates) within the bound, a pass and a chunk as large as the bound allows, nothing
    depends on the CU count, one table reproduces the one-table plan; a lower bound gives more passes or chunks and never a larger workspace."""
    from mosfhet_amd import engine
    GiB = 1 << 30

    def check(N, l, size, tables, count, cus, bound):
        p = engine.leveled_lut_tables_plan(N, l, size, tables, count, cus)
        what = (cus, N, l, size, tables, count, bound, p)
        log_N = N.bit_length() - 1
        one = engine.leveled_lut_plan(N, l, size, count, cus)
        assert p["levels"] == one["levels"] == max(0, size - log_N) and p["nodes"] == one["nodes"], what
        tp, chunk = p["tables_per_pass"], p["chunk"]
        assert 1 <= tp <= tables and 1 <= chunk <= count, what
        assert tp * -(-tables // tp) >= tables and chunk * -(-count // chunk) >= count, what
        table, per_input = p["nodes"] * 2 * l * (N // 2) * 16, p["nodes"] * 2 * N * 8
        assert p["workspace_bytes"] == (tp * (table + chunk * per_input) if p["levels"] else 0), what
        assert p["workspace_bytes"] <= bound, what
        if p["levels"]:
            # as large as the bound allows: all tables, or one more table per pass would not fit; the whole batch, or one more input per chunk would not fit
            assert tp == tables or (tp + 1) * (table + chunk * per_input) > bound, what
            assert chunk == count or tp * (table + (chunk + 1) * per_input) > bound, what
        else:
            assert tp == tables and chunk == count, what
        assert 1 <= p["group"] <= tp, what
        assert XCH_SLOTS[N] * 2 * 16 + p["group"] * 2 * N * 8 <= 160 * 1024, what
        assert p == engine.leveled_lut_tables_plan(N, l, size, tables, count, 256), what     # the CU count sizes grids only
        if tables == 1:
            assert (p["levels"], p["nodes"], p["chunk"], p["workspace_bytes"]) == (one["levels"], one["nodes"], one["chunk"], one["workspace_bytes"]), what
        return p

    for cus in (256, 64):
        for N in (1024, 2048):
            log_N = N.bit_length() - 1
            for l in (1, 3, 6):
                for size in range(1, log_N + engine.LEVELED_LUT_MAX_LEVELS + 1):
                    for tables in (1, 2, 8, 64):
                        for count in (1, 3, 257, 4096):
                            check(N, l, size, tables, count, cus, GiB)
    try:
        per_input, table = 32 * 2 * 1024 * 8, 32 * 6 * 512 * 16
        p0 = engine.leveled_lut_tables_plan(1024, 3, 16, 8, 5)
        assert p0 == dict(levels=6, nodes=32, chunk=5, tables_per_pass=8, workspace_bytes=8 * (table + 5 * per_input), group=p0["group"])
        for bound in (8 * (table + 5 * per_input), 8 * (table + 5 * per_input) - 1, 8 * (table + 2 * per_input), 8 * (table + per_input), 8 * (table + per_input) - 1,
                      3 * (table + 2 * per_input), 2 * (table + per_input), table + per_input):
            engine.set_leveled_lut_workspace(bound)
            p = check(1024, 3, 16, 8, 5, 256, bound)
            passes, chunks = -(-8 // p["tables_per_pass"]), -(-5 // p["chunk"])
            # lowered below what the whole call takes: more passes or chunks than the one of each at the default, never a larger workspace
            assert (passes > 1 or chunks > 1) == (bound < p0["workspace_bytes"]) and p["workspace_bytes"] <= p0["workspace_bytes"], (bound, p)
        assert (p["tables_per_pass"], p["chunk"]) == (1, 1)
        engine.set_leveled_lut_workspace(3 * (table + 2 * per_input))
        p = engine.leveled_lut_tables_plan(1024, 3, 16, 8, 5)
        assert (p["tables_per_pass"], p["chunk"]) == (3, 2), p                                       # several passes AND several chunks
        engine.set_leveled_lut_workspace(table + per_input - 1)                                      # not even one table with one input: refused, not overrun
        with pytest.raises(engine.MosfhetHipError, match="workspace bound"):
            engine.leveled_lut_tables_plan(1024, 3, 16, 8, 5)
        assert engine.leveled_lut_tables_plan(1024, 3, 10, 8, 5)["workspace_bytes"] == 0             # no tree, no workspace
    finally:
        engine.set_leveled_lut_workspace(0)
    assert engine.leveled_lut_tables_plan(1024, 3, 16, 8, 5) == p0
    # the tables per finishing workgroup: what was asked for, capped by the LDS of a CU (8 at N = 1024, 3 at N = 2048) and by the tables of a pass
    try:
        engine.set_leveled_lut_tables_group(64)
        assert engine.leveled_lut_tables_plan(1024, 3, 13, 13, 5)["group"] == 8
        assert engine.leveled_lut_tables_plan(2048, 4, 12, 13, 5)["group"] == 3
        assert engine.leveled_lut_tables_plan(1024, 3, 13, 2, 5)["group"] == 2
        engine.set_leveled_lut_tables_group(3)
        assert engine.leveled_lut_tables_plan(1024, 3, 13, 13, 5)["group"] == 3
    finally:
        engine.set_leveled_lut_tables_group(0)
    assert engine.leveled_lut_tables_plan(1024, 3, 16, 8, 5) == p0


def test_tables_kernels_of_the_build(native_lib):
    """The built library's kernel table holds the new finish once per ring -- VGPR <= 256, no scratch, its LDS at the largest group the plan ever gives within the
    160 KiB of a CU -- and fewer than 330 kernels in all; tools/check_lds_barriers.py lists the new form and finds nothing."""
    from mosfhet_amd import engine
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    import kernel_table
    forms = [f for f in chk.FORMS if "several tables" in f[0]]
    assert len(forms) == 1 and forms[0][2] == "leveled_lut_tables_ab.hip", [f[0] for f in chk.FORMS]
    assert chk.build_and_check(forms) == []
    rows = kernel_table.table()
    by_name = {r["name"].replace("> >", ">>"): r for r in rows}
    new = sorted(n for n in by_name if n.startswith("lut_tables_finish_kernel"))
    assert new == ["lut_tables_finish_kernel<Fft1024>", "lut_tables_finish_kernel<Fft2048T<false, false>>"], new
    assert sum(1 for r in rows if r["name"].startswith("lut_tables_finish_kernel")) == 2
    try:
        engine.set_leveled_lut_tables_group(64)
        for name, N in zip(new, (1024, 2048)):
            r = by_name[name]
            group = engine.leveled_lut_tables_plan(N, 3, 12, 64, 5)["group"]
            lds = r["lds"] + XCH_SLOTS[N] * 2 * 16 + group * 2 * N * 8
            print("%-50s vgpr %3d  agpr %3d  sgpr %3d  lds %6d static, %6d at %d tables per workgroup  scratch %4d" % (name, r["vgpr"], r["agpr"], r["sgpr"], r["lds"], lds, group,
                                                                                                                      r["scratch"]))
            assert r["vgpr"] <= 256 and r["scratch"] == 0 and lds <= 160 * 1024 and r["lds"] % 16 == 0, r
    finally:
        engine.set_leveled_lut_tables_group(0)
    print("%d kernels in the library" % len(rows))
    assert len(rows) < 330, len(rows)


@pytest.mark.parametrize("name", NEW_SETS)
def test_oracle_composition_decrypts_every_table(oracle, name):
    """The condition on the inputs, proven on the CPU: the oracle composition alone decrypts every (input, table) of every new set to LUT_tb[m_b] within
    2^(64 - prec - 1)."""
    T = _tcase(oracle, name)
    worst = _worst_distance(oracle, T, T["want"])
    bound = 64 - T["prec"] - 1
    print("set %s, %d tables: worst log2 torus_dist(phase, LUT_tb[m]) = %.1f, bound %d, margin %.1f bits" % (name, T["tables"], np.log2(max(worst, 1.0)), bound,
                                                                                                           bound - np.log2(max(worst, 1.0))))
    assert worst < 2.0 ** bound, (name, np.log2(max(worst, 1.0)))


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


def _assert_all(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    flat_g, flat_w = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    _assert_words(flat_g, flat_w, what)


@pytest.mark.gpu
@pytest.mark.parametrize("group", [0, 64], ids=["default group", "largest group"])
@pytest.mark.parametrize("name", NEW_SETS)
def test_tables_match_the_oracle(eng, oracle, name, group):
    """8 tables on 5 inputs (33 for A and A') of six parameter sets, at the default grouping of the finish and at the largest the LDS holds: all
    count x tables x (N + 1) words equal the oracle's, every output decrypts to LUT_tb[m_b], and the tables on the device are unchanged afterwards."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    T = _tcase(oracle, name)
    d_luts = ma.to_device(T["tabs"], eng.device)
    try:
        engine.set_leveled_lut_tables_group(group)
        got = ma.to_numpy(eng.leveled_lut_tables(_sel_dft(eng, T["sel"]), d_luts, T["size"], T["l"], T["Bg"]))
    finally:
        engine.set_leveled_lut_tables_group(0)
    assert got.shape == (T["inputs"], 8, T["N"] + 1)
    _assert_all(got, T["want"], "set %s, 8 tables" % name)
    assert _worst_distance(oracle, T, got) < 2.0 ** (64 - T["prec"] - 1), "set %s: an output does not decrypt" % name
    assert (ma.to_numpy(d_luts) == T["tabs"]).all(), "the tables were modified"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_tables_equal_the_one_table_call(eng, oracle, name):
    """leveled_lut_tables(...)[:, tb] is leveled_lut(..., luts[tb]) for every table, and one table through the new call is the one-table call."""
    import mosfhet_amd as ma
    T = _tcase(oracle, name)
    sel = _sel_dft(eng, T["sel"])
    d_luts = ma.to_device(T["tabs"], eng.device)
    got = ma.to_numpy(eng.leveled_lut_tables(sel, d_luts, T["size"], T["l"], T["Bg"]))
    for tb in range(T["tables"]):
        one = ma.to_numpy(eng.leveled_lut(sel, d_luts[tb], T["size"], T["l"], T["Bg"]))
        assert (got[:, tb] == one).all(), "set %s: table %d of the several-table call differs from the one-table call" % (name, tb)
        alone = ma.to_numpy(eng.leveled_lut_tables(sel, d_luts[tb:tb + 1], T["size"], T["l"], T["Bg"]))
        assert alone.shape == (T["inputs"], 1, T["N"] + 1) and (alone[:, 0] == one).all(), "set %s: tables = 1 on table %d differs from the one-table call" % (name, tb)


@pytest.mark.gpu
def test_tables_words_do_not_depend_on_the_shape(eng, oracle):
    """Set A with 1, 3, 8 and 13 tables at batch sizes 1, 3, CUs + 1 and 1024, tiled from 16 distinct inputs (the selectors are tiled on the device): the outputs are
    the expected rows tiled.  13 tables also in groups of 3 per finishing workgroup, so that a tail group of one table runs, and in groups of 8 (tail of 5).  Set G
    with the workspace bound lowered so that 8 tables take three passes AND 5 inputs take three chunks."""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    T = _tcase(oracle, "A", tables=13, inputs=16)
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    sel16 = _sel_dft(eng, T["sel"][:16])
    d_luts = ma.to_device(T["tabs"], eng.device)
    for B in (1, 3, cus + 1, 1024):
        idx = np.arange(B) % 16
        sel = sel16[torch.from_numpy(idx).to(eng.device)].contiguous()
        for tables, group in ((1, 0), (3, 0), (8, 0), (13, 0), (13, 3), (13, 8)):
            try:
                engine.set_leveled_lut_tables_group(group)
                if group:
                    assert eng.leveled_lut_tables_plan(T["N"], T["l"], T["size"], tables, B)["group"] == group
                got = ma.to_numpy(eng.leveled_lut_tables(sel, d_luts[:tables].contiguous(), T["size"], T["l"], T["Bg"]))
            finally:
                engine.set_leveled_lut_tables_group(0)
            _assert_all(got, T["want"][idx][:, :tables], "%d inputs tiled from 16, %d tables, group %d" % (B, tables, group))
        del sel
    G = _tcase(oracle, "G")
    p = eng.leveled_lut_tables_plan(G["N"], G["l"], G["size"], 8, 5)
    table, per_input = p["nodes"] * 2 * G["l"] * (G["N"] // 2) * 16, p["nodes"] * 2 * G["N"] * 8
    assert (p["tables_per_pass"], p["chunk"]) == (8, 5)
    d_g = ma.to_device(G["tabs"], eng.device)
    sel_g = _sel_dft(eng, G["sel"])
    try:
        engine.set_leveled_lut_workspace(3 * (table + 2 * per_input))
        q = eng.leveled_lut_tables_plan(G["N"], G["l"], G["size"], 8, 5)
        assert (q["tables_per_pass"], q["chunk"]) == (3, 2), q
        for group in (0, 2):
            engine.set_leveled_lut_tables_group(group)
            got = ma.to_numpy(eng.leveled_lut_tables(sel_g, d_g, G["size"], G["l"], G["Bg"]))
            _assert_all(got, G["want"], "set G in passes of 3 tables and chunks of 2 inputs, group %d" % group)
    finally:
        engine.set_leveled_lut_workspace(0)
        engine.set_leveled_lut_tables_group(0)


@pytest.mark.gpu
def test_the_pipeline_closes(eng, oracle):
    """At lvl2's ring and gadget with the cheap key set of test_circuit_bootstrap_output_is_the_selector_layout (words are compared, nothing is decrypted):
    2 inputs x 8 LWE bits -> circuit_bootstrap_3 -> trgsw_to_dft -> leveled_lut_tables with 8 one-bit tables (size 8, no tree) -> tlwe_keyswitch N -> n on the
    [2 * 8][N + 1] view -> circuit_bootstrap_3 -> trgsw_to_dft -> leveled_lut_tables again.  Every stage against the oracle's routine for it; no repacking
    between stages: d_out[b][tb] IS bit tb of input b of the next round."""
    import mosfhet_amd as ma
    from test_gpu_parity import _keyset, _ksk_for
    K = _keyset("lvl2", eng, oracle)
    P = K["P"]
    N, l, Bg, size, count, tables = P["N"], P["l"], P["Bg_bit"], 8, 2, 8
    key, _ = eng.clone_key(K["bsk"])
    key.set_product_order("reference")
    r = oracle.Rng(0xC105E)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    lwe_s = np.ascontiguousarray(K["lk"].s, dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kskb = oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(kskb, 2)
    ks0_dft, ks1_dft = oracle.ks_to_dft(ks0), oracle.ks_to_dft(ks1)
    ksk, dksk = _ksk_for(K, eng)
    rng = np.random.default_rng(0xC105E)
    m = [int(rng.integers(0, 1 << size)) for _ in range(count)]
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(0.25 * ((m[b] >> i) & 1)), lwe_s, P["lwe_sigma"]) for b in range(count) for i in range(size)])
    tabs = np.zeros((tables, 1, 2, N), dtype=np.uint64)              # 8 one-bit tables: entry in {0, 1/4}, the message the circuit bootstrap takes
    tabs[:, 0, 1, :] = (oracle.u64(r.words(tables * N)) % np.uint64(2)).reshape(tables, N) << np.uint64(62)
    d_luts = ma.to_device(tabs, eng.device)

    def cb(c):
        return np.stack(_map(lambda u: oracle.circuit_bootstrap_3(c[u], K["bk_dft"], ks0_dft, ks1_dft, 2, kskb, 2, l, Bg), range(len(c)))).reshape(count, size, 2 * l, 2, N)

    def luts(sel):
        dft = [oracle.bk_to_dft(sel[b], 1, l) for b in range(count)]
        return np.stack(_map(lambda u: _composition(oracle, tabs[u % tables], dft[u // tables], N, l, Bg, size), range(count * tables))).reshape(count, tables, N + 1)

    want_sel1 = cb(cts)
    want_out1 = luts(want_sel1)
    want_ks = np.stack(_map(lambda u: oracle.tlwe_keyswitch(want_out1.reshape(count * tables, N + 1)[u], ksk, P["n"], P["t"], P["base_bit"]), range(count * tables)))
    want_sel2 = cb(want_ks)
    want_out2 = luts(want_sel2)

    trgsw1 = eng.circuit_bootstrap_3(key, kska, pk, ma.to_device(cts, eng.device))                    # [count * size][2l][2][N]
    assert (ma.to_numpy(trgsw1).reshape(want_sel1.shape) == want_sel1).all(), "first circuit_bootstrap_3 differs from the oracle"
    out1 = eng.leveled_lut_tables(eng.trgsw_to_dft(trgsw1).reshape(count, size, 2 * l, 2, N), d_luts, size, l, Bg)
    _assert_all(ma.to_numpy(out1), want_out1, "first leveled_lut_tables")
    switched = eng.tlwe_keyswitch(dksk, out1.view(count * tables, N + 1))                                # "bit tb of input b", no repacking
    assert (ma.to_numpy(switched) == want_ks).all(), "tlwe_keyswitch of the [count * tables][N + 1] view differs from the oracle"
    trgsw2 = eng.circuit_bootstrap_3(key, kska, pk, switched)
    assert (ma.to_numpy(trgsw2).reshape(want_sel2.shape) == want_sel2).all(), "second circuit_bootstrap_3 differs from the oracle"
    out2 = eng.leveled_lut_tables(eng.trgsw_to_dft(trgsw2).reshape(count, size, 2 * l, 2, N), d_luts, size, l, Bg)
    _assert_all(ma.to_numpy(out2), want_out2, "second leveled_lut_tables")
    for h in (kska, pk, key):
        h.free()


@pytest.mark.gpu
def test_eval_LUTs_inputs_through_the_host_structs(native_lib, tmp_path):
    """tests/c/leveled_lut_tables.c: mosfhet_eval_LUTs_inputs with 4 tables on 4 inputs at set B's parameters equals the reference's own eval_LUT loop written
    against include/mosfhet.h, per table on a copy of the table, word for word; outputs decrypt to the table entries; the tables are left as they were."""
    exe = str(tmp_path / "leveled_lut_tables")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "leveled_lut_tables.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "leveled_lut_tables ok" in r.stdout, r.stdout[-3000:]
