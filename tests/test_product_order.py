"""The summation order of a bootstrap key's external products as a property of the KEY (include/mosfhet_hip.h: mosfhet_hip_bsk_set_product_order).

AUTO (the default) lets the kernel chosen for the batch size decide: the two-CU split kernels sum per accumulator component, every other kernel in the
reference's one chain.  REFERENCE never takes a split kernel; BY_COMPONENT takes a by-component kernel at EVERY batch size (the split kernel while the batch is
small enough for two CUs each, its one-CU form beyond, the by-component form of the throughput kernel for large batches).  With either, the words of a result depend neither on the batch
size, nor on the split switches, nor on how a batch is sharded.  Both orders are restated by the oracle (oracle.product_order) and every comparison below is bit for bit.

This file has no autouse fixture: it starts at the library's defaults (split kernels on) and restores every setter it touches.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import SEED, _assert_all_outputs_equal, _keyset, _ksk_for, _oracle_map, _rand_u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GADGET_BITS = {1: 23, 2: 15, 3: 10, 4: 9, 5: 6, 6: 7}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _governed(N, l, galois):
    """the rule of the header: the families in which AUTO can pick a by-component kernel for some batch size"""
    return N == 2048 and (l == 4 if galois else l in (2, 4, 6))


def test_bootstrap_plan_sweep(native_lib):
    """mosfhet_hip_bootstrap_plan -- the function the launchers decide with -- over rings, gadget lengths, both families and the batch sizes around every threshold,
    for a device of 256 CUs and one of 64: REFERENCE never sums by component; BY_COMPONENT does at every count wherever the rule governs and nowhere else; AUTO
    exactly where a split kernel is taken (N = 2048, governed gadgets, count <= CUs / 2).  The split switch moves AUTO's bits and none of the others'."""
    from mosfhet_amd import engine
    for cus in (256, 64):
        counts = [1, cus // 2, cus // 2 + 1, cus, cus + 1, 512, 513, 4 * cus, 4 * cus + 1, 4096]
        for N in (1024, 2048, 4096):
            for l in range(1, 7):
                for galois in (False, True):
                    gov = _governed(N, l, galois)
                    for count in counts:
                        what = (cus, N, l, galois, count)
                        ref = engine.bootstrap_plan(N, l, GADGET_BITS[l], count, "reference", cus, galois=galois)
                        assert not ref["by_component"] and ref["family"] in ("throughput", "latency"), (what, ref)
                        byc = engine.bootstrap_plan(N, l, GADGET_BITS[l], count, "by_component", cus, galois=galois)
                        assert byc["by_component"] == gov, (what, byc)
                        auto = engine.bootstrap_plan(N, l, GADGET_BITS[l], count, "auto", cus, galois=galois)
                        assert auto["by_component"] == (gov and count <= cus // 2), (what, auto)
                        assert (auto["family"] == "split") == auto["by_component"], (what, auto)
                        if gov:
                            # two CUs per bootstrap is a matter of speed: the same batches as under AUTO; beyond, the one-CU form; past 512 the throughput form in the
                            # throughput kernel's residency rounds (4 teams per CU) -- the Galois family: the one-CU form in rounds of one workgroup per CU
                            want = "split" if count <= cus // 2 else ("latency_by_component" if count <= 512 else "throughput_by_component")
                            assert byc["family"] == want, (what, byc)
                            assert byc["rounds"] == (-(-count // (cus if galois else 4 * cus)) if want == "throughput_by_component" else 1), (what, byc)
                        else:
                            assert byc == ref == auto, (what, byc, ref, auto)
                        assert ref["family"] == ("latency" if count <= {1024: 512, 2048: 512, 4096: 0 if galois else 256}[N] else "throughput"), (what, ref)
    try:
        engine.set_split_max_batch(0)
        for count in (1, 100, 600, 4096):
            assert not engine.bootstrap_plan(2048, 4, 9, count, "auto")["by_component"]
            assert engine.bootstrap_plan(2048, 4, 9, count, "by_component")["by_component"]
            assert engine.bootstrap_plan(2048, 4, 9, count, "by_component")["family"] != "split"
        engine.set_split_max_batch(300)
        assert engine.bootstrap_plan(2048, 4, 9, 300, "reference")["family"] == "latency"
        assert engine.bootstrap_plan(2048, 4, 9, 300, "by_component")["family"] == "split"
    finally:
        engine.set_split_max_batch(-1)
    import ctypes as C
    plan = (C.c_int * 4)()
    assert native_lib.mosfhet_hip_bootstrap_plan(2048, 4, 9, 1, 1, 0, 3, 256, plan) == -1 and b"unknown product order" in native_lib.mosfhet_hip_last_error()
    assert native_lib.mosfhet_hip_bootstrap_plan(2048, 4, 9, 0, 1, 0, 0, 256, plan) == -1
    assert native_lib.mosfhet_hip_bsk_set_product_order(None, 1) == -1 and native_lib.mosfhet_hip_bsk_get_product_order(None, None) == -1


BY_COMPONENT_KERNELS = ["pbs_split_kernel<Fft2048T<false, true>, %s, true>" % g for g in ("4, 9", "6, 7", "2, 0", "4, 0", "6, 0")] + \
                       ["pbs_ga_split_kernel<Fft2048T<false, true>, %s, true>" % g for g in ("4, 9", "4, 0")] + \
                       ["pbs_kernel<Fft2048T<false, false>, %s, true>" % g for g in ("4, 9", "6, 7", "2, 0", "4, 0", "6, 0")]


def test_by_component_kernels_of_the_build(native_lib):
    """The built library's kernel table holds the by-component instantiations that a parameter set reaches -- the one-CU form and the throughput form at compile-time
    4 x 2^9 and 6 x 2^7 and the run-time gadgets l = 2, 4, 6 of the plain family, the one-CU form at 4 x 2^9 and run-time l = 4 of the Galois family -- and no others,
    in fewer than 330 kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    by_name = {r["name"]: r for r in rows}
    for name in BY_COMPONENT_KERNELS:
        assert name in by_name, (name, sorted(n for n in by_name if "split_kernel" in n))
        r = by_name[name]
        print("%-70s vgpr %3d  agpr %3d  sgpr %3d  lds %6d  scratch %4d" % (name, r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
    built = sorted(n for n in by_name if n.startswith(("pbs_split_kernel<", "pbs_ga_split_kernel<", "pbs_kernel<")) and n.endswith(", true>"))
    assert built == sorted(BY_COMPONENT_KERNELS), built
    assert len(rows) < 330, len(rows)


def test_lds_barrier_check_covers_the_by_component_forms():
    """tools/check_lds_barriers.py builds the one-CU by-component forms (two-wavefront teams, barriers through workgroup_sync() only) and finds no LDS read behind
    the barrier its exchange stands in front of."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_barriers as chk
    names = [f[0] for f in chk.FORMS]
    assert sum("by component" in n for n in names) >= 5 and any("Galois" in n and "by component" in n for n in names) and any("throughput form" in n for n in names), names
    assert chk.build_and_check() == []


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cus(eng):
    import torch
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _ordered(eng, bsk, order):
    """a second handle of the key on the same device with the order set (the original keeps AUTO)"""
    key, _ = eng.clone_key(bsk)
    assert key.product_order == bsk.product_order
    key.set_product_order(order)
    assert key.product_order == order
    return key


@pytest.fixture(scope="module")
def lvl2(eng, oracle):
    """the TFHEpp lvl2 set (N = 2048, l = 4, Bg = 2^9, n = 632), a handle of its key per order, and 128 distinct ciphertexts -- among them the skipped-step inputs
    of test_split_kernel_batch_sizes_pairs_and_alone -- with the oracle's programmable bootstrap of each in both orders (batches are tiled from these)"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K = _keyset("lvl2", eng, oracle)
    P = K["P"]
    l, Bg = P["l"], P["Bg_bit"]
    lut = np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64)
    tv = host.torus_packing(lut, 1, P["N"])
    host.seed(SEED + 77)
    cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(128)], K["lk"])
    cts[3, 5] = 0            # a step that is skipped (src/bootstrap.c:114)
    cts[3, 6] = 2 ** 50      # rounds to abar = 0 as well
    want = {}
    for order in ("reference", "by_component"):
        with oracle.product_order(order):
            want[order] = np.stack(_oracle_map(lambda b: oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], l, Bg, 3, 0, 0), range(128)))
    keys = {"auto": K["bsk"], "reference": _ordered(eng, K["bsk"], "reference"), "by_component": _ordered(eng, K["bsk"], "by_component")}
    assert K["bsk"].product_order == "auto"
    yield dict(K=K, P=P, lut=lut, tv=tv, d_tv=ma.to_device(tv[None], eng.device), cts=cts, want=want, keys=keys)
    keys["reference"].free()
    keys["by_component"].free()


def _tiled(a, B):
    return a[np.arange(B) % a.shape[0]]


def _pbs(eng, S, order, B):
    import mosfhet_amd as ma
    return ma.to_numpy(eng.programmable_bootstrap(S["keys"][order], S["d_tv"], ma.to_device(_tiled(S["cts"], B), eng.device), 3, 0, 0))


@pytest.mark.gpu
def test_setter_validates_and_clone_copies(eng, lvl2):
    import mosfhet_amd as ma
    key = lvl2["keys"]["by_component"]
    with pytest.raises(ma.MosfhetHipError, match="product order"):
        key.set_product_order("fastest")
    assert ma.lib().mosfhet_hip_bsk_set_product_order(key.h, 3) == -1 and b"unknown order" in ma.lib().mosfhet_hip_last_error()
    assert key.product_order == "by_component"
    replica, _ = eng.clone_key(key)          # replicas sum alike
    assert replica.product_order == "by_component"
    replica.free()
    assert eng.bootstrap_plan(key, 600)["family"] == "throughput_by_component" and eng.bootstrap_plan(lvl2["keys"]["auto"], 600)["family"] == "throughput"


@pytest.mark.gpu
def test_by_component_key_at_every_batch_size(eng, oracle, lvl2, cus):
    """A BY_COMPONENT key: EVERY output word of programmable_bootstrap equals the oracle in the by-component order at batch sizes on both sides of every kernel
    switch-over (split kernel | one-CU form | throughput form in one and in several residency rounds) -- and the split switches (no two-CU kernel at all; every bootstrap of
    the split kernel taken alone) change nothing: they are performance switches for such a key."""
    from mosfhet_amd import engine
    sizes = (1, cus // 2, cus // 2 + 1, cus + 1, 513, 4 * cus + 76)
    outs = {}
    for B in sizes:
        outs[B] = _pbs(eng, lvl2, "by_component", B)
        if B <= cus // 2:
            assert engine.split_last_launch()[0] == B          # two CUs per bootstrap, as under AUTO
        _assert_all_outputs_equal(outs[B], list(_tiled(lvl2["want"]["by_component"], B)), "%d bootstraps of a by-component key" % B)
    try:
        engine.set_split_max_batch(0)
        for B in sizes:
            assert (_pbs(eng, lvl2, "by_component", B) == outs[B]).all(), ("split_max_batch(0)", B)
        engine.set_split_max_batch(-1)
        engine.set_split_wait_limit(0)
        for B in sizes:
            assert (_pbs(eng, lvl2, "by_component", B) == outs[B]).all(), ("split_wait_limit(0)", B)
    finally:
        engine.set_split_max_batch(-1)
        engine.set_split_wait_limit(200000)


@pytest.mark.gpu
def test_by_component_large_batches_on_two_streams_at_once(eng, oracle, lvl2):
    """The throughput form parks a partial sum in device memory per workgroup: launches of one host thread on two streams at once (what the host-struct pipeline
    does with its chunks) have a parking buffer each, and every output of every launch equals the oracle."""
    import torch
    import mosfhet_amd as ma
    B = 1100
    d_ct = [ma.to_device(np.roll(_tiled(lvl2["cts"], B), i, axis=0), eng.device) for i in range(2)]
    want = [np.roll(_tiled(lvl2["want"]["by_component"], B), i, axis=0) for i in range(2)]
    streams = [torch.cuda.Stream(device=eng.device) for _ in range(2)]
    outs = [[], []]
    torch.cuda.synchronize()
    for rep in range(2):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs[i].append(eng.programmable_bootstrap(lvl2["keys"]["by_component"], lvl2["d_tv"], d_ct[i], 3, 0, 0))
    torch.cuda.synchronize()
    for i in range(2):
        for o in outs[i]:
            _assert_all_outputs_equal(ma.to_numpy(o), list(want[i]), "1100 bootstraps of a by-component key on stream %d of two" % i)


@pytest.mark.gpu
def test_by_component_without_parking_memory(eng, oracle, lvl2, cus):
    """What a launch does when the throughput form's parking memory is refused (set_bycomp_parking(0) takes that path): the one-CU form in residency rounds -- the
    same words, plain and in row mode."""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    B = 4 * cus + 76
    try:
        engine.set_bycomp_parking(0)
        _assert_all_outputs_equal(_pbs(eng, lvl2, "by_component", B), list(_tiled(lvl2["want"]["by_component"], B)), "%d bootstraps of a by-component key without parking" % B)
        g_off = eng.functional_bootstrap_trgsw_phase1(lvl2["keys"]["by_component"], ma.to_device(_tiled(lvl2["cts"][:4], 140), eng.device), 4).cpu().numpy()
    finally:
        engine.set_bycomp_parking(1)
    g_on = eng.functional_bootstrap_trgsw_phase1(lvl2["keys"]["by_component"], ma.to_device(_tiled(lvl2["cts"][:4], 140), eng.device), 4).cpu().numpy()
    assert (g_on.view(np.uint64) == g_off.view(np.uint64)).all()


@pytest.mark.gpu
def test_reference_key_at_the_default_switches(eng, oracle, lvl2, cus):
    """A REFERENCE key at the library's default switches (split kernels on): every output equals the oracle in the reference's order, also at the batch sizes that
    an AUTO key sends to the split kernel."""
    for B in (1, cus // 2, 513):
        _assert_all_outputs_equal(_pbs(eng, lvl2, "reference", B), list(_tiled(lvl2["want"]["reference"], B)), "%d bootstraps of a reference-order key" % B)


@pytest.mark.gpu
def test_auto_key_keeps_todays_choice(eng, oracle, lvl2):
    """The default cannot drift: an AUTO key's single bootstrap is the split kernel's (by component), its batch of 513 the throughput kernel's (reference order)."""
    _assert_all_outputs_equal(_pbs(eng, lvl2, "auto", 1), list(lvl2["want"]["by_component"][:1]), "one bootstrap of an AUTO key")
    _assert_all_outputs_equal(_pbs(eng, lvl2, "auto", 513), list(_tiled(lvl2["want"]["reference"], 513)), "513 bootstraps of an AUTO key")


@pytest.mark.gpu
def test_the_two_orders_differ_as_words_and_agree_by_phase(eng, oracle, lvl2):
    """One batch of 128 under both orders: different words (as ciphertexts the two differ freely), phases within 2^47 of each other, both decrypt within 2^58 --
    the bounds test_split_kernel_batch_sizes_pairs_and_alone uses for this pair of orders at this key set."""
    from mosfhet_amd import host
    a, b = _pbs(eng, lvl2, "by_component", 128), _pbs(eng, lvl2, "reference", 128)
    assert (a != b).any()
    s = lvl2["K"]["out_key"].s
    ph_a, ph_b = host.tlwe_phase(a, s), host.tlwe_phase(b, s)
    assert oracle.torus_dist(ph_a, ph_b).max() < 2.0 ** 47
    keep = np.arange(128) != 3                       # (input 3's mask was edited: it no longer encrypts its message)
    for ph in (ph_a, ph_b):
        assert oracle.torus_dist(ph[keep], lvl2["lut"][np.arange(128) % 4][keep]).max() < 2.0 ** 58


@pytest.mark.gpu
def test_by_component_key_other_entries_of_the_parameter_block(eng, oracle, lvl2, cus):
    """TRLWE output with one test vector per ciphertext, blind_rotate in place on caller accumulators and the TRGSW-accumulator row mode under a BY_COMPONENT key, in
    the one-CU form (CUs / 2 + 1 workgroups) and in the throughput form (beyond 512): bit for bit against the oracle in the by-component order."""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K, P, key = lvl2["K"], lvl2["P"], lvl2["keys"]["by_component"]
    N, l, Bg = P["N"], P["l"], P["Bg_bit"]
    rng = np.random.default_rng(61)
    host.seed(SEED + 78)
    D = 16                                           # distinct inputs; batches are tiled
    cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(D)], K["lk"])
    tvs, accs = _rand_u64(rng, D, 2, N), _rand_u64(rng, D, 2, N)
    with oracle.product_order("by_component"):
        want_wo = np.stack(_oracle_map(lambda b: oracle.functional_bootstrap_wo_extract(tvs[b], cts[b], K["bk_dft"], l, Bg, 4), range(D)))
        want_br = np.stack(_oracle_map(lambda b: oracle.blind_rotate(accs[b], cts[b, :-1].copy(), K["bk_dft"], l, Bg), range(D)))
        want_g = np.stack(_oracle_map(lambda b: oracle.functional_bootstrap_trgsw_phase1(cts[b], K["bk_dft"], l, Bg, 4), range(4)))
    for B in (cus // 2 + 1, 513):
        d_ct = ma.to_device(_tiled(cts, B), eng.device)
        out = ma.to_numpy(eng.functional_bootstrap_wo_extract(key, ma.to_device(_tiled(tvs, B), eng.device), d_ct, 4))
        _assert_all_outputs_equal(out, list(_tiled(want_wo, B)), "wo_extract with per-ciphertext test vectors, %d" % B)
        d_acc = ma.to_device(_tiled(accs, B), eng.device)
        eng.blind_rotate_(key, d_acc, d_ct)
        _assert_all_outputs_equal(ma.to_numpy(d_acc), list(_tiled(want_br, B)), "blind_rotate in place, %d" % B)
    # x 2l rows: just past the split kernel's batches; 520 workgroups (the throughput form, one launch); 4 CUs + 8 l workgroups more than one residency round of 4 x CUs
    # (rounds of whole inputs, the parking memory sized for one round)
    for inputs in (cus // 2 // (2 * l) + 1, 65, 4 * cus // (2 * l) + 12):
        g_d = eng.functional_bootstrap_trgsw_phase1(key, ma.to_device(_tiled(cts[:4], inputs), eng.device), 4)
        g = ma.engine.slot_order_to_oracle(g_d.cpu().numpy().reshape(inputs * 2 * l * 2, N), N).reshape(inputs, 2 * l, 2, N)
        _assert_all_outputs_equal(g, list(_tiled(want_g, inputs)), "TRGSW-accumulator rows of %d inputs" % inputs)


@pytest.mark.gpu
@pytest.mark.parametrize("l,Bg", [(2, 15), (4, 9), (6, 7), (2, 8), (4, 7)])
def test_by_component_gadgets(eng, oracle, cus, l, Bg):
    """Every instantiation of the one-CU and of the throughput by-component kernels (compile-time 4 x 2^9 and 6 x 2^7, run-time l = 2, 4, 6) on short keys at N = 2048: batches of 3 (split
    kernel), CUs / 2 + 1 (one-CU form) and 520 (throughput form, ONE launch: these keys fit the L2s; rounds: the next test) of a BY_COMPONENT key, bit for bit against the oracle in the by-component order."""
    import mosfhet_amd as ma
    N = 2048
    r = oracle.Rng(0x6AD6E7 + 4096 * l + 64 * Bg + N)
    n, sigma = 16, 2.0 ** -45
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)
    bk = oracle.gen_bootstrap_key(r, lwe_s, s.reshape(1, N), l, Bg, sigma)
    bk_dft = oracle.bk_to_dft(bk, 1, l)
    bsk = eng.load_bootstrap_key(bk, 1, l, Bg)
    bsk.set_product_order("by_component")
    tv = oracle.trlwe_torus_packing(oracle.u64(r.words(4)), 1, N)
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(m / 8.0), lwe_s, 2.0 ** -25) for m in (0, 1, 2, 3, 1, 2, 0)])
    cts[4] = oracle.u64(r.words(n + 1))                                  # arbitrary mask / body words
    with oracle.product_order("by_component"):
        want_fb = np.stack([oracle.functional_bootstrap(tv, c, bk_dft, l, Bg, 4) for c in cts])
        want_pb = np.stack([oracle.programmable_bootstrap(tv, c, bk_dft, l, Bg, 4, 2, 1) for c in cts])
    d_tv = ma.to_device(tv[None], eng.device)
    for B in (3, cus // 2 + 1, 520):
        d_ct = ma.to_device(_tiled(cts, B), eng.device)
        _assert_all_outputs_equal(ma.to_numpy(eng.functional_bootstrap(bsk, d_tv, d_ct, 4)), list(_tiled(want_fb, B)), "functional, %d x %d, %d" % (l, Bg, B))
        _assert_all_outputs_equal(ma.to_numpy(eng.programmable_bootstrap(bsk, d_tv, d_ct, 4, 2, 1)), list(_tiled(want_pb, B)), "programmable, %d x %d, %d" % (l, Bg, B))
    bsk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,Bg", [(1024, 2, 8), (2048, 3, 10)])
def test_ungoverned_keys_accept_the_setter_and_keep_the_reference_order(eng, oracle, N, l, Bg):
    """Where no by-component kernel exists (another ring; an odd gadget length at N = 2048) results do not depend on the batch size already: the setter accepts
    every valid value and the bits stay the reference order's."""
    import mosfhet_amd as ma
    r = oracle.Rng(0x0DD + 64 * Bg + N)
    n = 16
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)
    bk = oracle.gen_bootstrap_key(r, lwe_s, s.reshape(1, N), l, Bg, 2.0 ** -45)
    bk_dft = oracle.bk_to_dft(bk, 1, l)
    bsk = eng.load_bootstrap_key(bk, 1, l, Bg)
    tv = oracle.trlwe_torus_packing(oracle.u64(r.words(4)), 1, N)
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(m / 8.0), lwe_s, 2.0 ** -25) for m in (0, 1, 2, 3, 1)])
    want = np.stack([oracle.functional_bootstrap(tv, c, bk_dft, l, Bg, 4) for c in cts])          # reference order
    d_tv = ma.to_device(tv[None], eng.device)
    for order in ("by_component", "reference", "auto"):
        bsk.set_product_order(order)
        assert bsk.product_order == order
        for B in (3, 520):
            out = ma.to_numpy(eng.functional_bootstrap(bsk, d_tv, ma.to_device(_tiled(cts, B), eng.device), 4))
            _assert_all_outputs_equal(out, list(_tiled(want, B)), "N = %d, l = %d, %s, %d" % (N, l, order, B))
    bsk.free()


@pytest.mark.gpu
def test_by_component_compositions(eng, oracle, lvl2):
    """Compositions on BY_COMPONENT keys at one GPU's share of a sharded batch (128: split kernel) and beyond every latency kernel (600: the throughput form):
    full-domain functional bootstrap, multi-value CLOT21 with 8 LUTs, key switch + bootstrap.  The first 128 outputs against the oracle's composition in the
    by-component order, the rest against those (the inputs are tiled)."""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K, P, key = lvl2["K"], lvl2["P"], lvl2["keys"]["by_component"]
    N, l, Bg, D = P["N"], P["l"], P["Bg_bit"], 128
    ksk, dksk = _ksk_for(K, eng)
    lut8 = np.array([host.double2torus(((3 * i + 1) % 8) / 8.0) for i in range(8)], dtype=np.uint64)
    tv8 = host.torus_packing_many_lut(lut8, 1, N, 4, 2)
    host.seed(SEED + 79)
    cts8 = host.tlwe_samples([(b % 8) << 61 for b in range(D)], K["lk"])
    lut16 = np.array([host.double2torus(((5 * i + 3) % 16) / 16.0) for i in range(16)], dtype=np.uint64)
    tvm = host.torus_packing_many_lut(lut16, 1, N, 2, 8)
    ctsm = host.tlwe_samples([host.double2torus(m / 4.0) for m in np.arange(D) % 2], K["lk"])
    big = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(D)], K["out_key"])
    with oracle.product_order("by_component"):
        want_fd = np.stack(_oracle_map(lambda b: oracle.full_domain_functional_bootstrap(tv8, cts8[b], K["bk_dft"], ksk, l, Bg, P["t"], P["base_bit"], 3), range(D)))
        want_mv = np.stack(_oracle_map(lambda b: oracle.multivalue_bootstrap_CLOT21(tvm, ctsm[b], K["bk_dft"], l, Bg, 2, 8), range(D)))
        want_ks = np.stack(_oracle_map(lambda b: oracle.functional_bootstrap(lvl2["tv"], oracle.tlwe_keyswitch(big[b], ksk, P["n"], P["t"], P["base_bit"]), K["bk_dft"], l, Bg, 4),
                                       range(D)))
    for B in (128, 600):
        fd = ma.to_numpy(eng.full_domain_functional_bootstrap(key, dksk, ma.to_device(tv8[None], eng.device), ma.to_device(_tiled(cts8, B), eng.device), 3))
        _assert_all_outputs_equal(fd, list(_tiled(want_fd, B)), "%d full-domain functional bootstraps" % B)
        mv = ma.to_numpy(eng.multivalue_bootstrap_CLOT21(key, ma.to_device(tvm[None], eng.device), ma.to_device(_tiled(ctsm, B), eng.device), 2, 8))
        _assert_all_outputs_equal(mv, list(_tiled(want_mv, B)), "%d multi-value bootstraps" % B)
        gate = ma.to_numpy(eng.keyswitch_functional_bootstrap(dksk, key, lvl2["d_tv"], ma.to_device(_tiled(big, B), eng.device), 4))
        _assert_all_outputs_equal(gate, list(_tiled(want_ks, B)), "%d key switch + bootstrap" % B)


@pytest.mark.gpu
def test_by_component_circuit_bootstrap_3(eng, oracle, lvl2):
    """circuit_bootstrap_3 (row mode: a 2l-slot LUT, l accumulator rows per input) on the lvl2 key set (n = 632: the key does not fit the L2s) with a BY_COMPONENT key:
    B = 128 inputs (512 workgroups: the one-CU form) and B = 600 (2400 workgroups: the throughput form in three residency rounds of whole inputs, paced).  The first
    128 outputs against the oracle's composition in the by-component order, the rest against those (tiled inputs).  The private key-switch pair is the reference test's
    (t = 20, 2 bits); the packing key has one digit of 2 bits -- the words are what is compared, and its 200 MB are made by the oracle in seconds."""
    import mosfhet_amd as ma
    K, P, key = lvl2["K"], lvl2["P"], lvl2["keys"]["by_component"]
    N, l, Bg = P["N"], P["l"], P["Bg_bit"]
    r = oracle.Rng(0xCB2)
    s = np.ascontiguousarray(K["rk"].s[0], dtype=np.uint64)
    lwe_s = np.ascontiguousarray(K["lk"].s, dtype=np.uint64)
    ks0, ks1 = oracle.gen_priv_ks_key(r, s, s, 20, 2, P["rlwe_sigma"])
    kskb = oracle.gen_packing1_ks_key(r, s, s, 1, 2, P["rlwe_sigma"])
    kska, pk = eng.load_trlwe_ks_keys(np.stack([ks0, ks1]), 2), eng.load_packing1_key(kskb, 2)
    ks0_dft, ks1_dft = oracle.ks_to_dft(ks0), oracle.ks_to_dft(ks1)
    D = 128
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(0.25 if b % 3 else 0.0), lwe_s, P["lwe_sigma"]) for b in range(D)])
    with oracle.product_order("by_component"):
        want = np.stack(_oracle_map(lambda b: oracle.circuit_bootstrap_3(cts[b], K["bk_dft"], ks0_dft, ks1_dft, 2, kskb, 2, l, Bg), range(D)))
    for B in (128, 600):
        assert eng.bootstrap_plan(key, B * l, rows=l)["family"] == ("latency_by_component" if B == 128 else "throughput_by_component")
        out = ma.to_numpy(eng.circuit_bootstrap_3(key, kska, pk, ma.to_device(_tiled(cts, B), eng.device)))
        _assert_all_outputs_equal(out, list(_tiled(want, B)), "%d circuit bootstraps" % B)
    for h in (kska, pk):
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("l,Bg,n", [(2, 15, 780), (4, 7, 392), (6, 7, 264)])
def test_by_component_gadgets_in_residency_rounds(eng, oracle, cus, l, Bg, n):
    """The run-time-gadget instantiations (l = 2, 4) and 6 x 2^7 of the throughput by-component kernel on keys of more than 96 MiB -- beyond the L2s, so the launcher
    cuts the batch into paced residency rounds: 4 CUs + 76 bootstraps (two rounds) of a BY_COMPONENT key, bit for bit against the oracle in the by-component order."""
    import mosfhet_amd as ma
    N = 2048
    r = oracle.Rng(0x6AD6E8 + 4096 * l + 64 * Bg + N)
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)
    bk = oracle.gen_bootstrap_key(r, lwe_s, s.reshape(1, N), l, Bg, 2.0 ** -45)
    assert bk.nbytes > (96 << 20)
    bk_dft = oracle.bk_to_dft(bk, 1, l)
    bsk = eng.load_bootstrap_key(bk, 1, l, Bg)
    bsk.set_product_order("by_component")
    tv = oracle.trlwe_torus_packing(oracle.u64(r.words(4)), 1, N)
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus(m / 8.0), lwe_s, 2.0 ** -25) for m in (0, 1, 2, 3, 1)])
    cts[4] = oracle.u64(r.words(n + 1))
    with oracle.product_order("by_component"):
        want = np.stack(_oracle_map(lambda b: oracle.programmable_bootstrap(tv, cts[b], bk_dft, l, Bg, 4, 2, 1), range(len(cts))))
    B = 4 * cus + 76
    assert eng.bootstrap_plan(bsk, B) == dict(family="throughput_by_component", by_component=True, rounds=2)
    out = ma.to_numpy(eng.programmable_bootstrap(bsk, ma.to_device(tv[None], eng.device), ma.to_device(_tiled(cts, B), eng.device), 4, 2, 1))
    _assert_all_outputs_equal(out, list(_tiled(want, B)), "%d bootstraps at %d x 2^%d in two residency rounds" % (B, l, Bg))
    bsk.free()


@pytest.mark.gpu
def test_by_component_galois_bootstrap(eng, oracle):
    """The Galois family at N = 2048, l = 4 (random automorphism key set, a real Galois bootstrap key with a short LWE key): a BY_COMPONENT key at 32 (two CUs per
    bootstrap), 300 (the one-CU form in one launch) and 520 (in residency rounds), with and without extraction, and blind_rotate_ga in place at the same sizes, against
    the oracle with its external products by component; a REFERENCE key at 32, both entry points, against the reference order."""
    import mosfhet_amd as ma
    N, l, Bg, n = 2048, 4, 9, 16
    r = oracle.Rng(0x6A2)
    rng = np.random.default_rng(62)
    lwe_s, s = oracle.gen_binary_key(r, n), oracle.gen_binary_key(r, N)
    ak = _rand_u64(rng, N, l, 2, N)
    gak, ak_dft = eng.load_automorphism_keys(ak, Bg), oracle.ks_to_dft(ak)
    bkg = oracle.gen_bootstrap_key_ga(r, lwe_s, s.reshape(1, N), l, Bg, 2.0 ** -45)
    bkg_dft, bskg = oracle.bk_to_dft(bkg, 1, l), eng.load_bootstrap_key(bkg, 1, l, Bg)
    tv = oracle.trlwe_torus_packing(oracle.u64(r.words(4)), 1, N)
    cts = np.stack([oracle.tlwe_sample(r, oracle.double2torus((b % 4) / 8.0), lwe_s, 2.0 ** -25) for b in range(32)])
    d_tv = ma.to_device(tv[None], eng.device)
    want = {}
    for order in ("reference", "by_component"):
        with oracle.product_order(order):
            for extract in (True, False):
                want[order, extract] = np.stack(_oracle_map(lambda b: oracle.functional_bootstrap_ga(tv, cts[b], bkg_dft, ak_dft, l, Bg, 4, extract=extract), range(32)))
    bskg.set_product_order("by_component")
    for B in (32, 300, 520):
        for extract in (True, False):
            out = ma.to_numpy(eng.functional_bootstrap_ga(bskg, gak, d_tv, ma.to_device(_tiled(cts, B), eng.device), 4, extract=extract))
            _assert_all_outputs_equal(out, list(_tiled(want["by_component", extract], B)), "%d Galois bootstraps by component, extract %s" % (B, extract))
    # blind_rotate_ga in place on caller accumulators: the same launcher, the same rule
    accs = _rand_u64(rng, 32, 2, N)
    want_br = {}
    for order in ("reference", "by_component"):
        with oracle.product_order(order):
            want_br[order] = np.stack(_oracle_map(lambda b: oracle.blind_rotate_ga(accs[b], cts[b, :n].copy(), bkg_dft, ak_dft, l, Bg), range(32)))
    assert (want_br["reference"] != want_br["by_component"]).any()
    for B in (32, 300, 520):
        out = ma.to_numpy(eng.blind_rotate_ga(bskg, gak, ma.to_device(_tiled(accs, B), eng.device), ma.to_device(_tiled(cts, B), eng.device)))
        _assert_all_outputs_equal(out, list(_tiled(want_br["by_component"], B)), "blind_rotate_ga of %d under a by-component key" % B)
    bskg.set_product_order("reference")
    out = ma.to_numpy(eng.functional_bootstrap_ga(bskg, gak, d_tv, ma.to_device(cts, eng.device), 4))
    _assert_all_outputs_equal(out, list(want["reference", True]), "32 Galois bootstraps of a reference-order key")
    out = ma.to_numpy(eng.blind_rotate_ga(bskg, gak, ma.to_device(accs, eng.device), ma.to_device(cts, eng.device)))
    _assert_all_outputs_equal(out, list(want_br["reference"]), "blind_rotate_ga of 32 under a reference-order key")
    bskg.free()
    gak.free()


@pytest.mark.gpu
def test_sharded_host_struct_batches_do_not_depend_on_the_shards(native_lib, tmp_path):
    """tests/c/product_order.c through the drop-in API with GPU 0 listed twice, then once: lvl2 keys with BY_COMPONENT and with REFERENCE give, for sharded batches of
    300 host structs, the words of the 300 single calls on the primary context; an AUTO key agrees by phase."""
    exe = str(tmp_path / "product_order")
    libdir = os.path.join(ROOT, "mosfhet_amd")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "product_order.c"),
                           "-o", exe, "-pthread", "-L" + libdir, "-lmosfhet_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    for n_dev in ("2", "1"):
        r = subprocess.run([exe, n_dev], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        print(r.stdout)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-3000:]
