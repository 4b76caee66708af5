"""SET_1's throughput bootstrap kernel with four ciphertexts per workgroup (pbs_group_kernel<Fft1024, 2, 8, 4>; capi.hip: mosfhet_hip_set_pbs_group).

The four one-wavefront teams of a workgroup are independent bootstraps that only keep the same pace over the bootstrap key, so every output word must equal what one
team per workgroup (G = 1) gives and what the oracle gives.  All GPU tests force G = 4 through the setter (mode 4: at any batch size) on SET_1's ring and gadget
(N = 1024, l = 2, Bg = 2^8) -- the production instantiation -- mostly with a short LWE side (n = 16: the step loop does not care how long it is)."""
import os

import numpy as np
import pytest

SEED = 0x4D4F5346
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng(native_lib):
    import mosfhet_amd as ma
    e = ma.Engine(0)
    yield e
    e.close()


_KEYS = {}


def _keys(eng, oracle, n, N=1024, l=2, Bg_bit=8):
    """a key set on SET_1's noise parameters with the LWE dimension, ring and gadget asked for; cached per session"""
    tag = (n, N, l, Bg_bit)
    if tag not in _KEYS:
        import mosfhet_amd as ma
        from mosfhet_amd import host
        P = dict(ma.PARAMS_SET1 if N == 1024 else ma.PARAMS_LVL2)
        host.seed(SEED + n + N + 16 * l + Bg_bit)
        lk = host.LweKey(n, P["lwe_sigma"])
        rk = host.RlweKey(N, 1, P["rlwe_sigma"])
        bk = host.gen_bootstrap_key(rk, lk, l, Bg_bit)
        _KEYS[tag] = dict(n=n, N=N, l=l, Bg_bit=Bg_bit, lk=lk, rk=rk, bk=bk, bsk=eng.load_bootstrap_key(bk, 1, l, Bg_bit), bk_dft=oracle.bk_to_dft(bk, 1, l))
    return _KEYS[tag]


@pytest.fixture(autouse=True)
def kernel_switches(native_lib):
    """every test of this file runs the THROUGHPUT kernel (no latency kernels, no two-CU kernel) and leaves the library's switches at their defaults"""
    from mosfhet_amd import engine
    engine.set_team_max_batch(0)
    engine.set_wide_team_max_batch(0)
    engine.set_split_max_batch(0)
    yield
    engine.set_pbs_group(-1)
    engine.set_team_max_batch(512)
    engine.set_wide_team_max_batch(512)
    engine.set_split_max_batch(-1)


def _both(call, expect_grouped=4):
    """call() -> numpy, once with one ciphertext per workgroup and once with four forced; the launcher's own account of what it launched is checked"""
    from mosfhet_amd import engine
    engine.set_pbs_group(0)
    plain = call()
    assert engine.last_pbs_group() == 1
    engine.set_pbs_group(4)
    grouped = call()
    assert engine.last_pbs_group() == expect_grouped
    return plain, grouped


def _samples(K, count, rng):
    from mosfhet_amd import host
    lut = rng.integers(0, 2 ** 64, size=4, dtype=np.uint64)
    tv = host.torus_packing(lut, 1, K["N"])
    cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(count)], K["lk"])
    return tv, cts


def _pbs_three_ways(eng, oracle, K, tv, cts, which=None):
    import mosfhet_amd as ma
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    plain, grouped = _both(lambda: ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct, 3)))
    assert plain.shape == grouped.shape == (len(cts), K["N"] + 1)
    differ = np.nonzero((plain != grouped).any(axis=1))[0]
    assert len(differ) == 0, "ciphertexts whose grouped output differs from the ungrouped one: %s" % differ[:16].tolist()
    for b in (range(len(cts)) if which is None else which):
        want = oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)
        assert (grouped[b] == want).all(), "ciphertext %d of %d differs from the oracle" % (b, len(cts))


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8, 9, 13])
def test_ragged_groups(eng, oracle, count):
    """full and ragged last workgroups: the teams past the end run along (every team passes every barrier) and store nothing"""
    K = _keys(eng, oracle, 16)
    tv, cts = _samples(K, count, np.random.default_rng(100 + count))
    _pbs_three_ways(eng, oracle, K, tv, cts)


@pytest.mark.gpu
def test_ragged_group_at_the_full_lwe_dimension(eng, oracle):
    """SET_1 as it is (n = 585), 5 ciphertexts: one full workgroup and one with a single live team"""
    K = _keys(eng, oracle, 585)
    tv, cts = _samples(K, 5, np.random.default_rng(7))
    _pbs_three_ways(eng, oracle, K, tv, cts)


@pytest.mark.gpu
def test_skipped_steps_inside_a_group(eng, oracle):
    """a step whose mod-switched mask word is 0 is skipped by ITS team only (src/bootstrap.c:114): one ciphertext skips several steps, one skips them all (its output is
    the extraction of the rotated test vector), their group mates skip none -- the teams' meeting stands in front of the skip, so all of them still arrive at it"""
    K = _keys(eng, oracle, 16)
    tv, cts = _samples(K, 8, np.random.default_rng(11))
    cts[2, [0, 3, 4, 9, 15]] = 0
    cts[2, 7] = 2 ** 51            # rounds to abar = 0 as well
    cts[5, :-1] = 0
    _pbs_three_ways(eng, oracle, K, tv, cts)


@pytest.mark.gpu
def test_entry_points_that_share_the_launcher(eng, oracle):
    """6 ciphertexts (one full workgroup, one half full) through the other callers of the launcher: grouped == ungrouped"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K = _keys(eng, oracle, 16)
    rng = np.random.default_rng(12)
    tv, cts = _samples(K, 6, rng)
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    # programmable_bootstrap's pre-processing
    a, b = _both(lambda: ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct, 3, 2, 1)))
    assert (a == b).all()
    assert (b[4] == oracle.programmable_bootstrap(tv, cts[4], K["bk_dft"], K["l"], K["Bg_bit"], 3, 2, 1)).all()
    # no extraction: the rotated TRLWE
    a, b = _both(lambda: ma.to_numpy(eng.functional_bootstrap_wo_extract(K["bsk"], d_tv, d_ct, 4)))
    assert a.shape == (6, 2, K["N"]) and (a == b).all()
    assert (b[5] == oracle.functional_bootstrap_wo_extract(tv, cts[5], K["bk_dft"], K["l"], K["Bg_bit"], 4)).all()
    # one test vector per ciphertext
    tvs = np.stack([host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, K["N"]) for _ in range(6)])
    d_tvs = ma.to_device(tvs, eng.device)
    a, b = _both(lambda: ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tvs, d_ct, 3)))
    assert (a == b).all()
    assert (b[5] == oracle.programmable_bootstrap(tvs[5], cts[5], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)).all()
    # blind_rotate alone, in place on the caller's accumulators
    accs = rng.integers(0, 2 ** 64, size=(6, 2, K["N"]), dtype=np.uint64)
    a, b = _both(lambda: ma.to_numpy(eng.blind_rotate_(K["bsk"], ma.to_device(accs, eng.device), d_ct)))
    assert (a == b).all()
    assert (b[4] == oracle.blind_rotate(accs[4], cts[4, :-1].copy(), K["bk_dft"], K["l"], K["Bg_bit"])).all()


@pytest.mark.gpu
def test_what_has_no_grouped_kernel_stays_on_one_team_per_workgroup(eng, oracle):
    """TRGSW accumulator rows, N = 2048 and a run-time gadget at 6 ciphertexts with the grouped kernel forced: the launcher reports one ciphertext per workgroup, same bits"""
    import mosfhet_amd as ma
    K = _keys(eng, oracle, 16)
    rng = np.random.default_rng(13)
    _, cts = _samples(K, 6, rng)
    d_ct = ma.to_device(cts, eng.device)
    a, b = _both(lambda: ma.to_numpy(eng.functional_bootstrap_trgsw_phase1(K["bsk"], d_ct, 4)), expect_grouped=1)   # rows = 2l per ciphertext
    assert a.view(np.uint64).shape == b.view(np.uint64).shape and (a.view(np.uint64) == b.view(np.uint64)).all()
    for K2 in (_keys(eng, oracle, 16, N=2048, l=4, Bg_bit=9), _keys(eng, oracle, 16, l=2, Bg_bit=7)):
        tv, cts = _samples(K2, 6, rng)
        d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
        a, b = _both(lambda: ma.to_numpy(eng.programmable_bootstrap(K2["bsk"], d_tv, d_ct, 3)), expect_grouped=1)
        assert (a == b).all()
        assert (b[5] == oracle.programmable_bootstrap(tv, cts[5], K2["bk_dft"], K2["l"], K2["Bg_bit"], 3, 0, 0)).all()


@pytest.mark.gpu
def test_one_residency_round_and_a_ragged_group(eng, oracle):
    """2051 ciphertexts: more workgroups than the device holds at once, and three live teams in the last one"""
    K = _keys(eng, oracle, 16)
    tv, cts = _samples(K, 2051, np.random.default_rng(14))
    _pbs_three_ways(eng, oracle, K, tv, cts, which=[0, 3, 1023, 1024, 2047, 2048, 2049, 2050])


def test_setter_takes_its_three_modes_only(native_lib):
    from mosfhet_amd import engine
    for mode in (0, 1, 4, -1):
        engine.set_pbs_group(mode)
    for mode in (2, 3, 5, 8, -2):
        with pytest.raises(Exception):
            engine.set_pbs_group(mode)


def test_kernel_table_has_the_grouped_instantiation(native_lib):
    """the build's own kernel table (code-object metadata, no GPU): the grouped SET_1 kernel is there, without scratch, within the register budget of two wavefronts per
    SIMD and with four teams' LDS slices (two workgroups per CU); the library stays below its kernel budget"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = kernel_table.table()
    grouped = [r for r in rows if r["name"].startswith("pbs_group_kernel<")]
    assert [r["name"] for r in grouped] == ["pbs_group_kernel<Fft1024, 2, 8, 4>"]
    g = grouped[0]
    assert g["scratch"] == 0, "%s spills %d bytes" % (g["name"], g["scratch"])
    assert g["vgpr"] <= 256 and g["lds"] == 4 * 17408 and g["max_threads"] == 256, g
    assert len(rows) < 330, len(rows)
