"""SET_1's throughput bootstrap kernel with four ciphertexts per workgroup (pbs_group_kernel<Fft1024, 2, 8, 4>; capi.hip: mosfhet_hip_set_pbs_group).

The four one-wavefront teams of a workgroup are independent bootstraps that only keep the same pace over the bootstrap key, so every output word must equal what one
team per workgroup (G = 1) gives and what the oracle gives.  Most GPU tests force G = 4 through the setter (mode 4: at any batch size) on SET_1's ring and gadget
(N = 1024, l = 2, Bg = 2^8) -- the production instantiation -- mostly with a short LWE side (n = 16: the step loop does not care how long it is); the default mode
(1: from one residency round of the device on), which is what production runs, has tests of its own at that threshold.  Every test asks the launcher which kernel
it launched (engine.last_pbs_group(), per host thread).  The one-team kernel's edge tests run on this kernel too: tests/test_gpu_parity.py, `grouped_kernel`."""
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
    """TRGSW accumulator rows, N = 2048, a run-time gadget and circuit_bootstrap's row-mode launch at 6 ciphertexts with the grouped kernel forced: the launcher reports
    one ciphertext per workgroup, same bits"""
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
    # circuit_bootstrap at fewer than 1024 inputs: its l bootstraps per input are ONE launch in row mode (rows = l) -> one ciphertext per workgroup; circuit_bootstrap_2
    # is a single plain bootstrap per input followed by extractions, so it does take the grouped kernel -- the same TRGSWs either way, and the oracle's
    r = oracle.Rng(0xCB16)
    s = K["rk"].s[0]
    sk = oracle.gen_priv_sk_ks_key(r, s, s, 2, 2, 2.0 ** -44)          # [N+1][2][3][2][N]: 100 MB
    kskb = oracle.gen_packing1_ks_key(r, s, s, 2, 2, 2.0 ** -44)       # [N][2][3][2][N]
    dsk, pk = eng.load_priv_key(sk, 2), eng.load_packing1_key(kskb, 2)
    try:
        _, cts = _samples(K, 6, rng)
        d_ct = ma.to_device(cts, eng.device)
        for variant, expect in ((0, 1), (1, 4)):
            a, b = _both(lambda: ma.to_numpy(eng.circuit_bootstrap(K["bsk"], dsk, pk, d_ct, variant)), expect_grouped=expect)
            assert a.shape == (6, 2 * K["l"], 2, K["N"]) and (a == b).all(), variant
            assert (b[5] == oracle.circuit_bootstrap(cts[5], K["bk_dft"], sk, 2, kskb, 2, K["l"], K["Bg_bit"], variant)).all(), variant
    finally:
        dsk.free()
        pk.free()


@pytest.mark.gpu
def test_one_residency_round_and_a_ragged_group(eng, oracle):
    """2051 ciphertexts: more workgroups than the device holds at once, and three live teams in the last one"""
    K = _keys(eng, oracle, 16)
    tv, cts = _samples(K, 2051, np.random.default_rng(14))
    _pbs_three_ways(eng, oracle, K, tv, cts, which=[0, 3, 1023, 1024, 2047, 2048, 2049, 2050])


def _residency_round(eng):
    """ciphertexts from which the default mode groups: 8 one-wavefront teams per CU (capi.hip: resident_teams(64))"""
    import torch
    return 8 * torch.cuda.get_device_properties(eng.device).multi_processor_count


@pytest.mark.gpu
def test_default_mode_groups_from_one_residency_round_on(eng, oracle):
    """mode 1, what production runs: R - 1 ciphertexts take one team per workgroup, R and R + 3 (a ragged last workgroup) take four -- the same words for the
    ciphertexts they share, and the oracle's on both sides of the threshold and in the ragged group"""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    K = _keys(eng, oracle, 16)
    R = _residency_round(eng)
    assert R % 4 == 0
    tv, cts = _samples(K, R + 3, np.random.default_rng(21))
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    engine.set_pbs_group(1)
    outs = {}
    for count, group in ((R - 1, 1), (R, 4), (R + 3, 4)):
        outs[count] = ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct[:count].contiguous(), 3))
        assert engine.last_pbs_group() == group, (count, R, engine.last_pbs_group())
        assert outs[count].shape == (count, K["N"] + 1)
    assert (outs[R][:R - 1] == outs[R - 1]).all() and (outs[R + 3][:R - 1] == outs[R - 1]).all()
    for b in (0, R - 2, R - 1, R, R + 2):
        want = oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)
        for count in (R - 1, R, R + 3):
            if b < count:
                assert (outs[count][b] == want).all(), "ciphertext %d of %d differs from the oracle" % (b, count)


@pytest.mark.gpu
def test_default_mode_leaves_small_batches_to_the_latency_kernel(eng, oracle):
    """the latency kernel at its default threshold: six ciphertexts in mode 1 run pbs_team_kernel and no throughput kernel at all (the launcher reports 0); mode 4
    takes them from it; the family the planner names at one residency round is still the throughput one -- grouping is a form of it"""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    K = _keys(eng, oracle, 16)
    tv, cts = _samples(K, 6, np.random.default_rng(22))
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    engine.set_team_max_batch(512)
    engine.set_wide_team_max_batch(512)
    engine.set_split_max_batch(-1)
    outs = []
    for mode, group in ((1, 0), (4, 4)):
        engine.set_pbs_group(mode)
        outs.append(ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct, 3)))
        assert engine.last_pbs_group() == group, (mode, engine.last_pbs_group())
    assert (outs[0] == outs[1]).all()
    for b in range(6):
        assert (outs[1][b] == oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)).all(), b
    engine.set_pbs_group(-1)
    R = _residency_round(eng)
    assert eng.bootstrap_plan(K["bsk"], R)["family"] == "throughput"
    assert eng.bootstrap_plan(K["bsk"], 6)["family"] == "latency"


@pytest.mark.gpu
def test_environment_variable_is_read_again_after_the_setter_gives_it_back(eng, oracle, monkeypatch):
    """MOSFHET_HIP_PBS_GROUP: set_pbs_group(-1) hands the choice back to the environment, which the library reads at the next launch -- 4 and 0 as the setter's
    modes; anything else ("2", not a number) is the built-in default: grouped from one residency round on"""
    import mosfhet_amd as ma
    from mosfhet_amd import engine
    K = _keys(eng, oracle, 16)
    R = _residency_round(eng)
    tv, cts = _samples(K, R, np.random.default_rng(23))
    d_tv, d_ct = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
    engine.set_pbs_group(0)
    plain = ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct, 3))

    def launch(value, count, group):
        monkeypatch.setenv("MOSFHET_HIP_PBS_GROUP", value)
        engine.set_pbs_group(-1)
        out = ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, d_ct[:count].contiguous(), 3))
        assert engine.last_pbs_group() == group, (value, count, engine.last_pbs_group())
        assert (out == plain[:count]).all(), (value, count)

    try:
        launch("4", 5, 4)
        launch("0", R, 1)
        for value in ("2", "x"):
            launch(value, R - 1, 1)
            launch(value, R, 4)
    finally:
        monkeypatch.delenv("MOSFHET_HIP_PBS_GROUP", raising=False)
        engine.set_pbs_group(-1)
    for b in (0, R - 1):
        assert (plain[b] == oracle.programmable_bootstrap(tv, cts[b], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)).all(), b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 17, 31, 32, 33])
def test_lwe_lengths_around_the_meeting_period(eng, oracle, n):
    """the teams of a workgroup meet in front of steps 0, 16, 32, ...: LWE lengths of one step, one short of / one past one and two periods, five ciphertexts (a full
    workgroup and a single live team); one ciphertext's mask is zero at exactly the steps in front of which the teams meet, so that team skips them and still arrives"""
    K = _keys(eng, oracle, n)
    tv, cts = _samples(K, 5, np.random.default_rng(300 + n))
    cts[1, [i for i in (0, 16, 32) if i < n]] = 0
    _pbs_three_ways(eng, oracle, K, tv, cts)


@pytest.mark.gpu
def test_compositions_that_bootstrap_on_set1s_ring(eng, oracle):
    """key switch + bootstrap (the gate of the benchmark), full_domain_functional_bootstrap (two bootstraps: the second one's input is what the kernels in front of
    it wrote, and here every ciphertext has a test vector of its own) and multivalue_bootstrap_CLOT21 at six ciphertexts: grouped == ungrouped == oracle"""
    import mosfhet_amd as ma
    from mosfhet_amd import host
    K = _keys(eng, oracle, 16)
    N, l, Bg, n = K["N"], K["l"], K["Bg_bit"], K["n"]
    P = ma.PARAMS_SET1
    t, bb = P["t"], P["base_bit"]
    out_key = K["rk"].extracted_lwe_key()
    ksk = host.gen_tlwe_ks_key(K["lk"], out_key, t, bb)
    dksk = eng.load_keyswitch_key(ksk, bb)
    rng = np.random.default_rng(31)
    try:
        # tlwe_keyswitch N -> n, then functional_bootstrap
        tv = host.torus_packing(rng.integers(0, 2 ** 64, size=4, dtype=np.uint64), 1, N)
        d_tv = ma.to_device(tv[None], eng.device)
        wide = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(6)], out_key)
        d_wide = ma.to_device(wide, eng.device)
        a, b = _both(lambda: ma.to_numpy(eng.keyswitch_functional_bootstrap(dksk, K["bsk"], d_tv, d_wide, 4)))
        assert a.shape == (6, N + 1) and (a == b).all()
        for i in range(6):
            sw = oracle.tlwe_keyswitch(wide[i], ksk, n, t, bb)
            assert (b[i] == oracle.functional_bootstrap(tv, sw, K["bk_dft"], l, Bg, 4)).all(), i
        # full-domain bootstrap, one test vector per ciphertext
        tvs = np.stack([host.torus_packing_many_lut(rng.integers(0, 2 ** 64, size=8, dtype=np.uint64), 1, N, 4, 2) for _ in range(6)])
        d_tvs = ma.to_device(tvs, eng.device)
        cts = host.tlwe_samples([(i << 61) % 2 ** 64 for i in range(6)], K["lk"])
        d_ct = ma.to_device(cts, eng.device)
        a, b = _both(lambda: ma.to_numpy(eng.full_domain_functional_bootstrap(K["bsk"], dksk, d_tvs, d_ct, 3)))
        assert a.shape == (6, N + 1) and (a == b).all()
        for i in range(6):
            assert (b[i] == oracle.full_domain_functional_bootstrap(tvs[i], cts[i], K["bk_dft"], ksk, l, Bg, t, bb, 3)).all(), i
        # multi-value bootstrap: one rotation, eight extractions
        mv = host.torus_packing(rng.integers(0, 2 ** 64, size=16, dtype=np.uint64), 1, N)
        d_mv = ma.to_device(mv[None], eng.device)
        cts = host.tlwe_samples([host.double2torus((i % 2) / 4.0) for i in range(6)], K["lk"])
        d_ct = ma.to_device(cts, eng.device)
        a, b = _both(lambda: ma.to_numpy(eng.multivalue_bootstrap_CLOT21(K["bsk"], d_mv, d_ct, 2, 8)))
        assert a.shape == (6, 8, N + 1) and (a == b).all()
        for i in range(6):
            assert (b[i] == oracle.multivalue_bootstrap_CLOT21(mv, cts[i], K["bk_dft"], l, Bg, 2, 8)).all(), i
    finally:
        dksk.free()


@pytest.mark.gpu
def test_grouped_launch_is_captured_in_a_graph_as_it_is(eng, oracle):
    """13 ciphertexts (three full workgroups and a single live team) captured on a side stream with the grouped kernel forced; the mode is set back before the
    replays, which run what was captured: every replay on fresh inputs gives the bits of the eager one-team calls -- no hidden allocation or synchronisation"""
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine, host
    K = _keys(eng, oracle, 16)
    B = 13
    tv, _ = _samples(K, B, np.random.default_rng(41))
    d_tv = ma.to_device(tv[None], eng.device)
    cts = [ma.to_device(host.tlwe_samples([host.double2torus(((b + r) % 4) / 8.0) for b in range(B)], K["lk"]), eng.device) for r in range(2)]
    d_in, d_out = eng.empty(B, K["n"] + 1), eng.empty(B, K["N"] + 1)
    engine.set_pbs_group(0)
    eager = [ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, c, 3)) for c in cts]
    assert engine.last_pbs_group() == 1
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=eng.device)
    d_in.copy_(cts[0])
    torch.cuda.synchronize()
    engine.set_pbs_group(4)
    with torch.cuda.graph(g, stream=side):
        eng.programmable_bootstrap(K["bsk"], d_tv, d_in, 3, out=d_out)
    assert engine.last_pbs_group() == 4              # what the launcher put into the graph
    engine.set_pbs_group(0)
    for r in (0, 1, 0):
        d_in.copy_(cts[r])
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (ma.to_numpy(d_out) == eager[r]).all(), r
    assert engine.last_pbs_group() == 4              # (a replay is no call of the launcher)
    assert (eager[0][4] == oracle.programmable_bootstrap(tv, ma.to_numpy(cts[0])[4], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)).all()


@pytest.mark.gpu
def test_host_threads_group_on_their_own_streams(eng, oracle):
    """two host threads, each on a stream of its own with the same key and its own five ciphertexts, grouped kernel forced: every call gives the single-threaded
    one-team words; the launcher's account is per thread -- each caller reads 4, a thread that made no call reads 0, the main thread still reads its own 1"""
    import threading
    import torch
    import mosfhet_amd as ma
    from mosfhet_amd import engine, host
    K = _keys(eng, oracle, 16)
    tv, _ = _samples(K, 5, np.random.default_rng(51))
    d_tv = ma.to_device(tv[None], eng.device)
    jobs = [ma.to_device(host.tlwe_samples([host.double2torus(((b + 2 * t + 1) % 4) / 8.0) for b in range(5)], K["lk"]), eng.device) for t in range(2)]
    engine.set_pbs_group(0)
    want = [ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, j, 3)) for j in jobs]
    assert engine.last_pbs_group() == 1
    assert not (want[0] == want[1]).all()
    torch.cuda.synchronize()
    engine.set_pbs_group(4)
    bad, seen, errors = [0, 0], [None, None, None], []

    def worker(t):
        try:
            stream = torch.cuda.Stream(device=eng.device)
            with torch.cuda.stream(stream):
                for _ in range(3):
                    got = ma.to_numpy(eng.programmable_bootstrap(K["bsk"], d_tv, jobs[t], 3))
                    bad[t] += int(not (got == want[t]).all())
            seen[t] = engine.last_pbs_group()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def bystander():
        seen[2] = engine.last_pbs_group()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    idle = threading.Thread(target=bystander)        # (started behind the callers: whatever they left behind is theirs alone)
    idle.start()
    idle.join()
    assert not errors, errors
    assert bad == [0, 0]
    assert seen == [4, 4, 0], seen
    assert engine.last_pbs_group() == 1
    for t in range(2):
        assert (want[t][4] == oracle.programmable_bootstrap(tv, ma.to_numpy(jobs[t])[4], K["bk_dft"], K["l"], K["Bg_bit"], 3, 0, 0)).all(), t


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
