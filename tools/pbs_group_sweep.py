"""From which batch size on SET_1's throughput bootstrap kernel gains from four ciphertexts per workgroup (capi.hip: pbs_group_takes): kernel time with one ciphertext
per workgroup and with four forced, interleaved on one GPU, at batch sizes around one residency round of the device.

    python tools/pbs_group_sweep.py [counts, comma separated] [rounds]      (GPU box; copy the output into profiles/)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mosfhet_amd as ma
from mosfhet_amd import engine, host

counts = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "256,512,1024,1536,2048,2560,3072,4096,6144,8192").split(",")]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
P = dict(ma.PARAMS_SET1)
host.seed(0x4D4F5346)
lk = host.LweKey(P["n"], P["lwe_sigma"])
rk = host.RlweKey(P["N"], 1, P["rlwe_sigma"])
eng = ma.Engine(0)
bsk = eng.load_bootstrap_key(host.gen_bootstrap_key(rk, lk, P["l"], P["Bg_bit"]), 1, P["l"], P["Bg_bit"])
tv = host.torus_packing(np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64), 1, P["N"])
cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(max(counts))], lk)
d_tv, d_all = ma.to_device(tv[None], eng.device), ma.to_device(cts, eng.device)
engine.set_team_max_batch(0)   # the throughput kernel at every size
print("%6s %12s %12s %8s   (median of %d rounds of 3 launches, ms per launch; same bits: %s)" % ("count", "1 per wg", "4 per wg", "change", rounds, "checked"))
for B in counts:
    d_ct = d_all[:B]
    t, outs = {0: [], 4: []}, {}
    for r in range(rounds):
        for g in (0, 4):
            engine.set_pbs_group(g)
            out = eng.empty(B, P["N"] + 1)
            t[g].append(eng.time_programmable_bootstrap(bsk, d_tv, d_ct, 3, 3, out=out))
            assert engine.last_pbs_group() == (4 if g else 1)
            if r == 0:
                outs[g] = ma.to_numpy(out)
    assert (outs[0] == outs[4]).all(), B
    m = {g: sorted(v)[len(v) // 2] for g, v in t.items()}
    print("%6d %12.3f %12.3f %+7.1f %%" % (B, m[0], m[4], 100 * (m[4] / m[0] - 1)))
engine.set_pbs_group(-1)
engine.set_team_max_batch(512)
