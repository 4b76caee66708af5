"""Latency of pbs_team_kernel's run-time-gadget forms (N = 1024, l = 1 .. 4 with a gadget that has no compile-time instantiation): tools/gpu_latency_team.py [l] [Bg_bit]
(default 3 x 2^10: pbs_team_kernel<3, 0>; 4 8: pbs_team_kernel<4, 0>).  SET_1's other parameters; 1 and 64 bootstraps, ten launches each, outputs checked by phase."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mosfhet_amd as ma
from mosfhet_amd import host, engine

P = dict(ma.PARAMS_SET1)
P.update(l=int(sys.argv[1]) if len(sys.argv) > 1 else 3, Bg_bit=int(sys.argv[2]) if len(sys.argv) > 2 else 10)
host.seed(0x7EA3)
lk = host.LweKey(P['n'], P['lwe_sigma'])
rk = host.RlweKey(P['N'], 1, P['rlwe_sigma'])
eng = ma.Engine(0)
bsk = eng.load_bootstrap_key(host.gen_bootstrap_key(rk, lk, P['l'], P['Bg_bit']), 1, P['l'], P['Bg_bit'])
lut = np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64)
d_tv = ma.to_device(host.torus_packing(lut, 1, P['N'])[None], eng.device)
d_ct = ma.to_device(host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(64)], lk), eng.device)
sk = rk.extracted_lwe_key().s
engine.set_team_max_batch(1 << 30)
for B in (64, 1):
    out = eng.functional_bootstrap(bsk, d_tv, d_ct[:B], 4)
    torch.cuda.synchronize()
    err = np.abs((host.tlwe_phase(ma.to_numpy(out), sk) - lut[np.arange(B) % 4]).astype(np.int64).astype(np.float64)).max()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            eng.functional_bootstrap(bsk, d_tv, d_ct[:B], 4, out=out)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 10)
    print("team kernel l=%d Bg=2^%d, %2d bootstraps: %.3f ms per launch, max phase error 2^%.1f" % (P['l'], P['Bg_bit'], B, best, np.log2(err + 1)))
