"""Same-box A/B of the product orders of a bootstrap key (mosfhet_hip_bsk_set_product_order) and of this build against another build of the library: lvl2
programmable_bootstrap (N = 2048, l = 4, Bg = 2^9, n = 632) at batches of 1 ... 4096 for AUTO, REFERENCE and BY_COMPONENT keys.  Every setting runs in child processes of
its own (a library is loaded once per process; environment switches are read once), settings alternate over AB_ROUNDS rounds (default 2), so the spread between the
runs of ONE setting stands next to the gaps between settings.  Device events around launches that end in a synchronise, a warm-up launch first, at least a second of timed
work per figure.  A digest of the outputs per order: settings that must agree bit for bit (the same order on two builds) show the same digest.

    python tools/product_order_ab.py "name[:lib=PATH][,VAR=val ...]" ...      (no lib: this tree's library; a library without the property runs AUTO only)
    python tools/product_order_ab.py this parent:lib=/path/to/parent/libmosfhet_hip.so "one-CU rounds:AB_PARKING=0" > profiles/product_order_ab.txt
                                      (AB_PARKING=0: mosfhet_hip_set_bycomp_parking(0), the one-CU by-component kernel in rounds for large batches: the yardstick)
"""
import os
import subprocess
import sys

PROBE = r"""
import os, sys, hashlib, math, numpy as np, torch
import mosfhet_amd as ma
from mosfhet_amd import host, engine
if os.environ.get("AB_LIB"):
    engine.lib_path = lambda: os.environ["AB_LIB"]
P = dict(ma.PARAMS_LVL2)
host.seed(11)
lk = host.LweKey(P['n'], P['lwe_sigma']); rk = host.RlweKey(P['N'], 1, P['rlwe_sigma'])
eng = ma.Engine(0)
ma.Engine.set_keygen_secret(bytes(range(32)))          # the device generator's noise key: the same key in every child process, so digests compare
key = eng.generate_bootstrap_key(rk.s[0], lk.s, P['l'], P['Bg_bit'], P['rlwe_sigma'], 1)
lut = np.array([1 << 60, 5 << 60, 9 << 60, 13 << 60], dtype=np.uint64)
d_tv = ma.to_device(host.torus_packing(lut, 1, P['N'])[None], eng.device)
cts = host.tlwe_samples([host.double2torus((b % 4) / 8.0) for b in range(128)], lk)
d_all = ma.to_device(cts[np.arange(4096) % 128], eng.device)
if os.environ.get("AB_PARKING") == "0":
    engine.set_bycomp_parking(0)          # the yardstick: the one-CU by-component kernel in residency rounds for large batches
orders = ["auto", "reference", "by_component"] if hasattr(engine.lib(), "mosfhet_hip_bsk_set_product_order") else ["auto"]
for order in orders:
    if order != "auto":
        key.set_product_order(order)
    h = hashlib.sha256()
    res = []
    for B in (1, 128, 256, 512, 1024, 4096):
        d_ct = d_all[:B]
        out = eng.programmable_bootstrap(key, d_tv, d_ct, 3)          # warm-up
        torch.cuda.synchronize()
        h.update(ma.to_numpy(out).tobytes())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); eng.programmable_bootstrap(key, d_tv, d_ct, 3, out=out); e1.record(); torch.cuda.synchronize()
        reps = max(4, int(math.ceil(1000.0 / max(e0.elapsed_time(e1), 0.05))))
        e0.record()
        for _ in range(reps):
            eng.programmable_bootstrap(key, d_tv, d_ct, 3, out=out)
        e1.record(); torch.cuda.synchronize()
        res.append("%d: %.3f" % (B, e0.elapsed_time(e1) / reps))
    print("RESULT %-12s" % order, "  ".join(res), " digest", h.hexdigest()[:12], flush=True)
"""

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    settings = []
    for spec in sys.argv[1:] or ["this"]:
        name, _, env = spec.partition(":")
        kv = dict(x.split("=", 1) for x in env.split(",") if x)
        lib = kv.pop("lib", "")
        settings.append((name, dict(kv, AB_LIB=lib)))
    print("ms per launch of lvl2 programmable_bootstrap, batch: ms   (settings: %s)" % ", ".join(
        "%s = %s%s" % (name, "library " + os.path.basename(os.path.dirname(env["AB_LIB"])) + "/" + os.path.basename(env["AB_LIB"]) if env["AB_LIB"] else "this tree's library",
                       "".join(" %s=%s" % kv for kv in env.items() if kv[0] != "AB_LIB")) for name, env in settings))
    for rnd in range(int(os.environ.get("AB_ROUNDS", "2"))):
        for name, env in settings:
            e = dict(os.environ, **env)
            e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
            r = subprocess.run([sys.executable, "-c", PROBE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=e, cwd=root, timeout=900)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
            if r.returncode != 0 or not lines:
                print("%-14s FAILED (%d): %s" % (name, r.returncode, r.stdout[-500:]), flush=True)
                sys.exit(1)      # nothing more is started on the GPU after a failure
            for ln in lines:
                print("%-14s %s" % (name, ln[7:]), flush=True)
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_table
    print("code-object figures of the by-component kernels (one-CU form: split kernels with `true`; throughput form: pbs_kernel with `true`) and their siblings:")
    for r in sorted(kernel_table.table(), key=lambda r: r["name"]):
        if "split_kernel" in r["name"] or (r["name"].startswith("pbs_kernel<Fft2048T<false, false>") and r["name"].split(",")[2].strip() in ("2", "4", "6")):
            print("  %-66s vgpr %3d  agpr %3d  sgpr %3d  lds %5d  scratch %d" % (r["name"], r["vgpr"], r["agpr"], r["sgpr"], r["lds"], r["scratch"]))
