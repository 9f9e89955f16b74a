#!/usr/bin/env python3
"""Victoria Park (configs[3]) update rate -- not the headline metric (bench.py), a measurement for DESIGN.md.
5000 particles, Victoria-Park-shaped maps (40 landmarks, 12 measurements per update); state re-seeded every step.
  python tools/vp_bench.py --batch B [--reps 3] [--particles 100] [--messages 900] [--capacity 384] [--only batch|handles|batch_dev]
      A sweep of B Victoria Park RB-PHD filters over the dataset extract (tests/golden/victoria_park_extract.npz, artificial clutter
      on): the filter batch (VPFilterBatch, rfsgpu_batch_vp_cycle_async) against the same B filters as plain handles stepped in turn,
      both through vp_driver.VictoriaParkBatchRun with the same realisations, alternating in this one invocation.  One line per
      repetition and route, then one JSON line: medians in seconds per sweep, runs (filters) per second, and the ratio.
  python tools/vp_bench.py --batch B --device-loop [...]
      Three routes, alternating: the host-stop batch, the device-loop batch (VictoriaParkBatchRun(device_loop=True): propagation, the
      resampling tail and the inheritance walk on the device, nothing read until the end) and the handles in turn under the device
      loop's realisations.  The JSON line adds batch_dev_s, batch_dev_runs_per_s, batch_dev_over_batch and batch_dev_over_handles."""
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package
pkg = load_package()
if os.environ.get("RFS_LIB"):
    pkg.engine.LIB = os.environ["RFS_LIB"]      # a tools/variant_bench.py --build variant
sc = pkg.scenarios


def batch_sweep(nF):
    """Per filter: parameter set (Pd table / expected clutter of the sweep), seed, artificial-clutter rate."""
    Ps, seeds, clutter = [], [], []
    for b in range(nF):
        P = dict(sc.VP_PARAMS)
        P["expected_clutter"] = [6.0, 3.0, 9.0, 12.0][b % 4]
        P["pd_table"] = [[0.0, 0.05, 0.35, 0.76, 0.89, 0.90], [0.0, 0.1, 0.5, 0.8, 0.95], [0.0, 0.03, 0.3, 0.7, 0.85, 0.88]][b % 3]
        Ps.append(P)
        seeds.append(100 + b)
        clutter.append([3.0, 1.0, 5.0, 2.0][(b // 4) % 4])
    return Ps, seeds, clutter


def batch_one_run(route, nF, n, data, messages, cap, device_loop=False):
    Ps, seeds, clutter = batch_sweep(nF)
    if route in ("batch", "batch_dev"):
        target = pkg.VPFilterBatch(nF, n, gm_capacity=cap)
        for b in range(nF):
            sc.apply_vp_batch_params(target, b, Ps[b])
        target.synchronize()
        owned = [target]
    else:
        target = [pkg.RBPHDFilter(n, gm_capacity=cap, model=pkg.capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b, h in enumerate(target):
            sc.apply_vp_params(h, Ps[b], np.full(361, 70.0))
            h.synchronize()
        owned = target
    t0 = time.perf_counter()
    dev = route == "batch_dev" or (route == "handles" and device_loop)
    r = pkg.vp_driver.VictoriaParkBatchRun(target, data, Ps, seeds, added_clutter=clutter, device_loop=dev).run(n_messages=messages)
    dt = time.perf_counter() - t0
    info = (int(r.n_lidar), int(r.n_resamples.sum()), float(np.mean(np.concatenate([h.gm_sizes() for h in owned]))))
    for h in owned:
        h.close()
    return dt, info


def batch_main():
    import argparse
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--particles", type=int, default=100)
    ap.add_argument("--messages", type=int, default=900)
    ap.add_argument("--only", choices=["batch", "handles", "batch_dev"], default=None)
    ap.add_argument("--capacity", type=int, default=384)      # (192 is transiently short under the heaviest clutter of the sweep)
    ap.add_argument("--device-loop", action="store_true")
    a = ap.parse_args()
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    routes = [a.only] if a.only else (["handles", "batch", "batch_dev"] if a.device_loop else ["handles", "batch"])
    times = {r: [] for r in routes}
    for rep in range(a.reps + 1):                     # (the first repetition warms up: code objects, allocations)
        for route in routes:
            dt, info = batch_one_run(route, a.batch, a.particles, data, a.messages, a.capacity, a.device_loop)
            if rep:
                times[route].append(dt)
            print("  %-9s rep %d%s: %.4f s for %d filters (%d lidar updates, %d resamplings, mean map size %.1f)" %
                  ((route, rep, "" if rep else " (warm-up)", dt, a.batch) + info), flush=True)
    out = dict(tool="vp_bench", filters=a.batch, particles=a.particles, messages=a.messages, reps=a.reps, device_loop=bool(a.device_loop))
    for r in routes:
        med = float(np.median(times[r]))
        out[r + "_s"] = med
        out[r + "_spread_s"] = float(np.max(times[r]) - np.min(times[r]))
        out[r + "_runs_per_s"] = a.batch / med
    if "batch" in routes and "handles" in routes:
        out["batch_over_handles"] = out["batch_runs_per_s"] / out["handles_runs_per_s"]
    if "batch_dev" in routes and "batch" in routes:
        out["batch_dev_over_batch"] = out["batch_dev_runs_per_s"] / out["batch_runs_per_s"]
    if "batch_dev" in routes and "handles" in routes:
        out["batch_dev_over_handles"] = out["batch_dev_runs_per_s"] / out["handles_runs_per_s"]
    print(json.dumps(out))


if "--batch" in sys.argv:
    batch_main()
    sys.exit(0)
N, NM, NZ = [int(os.environ.get(k, d)) for k, d in (("VP_N", 5000), ("VP_NM", 40), ("VP_NZ", 12))]
scen = sc.make_vp_scenario(N, NM, NZ, seed=4321, scan="ragged")
f = pkg.RBPHDFilter(N, gm_capacity=int(os.environ.get("VP_CAP", 192)), model=pkg.capi.MODEL_VICTORIAPARK_3D)
sc.load_scenario(f, scen)
f.save_state()
for _ in range(5):
    f.restore_state(); f.update(scen["Z"])
S = int(os.environ.get("VP_STEPS", 100))
t0 = time.perf_counter()
acc = np.zeros(4)
for _ in range(S):
    f.restore_state()
    f.update(scen["Z"])
    acc += np.array(f.last_kernel_ns(), dtype=np.float64)
dt = time.perf_counter() - t0
ns = acc / S      # mean over the timed steps
print("VP RB-PHD update, %d particles x %d landmarks x %d measurements: %.4f ms/update (%.1f updates/s); kernels us: update_map %.1f, weighting %.1f, merge+prune %.1f" %
      (N, NM, NZ, dt / S * 1e3, S / dt, ns[0] / 1e3, ns[1] / 1e3, ns[2] / 1e3))
if "--cpu" in sys.argv:
    import importlib
    ob = importlib.import_module("oracle.binding")
    n = 512
    sub = dict(scen); sub.update(n=n, poses=scen["poses"][:n], w=scen["w"][:n], mean=scen["mean"][:n], cov=scen["cov"][:n], particle_w=scen["particle_w"][:n])
    ow = ob.OracleFilter(n, model=pkg.capi.MODEL_VICTORIAPARK_3D)                     # warm-up instance: the first OpenMP region pays for starting the thread team
    sc.load_scenario(ow, sub)
    ow.update(scen["Z"])
    o = ob.OracleFilter(n, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    sc.load_scenario(o, sub)
    t0 = time.perf_counter()
    o.update(scen["Z"])
    dt = time.perf_counter() - t0
    print("oracle (OpenMP, all host threads): %.1f ms for %d particles -> %.2f updates/s at %d particles" % (dt * 1e3, n, 1.0 / (dt * N / n), N))
