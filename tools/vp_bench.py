#!/usr/bin/env python3
"""Victoria Park (configs[3]) update rate -- not the headline metric (bench.py), a measurement for DESIGN.md.
5000 particles, Victoria-Park-shaped maps (40 landmarks, 12 measurements per update); state re-seeded every step.
  python tools/vp_bench.py --batch B [--reps 3] [--particles 100] [--messages 900] [--capacity 384] [--only batch|handles|batch_dev]
      A sweep of B Victoria Park RB-PHD filters over the dataset extract (tests/golden/victoria_park_extract.npz, artificial clutter
      on): the filter batch (VPFilterBatch, rfsgpu_batch_vp_cycle_async) against the same B filters as plain handles stepped in turn,
      both through vp_driver.VictoriaParkBatchRun with the same realisations, alternating in this one invocation.  One line per
      repetition and route, then one JSON line: medians in seconds per sweep, runs (filters) per second, and the ratio.
  python tools/vp_bench.py --batch B --fastslam [--device-loop] [...]
      The FastSLAM half of the sweep: a VPFastSLAMBatch (rfsgpu_batch_vp_fastslam_cycle_async) against B FastSLAM handles stepped in
      turn, through VictoriaParkBatchRun(filter="fastslam"); the routes and the JSON fields of the RB-PHD forms.
  python tools/vp_bench.py --batch B --mhfastslam --device-loop [...]
      The multi-hypothesis third of the sweep (cfg/mhfastslam_VictoriaPark_artificialClutter.xml: 3 hypotheses, window 3.0, candidate
      count threshold 4, minTimesteps 2, minMeasurements 15): a VPMHFastSLAMBatch (rfsgpu_batch_vp_fastslam_mh_cycle_async) against B
      FastSLAM handles on rfsgpu_fastslam_cycle_full_async stepped in turn, through VictoriaParkBatchRun(filter="mhfastslam"), which
      has the device route only: the routes are handles and batch_dev.
  python tools/vp_bench.py --batch B --device-loop [...]
      Three routes, alternating: the host-stop batch, the device-loop batch (VictoriaParkBatchRun(device_loop=True): propagation, the
      resampling tail and the inheritance walk on the device, nothing read until the end) and the handles in turn under the device
      loop's realisations.  The JSON line adds batch_dev_s, batch_dev_runs_per_s, batch_dev_over_batch and batch_dev_over_handles.
  python tools/vp_bench.py --batch B --device-loop --log [--log-dir DIR] [--no-log-particles] [...]
      What recording the sweep's per-update estimates costs.  Three routes of the device-loop batch, alternating: unlogged; logged on
      the device (VictoriaParkBatchRun(log_estimates=True): rfsgpu_batch_vp_serve_estimates, one row per lidar message behind its
      resampling step, nothing read until the end -- the one read, estimates(), is timed apart as log_read_s); and the per-update
      getter route (get_weights + get_poses + the best slot's map per filter and lidar message, each of which synchronises).  The
      JSON line holds the medians, the log's size in MiB and the ratios.  --log-dir: the last logged repetition's files
      (write_vp_batch_logs: DIR/filter_%03d/particlePose.dat and landmarkEst.dat), written outside the timed part."""
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


def fastslam_sweep_config(f, P):
    """The FastSLAM half of the sweep (cfg/fastslam_VictoriaPark_artificialClutter.xml): candidate lists with a count threshold of 4."""
    cfg = f.default_fastslam_config()
    cfg.landmarkCandidateMeasurementCountThreshold = 4
    cfg.landmarkCandidateMeasurementCheckThreshold = 6
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.minUpdatesBeforeResample = int(P["min_updates"])
    cfg.minMeasurementsBeforeResample = int(P["min_measurements"])
    return cfg


MH_HYPOTHESES = 3


def mh_sweep_config(cfg, P, n):
    """The multi-hypothesis third of the sweep: fastslam_sweep_config's lists, three hypotheses inside a window of 3.0."""
    cfg.maxNDataAssocHypotheses = MH_HYPOTHESES
    cfg.maxDataAssocLogLikelihoodDiff = 3.0
    cfg.nParticlesMax = 3 * n
    cfg.landmarkCandidateMeasurementCountThreshold = 4
    cfg.landmarkCandidateMeasurementCheckThreshold = 6
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    return cfg


def mh_one_run(route, nF, n, data, messages, cap):
    Ps, seeds, clutter = batch_sweep(nF)
    for P in Ps:
        P["min_updates"], P["min_measurements"] = 2, 15
    if route == "batch_dev":
        target = pkg.VPMHFastSLAMBatch(nF, n, gm_capacity=cap, max_hypotheses=MH_HYPOTHESES)
        for b in range(nF):
            sc.apply_vp_batch_params(target, b, Ps[b])
            target.configure_fastslam(b, mh_sweep_config(target.fs_configs[b], Ps[b], n))
        target.synchronize()
        owned = [target]
        live = lambda: [np.asarray(target.gm_sizes())[target.block(b, c)] for b, c in enumerate(target.live_counts())]
    else:
        stride = min(2048, 3 * n * MH_HYPOTHESES)
        target = [pkg.FastSLAM(n, gm_capacity=cap, max_hypotheses=MH_HYPOTHESES, device_cycle=True, max_particles=stride,
                               model=pkg.capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b, h in enumerate(target):
            sc.apply_vp_params(h, Ps[b], np.full(361, 70.0))
            h.config = h.get_filter_config()
            mh_sweep_config(h.fs_config, Ps[b], n)
            h.synchronize()
        owned = target
        live = lambda: [h.gm_sizes() for h in target]
    t0 = time.perf_counter()
    r = pkg.vp_driver.VictoriaParkBatchRun(target, data, Ps, seeds, added_clutter=clutter, device_loop=True, filter="mhfastslam").run(n_messages=messages)
    dt = time.perf_counter() - t0
    info = (int(r.n_lidar), -1, float(np.mean(np.concatenate(live()))))      # (the resamplings are counted on the device and not read)
    for h in owned:
        h.close()
    return dt, info


def batch_one_run(route, nF, n, data, messages, cap, device_loop=False, fastslam=False):
    Ps, seeds, clutter = batch_sweep(nF)
    if route in ("batch", "batch_dev"):
        target = (pkg.VPFastSLAMBatch if fastslam else pkg.VPFilterBatch)(nF, n, gm_capacity=cap)
        for b in range(nF):
            sc.apply_vp_batch_params(target, b, Ps[b])
            if fastslam:
                target.configure_fastslam(b, fastslam_sweep_config(target, Ps[b]))
        target.synchronize()
        owned = [target]
    else:
        target = [(pkg.FastSLAM if fastslam else pkg.RBPHDFilter)(n, gm_capacity=cap, model=pkg.capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b, h in enumerate(target):
            sc.apply_vp_params(h, Ps[b], np.full(361, 70.0))
            if fastslam:
                h.set_fastslam_config(fastslam_sweep_config(h, Ps[b]))
            h.synchronize()
        owned = target
    t0 = time.perf_counter()
    dev = route == "batch_dev" or (route == "handles" and device_loop)
    r = pkg.vp_driver.VictoriaParkBatchRun(target, data, Ps, seeds, added_clutter=clutter, device_loop=dev,
                                           filter="fastslam" if fastslam else "rbphd").run(n_messages=messages)
    dt = time.perf_counter() - t0
    info = (int(r.n_lidar), int(r.n_resamples.sum()), float(np.mean(np.concatenate([h.gm_sizes() for h in owned]))))
    for h in owned:
        h.close()
    return dt, info


def log_one_run(route, nF, n, data, messages, cap, particles=True, log_dir=None):
    """One device-loop sweep of the batch: route 'plain' (no log), 'logged' (the device-side log) or 'getters' (the per-update getters).
    Returns (seconds of the run, seconds of the one read or 0, info, log bytes)."""
    drv = pkg.vp_driver
    Ps, seeds, clutter = batch_sweep(nF)
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=cap)
    for b in range(nF):
        sc.apply_vp_batch_params(batch, b, Ps[b])
    batch.synchronize()
    kept = []

    class GetterRun(drv.VictoriaParkBatchRun):
        """What a sweep without the device-side log has to do per lidar message to keep the two files' content."""

        def _log_row(self, t):
            w, x = batch.get_weights(), batch.get_poses()
            best = [b * n + int(np.argmax(w[b * n:(b + 1) * n])) for b in range(nF)]
            kept.append((t, w, x, [batch.export_gm(s) for s in best]))

    cls = GetterRun if route == "getters" else drv.VictoriaParkBatchRun
    t0 = time.perf_counter()
    r = cls(batch, data, Ps, seeds, added_clutter=clutter, device_loop=True, log_estimates=(route == "logged"), log_particles=particles).run(n_messages=messages)
    dt = time.perf_counter() - t0
    t_read, nbytes = 0.0, 0
    if route == "logged":
        t1 = time.perf_counter()
        est = r.estimates()
        t_read = time.perf_counter() - t1
        nbytes = sum(a.nbytes for a in est if a is not None)
        if log_dir:
            drv.write_vp_batch_logs(log_dir, est)
    info = (int(r.n_lidar), int(np.sum(r.n_resamples)), float(np.mean(batch.gm_sizes())))
    batch.close()
    return dt, t_read, info, nbytes


def log_main():
    import argparse
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--particles", type=int, default=100)
    ap.add_argument("--messages", type=int, default=900)
    ap.add_argument("--capacity", type=int, default=384)
    ap.add_argument("--device-loop", action="store_true", required=True)
    ap.add_argument("--log", action="store_true")
    ap.add_argument("--log-dir", default=None)
    ap.add_argument("--no-log-particles", action="store_true")
    ap.add_argument("--only", choices=["plain", "logged", "getters"], default=None)
    a = ap.parse_args()
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    routes = [a.only] if a.only else ["plain", "logged", "getters"]
    times, reads, nbytes = {r: [] for r in routes}, [], 0
    for rep in range(a.reps + 1):                     # (the first repetition warms up: code objects, allocations)
        for route in routes:
            dt, t_read, info, nb = log_one_run(route, a.batch, a.particles, data, a.messages, a.capacity, not a.no_log_particles,
                                               a.log_dir if rep == a.reps else None)
            if rep:
                times[route].append(dt)
                if route == "logged":
                    reads.append(t_read)
            nbytes = max(nbytes, nb)
            print("  %-8s rep %d%s: %.4f s%s for %d filters (%d lidar updates, %d resamplings, mean map size %.1f)" %
                  ((route, rep, "" if rep else " (warm-up)", dt, (" + %.4f s read" % t_read) if route == "logged" else "", a.batch) + info), flush=True)
    out = dict(tool="vp_bench", mode="log", filters=a.batch, particles=a.particles, messages=a.messages, reps=a.reps, log_particles=not a.no_log_particles)
    for r in routes:
        out[r + "_s"] = float(np.median(times[r]))
        out[r + "_spread_s"] = float(np.max(times[r]) - np.min(times[r]))
    if "logged" in routes:
        out["log_read_s"] = float(np.median(reads))
        out["logged_with_read_s"] = out["logged_s"] + out["log_read_s"]
        out["log_mib"] = nbytes / 2.0 ** 20
    if "logged" in routes and "plain" in routes:
        out["logged_with_read_over_plain"] = out["logged_with_read_s"] / out["plain_s"]
    if "logged" in routes and "getters" in routes:
        out["getters_over_logged_with_read"] = out["getters_s"] / out["logged_with_read_s"]
    print(json.dumps(out))


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
    ap.add_argument("--fastslam", action="store_true")
    ap.add_argument("--mhfastslam", action="store_true")
    a = ap.parse_args()
    if a.mhfastslam and not a.device_loop:
        ap.error("--mhfastslam runs on the device route only: add --device-loop")
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    routes = [a.only] if a.only else (["handles", "batch_dev"] if a.mhfastslam else (["handles", "batch", "batch_dev"] if a.device_loop else ["handles", "batch"]))
    times = {r: [] for r in routes}
    for rep in range(a.reps + 1):                     # (the first repetition warms up: code objects, allocations)
        for route in routes:
            if a.mhfastslam:
                dt, info = mh_one_run(route, a.batch, a.particles, data, a.messages, a.capacity)
            else:
                dt, info = batch_one_run(route, a.batch, a.particles, data, a.messages, a.capacity, a.device_loop, a.fastslam)
            if rep:
                times[route].append(dt)
            print("  %-9s rep %d%s: %.4f s for %d filters (%d lidar updates, %d resamplings, mean map size %.1f)" %
                  ((route, rep, "" if rep else " (warm-up)", dt, a.batch) + info), flush=True)
    out = dict(tool="vp_bench", filters=a.batch, particles=a.particles, messages=a.messages, reps=a.reps, device_loop=bool(a.device_loop))
    if a.fastslam or a.mhfastslam:
        out["filter"] = "mhfastslam" if a.mhfastslam else "fastslam"
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
    log_main() if "--log" in sys.argv else batch_main()
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
