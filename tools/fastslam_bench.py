#!/usr/bin/env python3
"""FastSLAM 1.0 update rate -- not the headline metric (bench.py), a measurement for DESIGN.md.
2000 particles, 200 landmarks over a 25 m disc, 30 measurements per update; state re-seeded every step.
  python tools/fastslam_bench.py [--cpu]    (--cpu also times the oracle on the host cores)
  python tools/fastslam_bench.py --mh-device-cycle
      MH-FastSLAM cycles per second over one simulator trajectory, timed both ways in this one invocation: the host-planned route
      (rfsgpu_fastslam_update + the numpy resampling of FastSLAM.update_and_resample) and rfsgpu_fastslam_cycle_async
      (FastSLAM(device_cycle=True)).  FS_N particles (200), FS_HYP hypotheses (4), FS_STEPS steps (100), median of FS_REPS (3).
  python tools/fastslam_bench.py --vp-cycle [--rbphd]
      The Victoria Park extract through vp_driver.VictoriaParkRun on three routes that alternate in this one invocation -- the host-stop
      route, the device cycle read after every lidar message, the device cycle with nothing read until the end -- medians of FS_REPS;
      FastSLAM with 1 and 3 hypotheses, or with --rbphd the RB-PHD filter (rfsgpu_rbphd_cycle_async).  FS_N particles (100).
  python tools/fastslam_bench.py --vp-cycle --log [--rbphd]
      The logging column: the device cycle with nothing read until the end, the same with the device-side estimate log (one row
      behind every lidar update, vp_driver's log_estimates; the one read at the end is timed apart), and the same with the per-update
      getter route (weights, poses and the best particle's map read after every lidar update, which resolves the pending cycle)."""
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package
pkg = load_package()
sc = pkg.scenarios


def mh_route_times(pkg, device_cycle, n, hyp, steps, reps, quiet=False):
    """Seconds per cycle (one per repetition) of `steps` MH-FastSLAM cycles of the 2-D simulator's configuration, poses at the ground
    truth (the driver's first 100 steps): set_poses, predict, update with its resampling.  device_cycle is ignored by a package that
    does not know it (False must be passed there)."""
    drv = pkg.sim2d_driver
    P = dict(drv.C1_FASTSLAM_SIM, max_hypotheses=hyp, kmax=3 * steps)     # (kmax spaces the generator's landmarks: one per 6 steps)
    data = drv.generate(P, traj_seed=3, kmax=steps + 1)
    draws = np.random.default_rng(8).random(steps + 1)
    out = []
    for rep in range(reps + 1):                       # (the first repetition warms up: code objects, allocations)
        kw = dict(device_cycle=True) if device_cycle else {}
        f = pkg.FastSLAM(n, gm_capacity=64, max_hypotheses=hyp, n_particles_max=2048 // hyp, **kw)
        drv.configure(f, P)
        f.config = f.get_filter_config()
        f.fs_config = drv.fastslam_config(f, P)
        f.fs_config.nParticlesMax = 2048 // hyp
        f.setEffectiveParticleCountThreshold(P["eff_n"])
        f.synchronize()
        fired = grown = 0
        t0 = time.perf_counter()
        for k in range(1, steps + 1):
            f.set_poses(np.tile(data["gt"][k], (f.n, 1)), np.zeros((3, 3)))
            f.predict_map()
            fired += bool(f.update_and_resample(data["Z"][k], u01_fn=lambda: float(draws[k])))
            grown = max(grown, len(f.parents))
        f.synchronize()
        dt = (time.perf_counter() - t0) / steps
        sizes = int(np.asarray(f.gm_sizes()).mean())
        f.close()
        if rep:
            out.append(dt)
        if not quiet:
            print("  %s rep %d: %.4f ms/cycle, %d resamplings, largest grown set %d, mean map size %d%s" %
                  ("device cycle" if device_cycle else "host-planned", rep, dt * 1e3, fired, grown, sizes, "" if rep else "  (warm-up)"))
    return out


class GetterLogRun(pkg.vp_driver.VictoriaParkRun):
    """The per-update getter route of a logged run: after every lidar update the weights, the poses and the map of the highest-weight
    particle come to the host, as the C++ driver's -o route reads them."""
    rows = None

    def _log_row(self, t):
        if self.rows is None:
            self.rows = []
        w, x = self.f.get_weights(), self.f.get_poses()
        best = int(np.argmax(w)) if (w > 0).any() else 0
        self.rows.append((t, x, w, best, self.f.export_gm(best)))


def log_setup(pkg, log, opts):
    """The run class and options of a logged run: log None, "device" (the device-side estimate log) or "getter"."""
    if log == "device":
        opts["log_estimates"] = True
    return GetterLogRun if log == "getter" else pkg.vp_driver.VictoriaParkRun


def log_read(run, log):
    """Seconds of the one read at the end of a run with the device log (0 on the other routes)."""
    if log != "device":
        return 0.0
    t0 = time.perf_counter()
    hdr = run.estimates()[0]
    dt = time.perf_counter() - t0
    assert hdr.shape[0] > run.n_lidar and (hdr["status"] == 0).all()
    return dt


def vp_cycle_run(pkg, route, hyp, n, messages, log=None):
    """Seconds for one run of `messages` messages of the Victoria Park extract through vp_driver.VictoriaParkRun: the values of the
    reference's fastslam_VictoriaPark.xml / mhfastslam_VictoriaPark.xml (100 particles, candidate threshold 4, 1 or 3 hypotheses),
    poses propagated on the device on every route.  route: "host" (rfsgpu_fastslam_update + the host's resampleWithMapCopy),
    "sync" (rfsgpu_fastslam_cycle_full_async, results read after every lidar message) or "queue" (nothing read until the end)."""
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    P = dict(sc.VP_PARAMS)
    n_max = 3 * n if hyp > 1 else n
    f = pkg.RBPHDFilter(n, gm_capacity=192, model=pkg.capi.MODEL_VICTORIAPARK_3D, max_particles=n_max * hyp)
    sc.apply_vp_params(f, P, np.full(361, 70.0))
    cfg = f.default_fastslam_config()
    cfg.minLogMeasurementLikelihood = -15.0
    cfg.mapExistencePruneThreshold = -5.0
    cfg.landmarkCandidateMeasurementCountThreshold = 4
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementCheckThreshold = 5
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.maxNDataAssocHypotheses = hyp
    cfg.maxDataAssocLogLikelihoodDiff = 3.0
    f.set_fastslam_config(cfg)
    opts = dict(device_motion=True, draw_every_update=True) if route == "host" else dict(device_cycle=True, sync_every_update=route == "sync")      # ("queue", and "log" of the logging column: nothing read)
    cls = log_setup(pkg, log, opts)
    f.synchronize()
    t0 = time.perf_counter()
    run = cls(f, data, P, seed=5, filter="fastslam", max_hypotheses=hyp, n_particles_max=n_max, **opts).run(n_messages=messages)
    dt = time.perf_counter() - t0
    out = (dt, run.n_lidar, run.n_resamples, run.n, float(np.asarray(f.gm_sizes()).mean())) + ((log_read(run, log),) if log is not None or route == "log" else ())
    f.close()
    return out


def vp_rbphd_run(pkg, route, n, messages, log=None):
    """The same run around the RB-PHD filter (the XML's values, scenarios.VP_PARAMS), poses propagated on the device on every route.
    route: "host" (the update, then the host's gate and resampling), "sync" (rfsgpu_rbphd_cycle_async, results read after every lidar
    message) or "queue" (nothing read until the end)."""
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    P = dict(sc.VP_PARAMS)
    f = pkg.RBPHDFilter(n, gm_capacity=192, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    sc.apply_vp_params(f, P, np.full(361, 70.0))
    opts = dict(device_motion=True, draw_every_update=True) if route == "host" else dict(device_cycle=True, sync_every_update=route == "sync")      # ("queue", and "log" of the logging column: nothing read)
    cls = log_setup(pkg, log, opts)
    f.synchronize()
    t0 = time.perf_counter()
    run = cls(f, data, P, seed=5, filter="rbphd", **opts).run(n_messages=messages)
    dt = time.perf_counter() - t0
    out = (dt, run.n_lidar, run.n_resamples, run.n, float(np.asarray(f.gm_sizes()).mean())) + ((log_read(run, log),) if log is not None or route == "log" else ())
    f.close()
    return out


if "--vp-cycle" in sys.argv and "--log" in sys.argv:
    n, messages, reps = [int(os.environ.get(k, d)) for k, d in (("FS_N", 100), ("FS_MESSAGES", 900), ("FS_REPS", 3))]
    kinds = [("rbphd", 1)] if "--rbphd" in sys.argv else [("fastslam", h) for h in ([int(os.environ["FS_HYP"])] if "FS_HYP" in os.environ else [1, 3])]
    for kind, hyp in kinds:
        print("Victoria Park extract, %s, %d hypothes%s, %d messages, %d particles, %d repetitions (the logging routes alternate; the first round warms up)" %
              (kind, hyp, "is" if hyp == 1 else "es", messages, n, reps))
        times = {None: [], "device": [], "getter": []}
        reads = []
        for rep in range(reps + 1):
            for log in (None, "device", "getter"):
                r = vp_rbphd_run(pkg, "log", n, messages, log=log) if kind == "rbphd" else vp_cycle_run(pkg, "log", hyp, n, messages, log=log)
                if rep:
                    times[log].append(r[0])
                    if log == "device":
                        reads.append(r[5])
                print("  rep %d %-7s: %.4f s/run%s, %d lidar updates, %d resamplings, final count %d%s" %
                      (rep, log or "no log", r[0], " + %.4f s for the one read" % r[5] if log == "device" else "", r[1], r[2], r[3], "" if rep else "  (warm-up)"))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("%s hyp %d medians: device cycle %.4f s, with the device log %.4f s (%.3fx) + %.4f s read at the end, with per-update getters %.4f s (%.3fx)" %
              (kind, hyp, med[None], med["device"], med["device"] / med[None], float(np.median(reads)), med["getter"], med["getter"] / med[None]))
    sys.exit(0)

if "--vp-cycle" in sys.argv and "--rbphd" in sys.argv:
    n, messages, reps = [int(os.environ.get(k, d)) for k, d in (("FS_N", 100), ("FS_MESSAGES", 900), ("FS_REPS", 3))]
    print("Victoria Park extract, RB-PHD, %d messages, %d particles, %d repetitions (routes alternate; the first round warms up)" % (messages, n, reps))
    times = {"host": [], "sync": [], "queue": []}
    for rep in range(reps + 1):
        for route in ("host", "sync", "queue"):
            dt, nl, nr, nn, size = vp_rbphd_run(pkg, route, n, messages)
            if rep:
                times[route].append(dt)
            print("  rep %d %-5s: %.4f s/run, %d lidar updates, %d resamplings, %d particles, mean map size %.1f%s" %
                  (rep, route, dt, nl, nr, nn, size, "" if rep else "  (warm-up)"))
    med = {k: float(np.median(v)) for k, v in times.items()}
    print("rbphd medians: host-stop %.4f s, cycle + sync per update %.4f s (%.2fx), cycle queued %.4f s (%.2fx)" %
          (med["host"], med["sync"], med["host"] / med["sync"], med["queue"], med["host"] / med["queue"]))
    sys.exit(0)

if "--vp-cycle" in sys.argv:
    n, messages, reps = [int(os.environ.get(k, d)) for k, d in (("FS_N", 100), ("FS_MESSAGES", 900), ("FS_REPS", 3))]
    for hyp in (1, 3):
        print("Victoria Park extract, %d messages, %d particles, %d hypothes%s, %d repetitions (routes alternate; the first round warms up)" %
              (messages, n, hyp, "is" if hyp == 1 else "es", reps))
        times = {"host": [], "sync": [], "queue": []}
        for rep in range(reps + 1):
            for route in ("host", "sync", "queue"):
                dt, nl, nr, nn, size = vp_cycle_run(pkg, route, hyp, n, messages)
                if rep:
                    times[route].append(dt)
                print("  rep %d %-5s: %.4f s/run, %d lidar updates, %d resamplings, final count %d, mean map size %.1f%s" %
                      (rep, route, dt, nl, nr, nn, size, "" if rep else "  (warm-up)"))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("hyp %d medians: host-stop %.4f s, cycle + sync per update %.4f s (%.2fx), cycle queued %.4f s (%.2fx)" %
              (hyp, med["host"], med["sync"], med["host"] / med["sync"], med["queue"], med["host"] / med["queue"]))
    sys.exit(0)

if "--mh-device-cycle" in sys.argv:
    n, hyp, steps, reps = [int(os.environ.get(k, d)) for k, d in (("FS_N", 200), ("FS_HYP", 4), ("FS_STEPS", 100), ("FS_REPS", 3))]
    print("MH-FastSLAM, %d particles, %d hypotheses, %d steps, %d repetitions" % (n, hyp, steps, reps))
    th = mh_route_times(pkg, False, n, hyp, steps, reps)
    td = mh_route_times(pkg, True, n, hyp, steps, reps)
    mh, md = float(np.median(th)), float(np.median(td))
    print("host-planned route: median %.4f ms/cycle (min %.4f, max %.4f)" % (mh * 1e3, min(th) * 1e3, max(th) * 1e3))
    print("device cycle:       median %.4f ms/cycle (min %.4f, max %.4f)  -> %.2fx" % (md * 1e3, min(td) * 1e3, max(td) * 1e3, mh / md))
    sys.exit(0)

N, NM, NZ, HYP = [int(os.environ.get(k, d)) for k, d in (("FS_N", 2000), ("FS_NM", 200), ("FS_NZ", 30), ("FS_HYP", 1))]
scen = sc.make_scenario(N, NM, NZ, seed=4242, rmax=25.0)
f = pkg.FastSLAM(N, gm_capacity=384, max_hypotheses=HYP)    # FS_HYP > 1: MH-FastSLAM (dense table: keep FS_NM, FS_NZ <= 64)
sc.load_scenario(f, scen)
for i in range(N):
    f.import_gm(i, np.zeros(NM), scen["mean"][i], scen["cov"][i])
f.set_fastslam_config(f.fs_config)
f.save_state()
for _ in range(5):
    f.restore_state(); f.fastslam_update(scen["Z"])
f.synchronize()
S = 100
t0 = time.perf_counter()
for _ in range(S):
    f.restore_state()
    f.fastslam_update(scen["Z"])
f.synchronize()
dt = time.perf_counter() - t0
ns = f.last_kernel_ns()
print("device: %.4f ms/update (%.1f updates/s); associate+KF kernel %.1f us, prune+new landmarks %.1f us; map size after %d; particles after %d" %
      (dt / S * 1e3, S / dt, ns[0] / 1e3, ns[3] / 1e3, int(f.gm_sizes().mean()), f.n))
if "--cpu" in sys.argv:
    import importlib
    ob = importlib.import_module("oracle.binding")
    n = 256
    sub = dict(scen); sub.update(n=n, poses=scen["poses"][:n], w=scen["w"][:n], mean=scen["mean"][:n], cov=scen["cov"][:n], particle_w=scen["particle_w"][:n])
    def make():
        o = ob.OracleFilter(n)
        sc.load_scenario(o, sub)
        for i in range(n):
            o.import_gm(i, np.zeros(NM), scen["mean"][i], scen["cov"][i])
        ocfg = o.default_fastslam_config()
        ocfg.maxNDataAssocHypotheses = HYP
        o.set_fastslam_config(ocfg)
        return o
    make().fastslam_update(scen["Z"])          # warm-up instance: the first OpenMP region pays for starting the thread team
    o = make()
    t0 = time.perf_counter()
    o.fastslam_update(scen["Z"])
    dt = time.perf_counter() - t0
    print("oracle (OpenMP, %d host threads): %.1f ms for %d particles -> %.2f updates/s at %d particles" % (os.cpu_count(), dt * 1e3, n, 1.0 / (dt * N / n), N))
