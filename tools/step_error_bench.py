#!/usr/bin/env python3
"""Workloads for timing map_metric_kernel (csrc/map_metric.h) under a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/step_error_bench.py --batch 16 [--steps 100]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/step_error_bench.py --big 500 [--calls 50]

--batch B: the batch sweep of tools/batch_sim.py at B filters x 200 particles with the device-side error tracking on (at 100 steps
           the realisations hold 2 landmarks: a new one appears every 60 steps).
--batch B --planted N: no simulation: every filter's best particle holds N planted estimates against N landmarks (a finished
           configs[0] map holds 50), scored --calls times.
--batch B --mhfastslam: the multi-hypothesis sweep of tools/batch_sim.py --mhfastslam (golden configuration, --max-per-filter slots per
           filter, default nParticlesMax x hypotheses) on its device loop with tracking: the kernel's live-count instantiation
           (map_metric_kernel<MetricLive>).
--big N:   one ordinary handle whose best particle holds N estimates (jittered copies of N ground-truth landmarks), scored --calls times.
Prints the host's wall time per call; the kernel's own time comes from the trace."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--planted", type=int, default=0)
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--mhfastslam", action="store_true")
    ap.add_argument("--max-per-filter", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    sim = pkg.sim2d_driver
    if a.batch and a.planted:
        n = a.planted
        rng = np.random.default_rng(2)
        side = 0.6 * np.sqrt(n)
        batch = pkg.FilterBatch(a.batch, a.particles, gm_capacity=max(64, n))
        for b in range(a.batch):
            truth = rng.uniform(0, side, (n, 2))
            k = n - int(rng.integers(0, 6))
            est = np.vstack([truth[rng.permutation(n)[:k]] + 0.08 * rng.standard_normal((k, 2)), rng.uniform(0, side, (n - k, 2))])
            batch.import_gm(b * a.particles, np.ones(n), est, np.tile(np.eye(2) * 0.01, (n, 1, 1)))
            batch.set_ground_truth(truth, filter=b)
        batch.error_log_create(a.calls)
        batch.step_error(0.0)
        t0 = time.perf_counter()
        for k in range(a.calls):
            batch.step_error_async(0.1 * k)
        log = batch.error_log_read()
        dt = time.perf_counter() - t0
        print("batch %d, %d planted estimates against %d landmarks per filter: %.1f us per call (host wall, %d calls); mean cola %.3f"
              % (a.batch, n, n, 1e6 * dt / a.calls, a.calls, log["cola"][-1].mean()))
        batch.close()
    elif a.batch and a.mhfastslam:
        import batch_sim
        P0, n = batch_sim.mh_params(sim)
        stride = a.max_per_filter or min(2048, 3 * n * P0["max_hypotheses"])
        Ps, _, seeds = batch_sim.grid(sim, a.batch, 3, fastslam=True)
        Ps = [dict(P0, Pd=P["Pd"], clutter=P["clutter"]) for P in Ps]
        datas = [sim.generate(P, traj_seed=1 + b, kmax=a.steps + 2) for b, P in enumerate(Ps)]
        batch = pkg.MHFastSLAMBatch(a.batch, n, stride, gm_capacity=256)
        run = sim.Sim2dMHBatchRun(batch, datas, Ps, seeds, n, device_loop=True, track_errors=True)
        run.step(1)
        run.synchronize()
        t0 = time.perf_counter()
        for k in range(2, a.steps + 2):
            run.step(k)
        log = run.errors()
        dt = time.perf_counter() - t0
        print("MH batch %d (stride %d): %.1f filter-steps/s on the device loop with tracking; final counts %s; last row n_est %s n_truth %s"
              % (a.batch, stride, a.batch * a.steps / dt, batch.live_counts().tolist(), log["n_est"][-1].tolist(), log["n_truth"][-1].tolist()))
        batch.close()
    elif a.batch:
        import batch_sim
        Ps, datas, seeds = batch_sim.grid(sim, a.batch, a.steps + 2)
        batch = pkg.FilterBatch(a.batch, a.particles, gm_capacity=256)
        run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, track_errors=True)
        dt = batch_sim.timed(run, a.steps)
        log = run.errors()
        print("batch %d: %.1f filter-steps/s with tracking; last row n_est %s n_truth %s" % (a.batch, a.batch * a.steps / dt, log["n_est"][-1].tolist(),
                                                                                           log["n_truth"][-1].tolist()))
        batch.close()
    if a.big:
        n = a.big
        rng = np.random.default_rng(1)
        side = 0.6 * np.sqrt(n)
        truth = rng.uniform(0, side, (n, 2))
        est = truth[rng.permutation(n)] + 0.08 * rng.standard_normal((n, 2))
        f = pkg.RBPHDFilter(200, gm_capacity=max(64, n))
        f.import_gm(0, np.ones(n), est, np.tile(np.eye(2) * 0.01, (n, 1, 1)))
        f.set_ground_truth(truth)
        f.error_log_create(a.calls)
        f.step_error(0.0)          # warm-up (kernel load)
        t0 = time.perf_counter()
        for k in range(a.calls):
            f.step_error_async(0.1 * k)
        log = f.error_log_read()
        dt = time.perf_counter() - t0
        print("one handle, %d estimates against %d landmarks: %.1f us per call (host wall, %d calls); cola %.4f" % (n, n, 1e6 * dt / a.calls, a.calls, log["cola"][-1, 0]))
        f.close()


if __name__ == "__main__":
    main()
