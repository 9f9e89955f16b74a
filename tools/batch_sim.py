#!/usr/bin/env python3
"""A batchSim-style sweep on one GPU (the reference's scripts/batchSim/batchSim_rbphdslam.bash: Pd x clutter x seeds of independent
rbphdslam2dSim runs) through a filter batch (rfsgpu_create_batch), against the same filters as independent handles stepped in turn.

Prints filter-steps/s for batch sizes 1, 4, 16 and 64 at 200 particles (both forms, same per-filter realisations and randomness),
then each run's final map error.  A tuning / evaluation tool, not part of bench.py.

    python tools/batch_sim.py [--steps 200] [--sizes 1,4,16,64] [--particles 200] [--handles-max 64]

--errors: the sweep with the device-side error tracking on (Sim2dBatchRun(track_errors=True): one rfsgpu_step_error_async per cycle, one
log read at the end).  Per filter the final and mean COLA and pose error with the reference's constants (0.75, 0.20, 1.0: src/analysis2dSim.cpp),
the curves in --json, and for every batch size three throughput figures from the one invocation: filter-steps/s (a) with tracking off, (b) with
device tracking, (c) with the host route (per step and filter get_weights + export_gm of the best particle + tools/analysis2d_sim.py::cola).

--device-loop: the batch runs its whole cycle on the device (Sim2dBatchRun(device_loop=True): propagate_async -> cycle_async ->
resample_async, nothing read back until the end; the final synchronisation is inside the timed span).  --both-loops: the host loop
and the device loop from the one invocation, both figures in the line.  Every line names its loop kind ("loop").  --reps N: N timed
repetitions of each figure (fresh batch each), all of them in the line ("..._reps") next to their median.

--fastslam: the same table for the FastSLAM half of a comparison sweep (the reference's fastslam2dSim over the same grid): a
FastSLAMBatch (rfsgpu_batch_fastslam_cycle_async) against FastSLAM handles stepped in turn (predict_map, fastslam_update, normalise,
resample per handle), host loop / device loop, --errors.  Every line then carries "filter": "fastslam".

--mhfastslam: the third sweep of the reference's scripts/batchSim (batchSim_mhfastslam.bash): multi-hypothesis FastSLAM filters with the
filter values of tests/golden/mhfastslam2dSim_c1.xml (200 particles, 3 hypotheses, log-likelihood window 3.0) as an MHFastSLAMBatch
(rfsgpu_batch_fastslam_mh_cycle_async; --max-per-filter slots per filter, default nParticlesMax x hypotheses = 1800) against the same filters as handles on
rfsgpu_fastslam_cycle_async stepped in turn.  --both-loops / --device-loop / --reps as above; every line carries "filter": "mhfastslam".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.load_package() if hasattr(g, "load_package") else None


def grid(sim, n, kmax, fastslam=False):
    pds = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.85, 0.75, 0.65]
    clutters = [1e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 1e-1]
    Ps, datas, seeds = [], [], []
    for b in range(n):
        P = dict(sim.C1_FASTSLAM_SIM if fastslam else sim.C1_SIM)
        P["Pd"] = pds[b % len(pds)]
        P["clutter"] = clutters[(b // len(pds)) % len(clutters)]
        Ps.append(P)
        datas.append(sim.generate(P, traj_seed=1 + b, kmax=kmax))
        seeds.append(100 + b)
    return Ps, datas, seeds


def timed(run, steps):
    run.step(1)                       # warm-up (kernel loads, first allocations)
    t0 = time.perf_counter()
    for k in range(2, steps + 2):
        run.step(k)
    return time.perf_counter() - t0


def timed_synced(run, steps):
    """As timed(), for a loop that waits for nothing: the span ends when the queued work is done."""
    run.step(1)
    run.batch.synchronize()
    t0 = time.perf_counter()
    for k in range(2, steps + 2):
        run.step(k)
    run.batch.synchronize()
    return time.perf_counter() - t0


def host_route_errors(batch, datas, firsts, Ps, k, a2d, fastslam=False):
    """What a caller had to do per step before the device metric: per filter the weights, the best particle's mixture, scipy."""
    out = []
    for b in range(batch.n_filters):
        w = batch.get_weights()[batch.block(b)]
        i = b * batch.n_per_filter + int(np.argmax(w))
        gw, _, mean, _ = batch.export_gm(i)
        if fastslam:
            gw = 1 - 1 / (1 + np.exp(gw))         # log-odds -> existence probability (fastslam2dSim.cpp:628)
        seen = datas[b]["landmarks"][firsts[b] <= k * Ps[b]["dt"]]
        out.append(a2d.cola(mean[gw >= a2d.W_THRESHOLD], seen))
    return out


def timed_host_route(run, steps, datas, firsts, Ps, a2d, fastslam=False):
    run.step(1)
    t0 = time.perf_counter()
    for k in range(2, steps + 2):
        run.step(k)
        host_route_errors(run.batch, datas, firsts, Ps, k, a2d, fastslam)
    return time.perf_counter() - t0


def errors_sweep(pkg, a, sizes, Ps, datas, seeds):
    import importlib.util
    spec = importlib.util.spec_from_file_location("analysis2d_sim", os.path.join(ROOT, "tools", "analysis2d_sim.py"))
    a2d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(a2d)
    sim = pkg.sim2d_driver
    firsts = [sim.first_seen_times(d, P) for d, P in zip(datas, Ps)]
    rows = []
    for B in sizes:
        row = dict(B=B, particles=a.particles, steps=a.steps)
        if a.fastslam:
            row["filter"] = "fastslam"
        for name in ("off", "device", "host"):
            batch = make_batch(pkg, a, B)
            run = sim.Sim2dBatchRun(batch, datas[:B], Ps[:B], seeds[:B], track_errors=(name == "device"), fastslam=a.fastslam)
            dt = timed_host_route(run, a.steps, datas, firsts, Ps, a2d, a.fastslam) if name == "host" else timed(run, a.steps)
            if name == "device":
                t0 = time.perf_counter()
                log = run.errors()                      # the one read (it also waits for the queued work)
                dt += time.perf_counter() - t0
            else:
                batch.synchronize()
            row["filter_steps_per_s_tracking_" + name] = B * a.steps / dt
            if name == "device":
                row["filters"] = [dict(filter=b, Pd=Ps[b]["Pd"], clutter=Ps[b]["clutter"], seed=1 + b, final_cola=float(log["cola"][-1, b]),
                                       mean_cola=float(log["cola"][:, b].mean()), final_pose_error=float(log["pose_ed"][-1, b]),
                                       mean_pose_error=float(log["pose_ed"][:, b].mean()), n_est=int(log["n_est"][-1, b]), n_truth=int(log["n_truth"][-1, b]),
                                       curve_t=log["t"][:, b].tolist(), curve_cola=log["cola"][:, b].tolist(), curve_pose_error=log["pose_ed"][:, b].tolist())
                                  for b in range(B)]
            batch.close()
        row["device_over_off"] = row["filter_steps_per_s_tracking_device"] / row["filter_steps_per_s_tracking_off"]
        row["host_over_off"] = row["filter_steps_per_s_tracking_host"] / row["filter_steps_per_s_tracking_off"]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "filters"}), flush=True)
    for r in rows[-1]["filters"]:
        print("filter %3d  Pd %.2f  clutter %.0e  seed %3d  COLA final %6.2f mean %6.2f (est %2d / truth %2d)  pose error final %.4f mean %.4f"
              % (r["filter"], r["Pd"], r["clutter"], r["seed"], r["final_cola"], r["mean_cola"], r["n_est"], r["n_truth"], r["final_pose_error"], r["mean_pose_error"]))
    return rows


def mh_params(sim):
    """C1_FASTSLAM_SIM with the filter values of tests/golden/mhfastslam2dSim_c1.xml (200 particles, 3 hypotheses, window 3.0)."""
    import xml.etree.ElementTree as ET
    t = ET.parse(os.path.join(ROOT, "tests", "golden", "mhfastslam2dSim_c1.xml")).getroot()
    g = lambda path: t.find(path).text
    P = dict(sim.C1_FASTSLAM_SIM, max_hypotheses=int(g("filter/update/maxNDataAssocHypotheses")), max_loglik_diff=float(g("filter/update/maxDataAssocLogLikelihoodDiff")),
             min_log_likelihood=float(g("filter/weighting/minLogMeasurementLikelihood")), existence_prune_thr=float(g("filter/prune/threshold")),
             eff_n=float(g("filter/resampling/effNParticle")), min_updates=int(g("filter/resampling/minTimesteps")))
    return P, int(next(t.iter("nParticles")).text)


class MhRun:
    """The simulator loop for multi-hypothesis FastSLAM filters in one of three forms: an MHFastSLAMBatch with its host loop (the host
    reads the counts and poses back, propagates the live slots and passes them with the cycle) or its device loop (propagate_async +
    cycle, nothing read back), or handles on rfsgpu_fastslam_cycle_async stepped in turn.  Every filter's draws are pre-drawn from its
    seed, so the device loop waits for nothing."""

    def __init__(self, pkg, target, datas, Ps, seeds, n, device_loop=False):
        sim = pkg.sim2d_driver
        self.sim, self.datas, self.Ps, self.n, self.nF = sim, datas, Ps, n, len(datas)
        self.batch = target if isinstance(target, pkg.capi.CBatchMH) else None
        self.handles = None if self.batch is not None else list(target)
        self.device_loop = bool(device_loop)
        K = int(min(d["K"] for d in datas))
        self.rngs = [np.random.default_rng(s) for s in seeds]
        self.u01 = np.ascontiguousarray(np.stack([np.random.default_rng(10_000 + s).random(K) for s in seeds], axis=1))      # [K, nF]
        self.Q = [np.diag([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2 for P in Ps]
        for b, P in enumerate(Ps):
            if self.batch is not None:
                c = sim.configure_fastslam_batch_filter(self.batch, b, P)
                c.nParticlesMax = 3 * n
                self.batch.configure_fastslam(b, c)
                self.batch.set_resampling(b, P["eff_n"], P["eff_n"] / n)
                self.batch.set_motion_odometry(b, np.diag(self.Q[b]), seeds[b])
            else:
                h = self.handles[b]
                h.fs_config = sim.configure_fastslam(h, P)
                h.fs_config.nParticlesMax = 3 * n
                h.setEffectiveParticleCountThreshold(P["eff_n"])
        self._u = np.ascontiguousarray(np.stack([d["odom"][:K] for d in datas], axis=1))
        self._gt = np.ascontiguousarray(np.stack([d["gt"][:K] for d in datas], axis=1))
        self._z = np.zeros((K, self.nF, pkg.capi.MAX_Z, 2))
        self._nz = np.zeros((K, self.nF), dtype=np.int32)
        for b, d in enumerate(datas):
            for k in range(K):
                Z = d["Z"][k] if k < len(d["Z"]) else np.zeros((0, 2))
                self._nz[k, b] = len(Z)
                self._z[k, b, :len(Z)] = Z
        self._pin_all = np.ones(self.nF, dtype=np.uint8)

    def _moved(self, b, x, k):
        """ParticleFilter::propagate of filter b's live particles on the host (the ground truth for the first 100 steps, :590-593)."""
        if k <= 100:
            return np.tile(self._gt[k, b], (x.shape[0], 1)), np.zeros(9)
        noise = self.rngs[b].standard_normal(x.shape) * np.sqrt(np.diag(self.Q[b]))
        return self.sim.odometry_step(x, self._u[k, b]) + noise, self.Q[b].ravel()

    def step(self, k):
        bt = self.batch
        if self.device_loop:
            bt.propagate_async(self._u[k], k, pin=self._pin_all if k <= 100 else None, pin_pose=self._gt[k] if k <= 100 else None)
            bt.batch_fastslam_mh_cycle_async_packed(True, self._z[k], self._nz[k], self.u01[k])
        elif bt is not None:
            counts = bt.live_counts()
            x = bt.get_poses()
            cov = np.zeros((bt.n, 9))
            for b in range(self.nF):
                blk = bt.block(b, counts[b])
                x[blk], cov[blk] = self._moved(b, x[blk], k)
            bt.batch_fastslam_mh_cycle_async_packed(True, self._z[k], self._nz[k], self.u01[k], poses=x, pose_cov=cov)
        else:
            for b, h in enumerate(self.handles):
                x, c = self._moved(b, h.get_poses(), k)
                h.set_poses(x, np.tile(c, (x.shape[0], 1)))
                h.cycle_async(self._z[k, b, :self._nz[k, b]], float(self.u01[k, b]), predict=True)

    def synchronize(self):
        for f in ([self.batch] if self.batch is not None else self.handles):
            f.synchronize()


def mh_handle(pkg, n, max_per_filter, capacity):
    """A FastSLAM handle on the device cycle with exactly max_per_filter particle slots: the batch's yardstick."""
    return pkg.FastSLAM(n, gm_capacity=capacity, device_cycle=True, max_particles=max_per_filter)


def mh_sweep(pkg, a, sizes):
    """--mhfastslam: filter-steps/s of an MHFastSLAMBatch (host loop and / or device loop) and of the same filters as handles on
    rfsgpu_fastslam_cycle_async stepped in turn; each figure the median of --reps timed repetitions within this invocation."""
    sim = pkg.sim2d_driver
    P0, n_xml = mh_params(sim)
    n = a.particles or n_xml
    stride = a.max_per_filter or min(2048, 3 * n * P0["max_hypotheses"])      # nParticlesMax x hypotheses: cannot overflow
    pds = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.85, 0.75, 0.65]
    clutters = [1e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 1e-1]
    Ps = [dict(P0, Pd=pds[b % len(pds)], clutter=clutters[(b // len(pds)) % len(clutters)]) for b in range(max(sizes))]
    datas = [sim.generate(P, traj_seed=1 + b, kmax=a.steps + 2) for b, P in enumerate(Ps)]
    seeds = [100 + b for b in range(max(sizes))]
    loops = ["host", "device"] if a.both_loops else (["device"] if a.device_loop else ["host"])

    def timed_run(make):
        figs = []
        for _ in range(max(1, a.reps)):
            run, close = make()
            run.step(1)
            run.synchronize()
            t0 = time.perf_counter()
            for k in range(2, a.steps + 2):
                run.step(k)
            run.synchronize()
            figs.append(len(run.datas) * a.steps / (time.perf_counter() - t0))
            extra = run.batch.live_counts().tolist() if run.batch is not None else None
            close()
        return figs, extra

    rows = []
    for B in sizes:
        row = dict(B=B, particles=n, max_per_filter=stride, steps=a.steps, filter="mhfastslam", hypotheses=P0["max_hypotheses"], loop="+".join(loops))
        for loop in loops:
            def make(loop=loop):
                bt = pkg.MHFastSLAMBatch(B, n, stride, gm_capacity=a.capacity)
                return MhRun(pkg, bt, datas[:B], Ps[:B], seeds[:B], n, device_loop=(loop == "device")), bt.close
            figs, counts = timed_run(make)
            key = "batch_filter_steps_per_s" if loop == "host" else "device_loop_filter_steps_per_s"
            row[key], row[key + "_reps"] = float(np.median(figs)), figs
            row["final_counts_" + loop] = counts
        if B <= a.handles_max:
            def make_h():
                hs = [mh_handle(pkg, n, stride, a.capacity) for _ in range(B)]
                return MhRun(pkg, hs, datas[:B], Ps[:B], seeds[:B], n), (lambda: [h.close() for h in hs])
            figs, _ = timed_run(make_h)
            row["handles_filter_steps_per_s"], row["handles_filter_steps_per_s_reps"] = float(np.median(figs)), figs
            for key, name in (("batch_filter_steps_per_s", "speedup"), ("device_loop_filter_steps_per_s", "device_loop_speedup")):
                if key in row:
                    row[name] = row[key] / row["handles_filter_steps_per_s"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


def make_batch(pkg, a, B):
    return pkg.FastSLAMBatch(B, a.particles, gm_capacity=a.capacity) if a.fastslam else pkg.FilterBatch(B, a.particles, gm_capacity=a.capacity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--particles", type=int, default=None, help="particles per filter (default 200; --mhfastslam: the golden configuration's)")
    ap.add_argument("--handles-max", type=int, default=64, help="largest batch size also run as independent handles")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--json", default="")
    ap.add_argument("--errors", action="store_true", help="track COLA / pose error on the device; tracking off / device / host route timed side by side")
    ap.add_argument("--device-loop", action="store_true", help="the batch's whole cycle on the device (propagation and resampling included)")
    ap.add_argument("--both-loops", action="store_true", help="host loop and device loop side by side")
    ap.add_argument("--fastslam", action="store_true", help="FastSLAM filters: a FastSLAMBatch against FastSLAM handles stepped in turn")
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions of every batch figure")
    ap.add_argument("--mhfastslam", action="store_true", help="multi-hypothesis FastSLAM filters: an MHFastSLAMBatch against handles on the device cycle stepped in turn")
    ap.add_argument("--max-per-filter", type=int, default=0, help="--mhfastslam: particle slots per filter (default nParticlesMax x hypotheses = 9 x particles, which cannot overflow; at most 2048)")
    a = ap.parse_args()
    pkg = load_pkg()
    if a.mhfastslam:
        return mh_sweep(pkg, a, [int(s) for s in a.sizes.split(",")])
    a.particles = a.particles or 200
    sim = pkg.sim2d_driver
    sizes = [int(s) for s in a.sizes.split(",")]
    kmax = a.steps + 2
    Ps, datas, seeds = grid(sim, max(sizes), kmax, a.fastslam)
    rows = []
    if a.errors:
        erows = errors_sweep(pkg, a, sizes, Ps, datas, seeds)
    loops = ["host", "device"] if a.both_loops else (["device"] if a.device_loop else ["host"])
    for B in sizes:
        figs = {}
        for loop in loops:
            figs[loop] = []
            for rep in range(max(1, a.reps)):
                if rep or loop != loops[0]:
                    batch.close()
                batch = make_batch(pkg, a, B)
                rb = sim.Sim2dBatchRun(batch, datas[:B], Ps[:B], seeds[:B], device_loop=(loop == "device"), fastslam=a.fastslam)
                t = timed_synced(rb, a.steps) if loop == "device" else timed(rb, a.steps)
                batch.synchronize()
                figs[loop].append(B * a.steps / t)
        tb = B * a.steps / float(np.median(figs[loops[0]]))
        row = dict(B=B, particles=a.particles, steps=a.steps, loop="+".join(loops), batch_filter_steps_per_s=float(np.median(figs[loops[0]])))
        if a.fastslam:
            row["filter"] = "fastslam"
        if a.reps > 1:
            row["batch_filter_steps_per_s_reps"] = figs[loops[0]]
        if len(loops) == 2:
            row["device_loop_filter_steps_per_s"] = float(np.median(figs["device"]))
            row["device_over_host_loop"] = row["device_loop_filter_steps_per_s"] / row["batch_filter_steps_per_s"]
            if a.reps > 1:
                row["device_loop_filter_steps_per_s_reps"] = figs["device"]
            row["resamples_device_loop"] = rb.resample_counts().tolist()
        if B <= a.handles_max:
            hs = [(pkg.FastSLAM if a.fastslam else pkg.RBPHDFilter)(a.particles, gm_capacity=a.capacity) for _ in range(B)]
            rh = sim.Sim2dBatchRun(hs, datas[:B], Ps[:B], seeds[:B], fastslam=a.fastslam)
            th = timed(rh, a.steps)
            for h in hs:
                h.synchronize()
            row["handles_filter_steps_per_s"] = B * a.steps / th
            row["speedup"] = th / tb
            if len(loops) == 2:
                row["device_loop_speedup"] = row["device_loop_filter_steps_per_s"] / row["handles_filter_steps_per_s"]
            for h in hs:
                h.close()
        if B == max(sizes):
            errs = []
            for b in range(B):
                w = batch.get_weights()[batch.block(b)]
                i = b * a.particles + int(np.argmax(w))
                nm, e, ns = sim.map_error(batch, i, datas[b]["landmarks"], w_min=(float(np.log(3.0)) if a.fastslam else 0.5))   # (log-odds of 0.75)
                errs.append(dict(filter=b, Pd=Ps[b]["Pd"], clutter=Ps[b]["clutter"], seed=1 + b, matched=nm, n_landmarks=len(datas[b]["landmarks"]),
                                 mean_error=e, strong=ns))
            row["map_error"] = errs
        batch.close()
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "map_error"}), flush=True)
    for r in rows[-1].get("map_error", []):
        print("filter %3d  Pd %.2f  clutter %.0e  seed %3d  matched %2d/%2d  mean error %.4f" % (r["filter"], r["Pd"], r["clutter"], r["seed"], r["matched"],
                                                                                            r["n_landmarks"], r["mean_error"]))
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(sweep=rows, errors=erows) if a.errors else rows, fh, indent=1)


if __name__ == "__main__":
    main()
