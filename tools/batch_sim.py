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


def make_batch(pkg, a, B):
    return pkg.FastSLAMBatch(B, a.particles, gm_capacity=a.capacity) if a.fastslam else pkg.FilterBatch(B, a.particles, gm_capacity=a.capacity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--handles-max", type=int, default=64, help="largest batch size also run as independent handles")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--json", default="")
    ap.add_argument("--errors", action="store_true", help="track COLA / pose error on the device; tracking off / device / host route timed side by side")
    ap.add_argument("--device-loop", action="store_true", help="the batch's whole cycle on the device (propagation and resampling included)")
    ap.add_argument("--both-loops", action="store_true", help="host loop and device loop side by side")
    ap.add_argument("--fastslam", action="store_true", help="FastSLAM filters: a FastSLAMBatch against FastSLAM handles stepped in turn")
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions of every batch figure")
    a = ap.parse_args()
    pkg = load_pkg()
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
