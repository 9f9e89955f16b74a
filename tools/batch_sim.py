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

--device-sensor (any of the three kinds: with --fastslam / --mhfastslam the batch's sensor service is switched on,
rfsgpu_batch_fastslam_serve_sensor, and the sensed cycle is the kind's own; implies the device loop, --device-loop / --both-loops are accepted and ignored): per batch size the
device loop fed with host-made scans against the device loop whose scans the device draws (Sim2dBatchRun(device_sensor=True):
propagate_async -> sense_async -> cycle_sensed_async -> resample_sensed_async).  Each line has, for either route and from the one
invocation, the setup time (sim2d_driver.generate + packing, or generate(measurements=False) + set_sensor) and the run time
separately, with all --reps repetitions and their medians, and filter-steps/s without and with the setup.  --errors / --results / --json
work as elsewhere (the filters listed are the device-sensor route's).

--device-truth (any of the three kinds; implies --device-loop --device-sensor; given TOGETHER with --device-sensor the line has all
three routes -- host-made scans, device-made scans, device-made truth -- and the host-made against the device-made ratio): per batch size the
device loop with device-made scans on a host-made ground truth (generate(measurements=False): the "device_scans" route above) against
the same loop on a device-made ground truth (Sim2dBatchRun(device_truth=True): set_truth + one generate_truth, the landmarks read back
once for the sensors, and the whole run ONE rfsgpu_batch_run_truth_async).  Setup and run time of each route as with --device-sensor.

--estimates [--log-particles] [--log-dir DIR] (with --device-truth; any of the three kinds): the one-call run with the device-side estimate
log ([estimate] in include/rfsgpu.h) off, on and -- with --log-particles -- on with the particle planes, side by side (the one read of the log
timed apart), against the per-step host route to the same data (get_weights + get_poses + get_map_estimate per filter and step).
--log-dir leaves one directory per filter of the largest batch in the reference's log-file formats (sim2d_driver.write_run_logs):
    python tools/analysis2d_sim.py DIR/filter_000/

--fastslam: the same table for the FastSLAM half of a comparison sweep (the reference's fastslam2dSim over the same grid): a
FastSLAMBatch (rfsgpu_batch_fastslam_cycle_async) against FastSLAM handles stepped in turn (predict_map, fastslam_update, normalise,
resample per handle), host loop / device loop, --errors.  Every line then carries "filter": "fastslam".

--mhfastslam: the third sweep of the reference's scripts/batchSim (batchSim_mhfastslam.bash): multi-hypothesis FastSLAM filters with the
filter values of tests/golden/mhfastslam2dSim_c1.xml (200 particles, 3 hypotheses, log-likelihood window 3.0) as an MHFastSLAMBatch
(rfsgpu_batch_fastslam_mh_cycle_async; --max-per-filter slots per filter, default nParticlesMax x hypotheses = 1800) against the same filters as handles on
rfsgpu_fastslam_cycle_async stepped in turn (sim2d_driver.Sim2dMHBatchRun).  --both-loops / --device-loop / --reps as above; every line
carries "filter": "mhfastslam".  With --errors the sweep is the tracking one instead: per batch size and loop kind filter-steps/s with
tracking off, with device tracking (the batch's metric service on, one rfsgpu_step_error_async per step whose kernel reads every filter's
live count on the device, the log read inside the span) and with the host route (per step and filter live_counts + get_weights of the live
slots + export_gm of the best one + tools/analysis2d_sim.py::cola on 1 - 1 / (1 + exp(w))); then per filter the final and mean COLA and
pose error, the curves in --json.

--results FILE (with --errors, any of the three kinds): one line per filter of the largest batch, "Pd  c  posError  mapError" -- the final
row's pose_ed and cola, the two columns the reference's batchSim scripts cut out of poseEstError.dat (field 5) and landmarkEstError.dat
(field 4).
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
    a2d = load_a2d()
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
                row["filters"] = filter_rows(log, Ps, B)
            batch.close()
        row["device_over_off"] = row["filter_steps_per_s_tracking_device"] / row["filter_steps_per_s_tracking_off"]
        row["host_over_off"] = row["filter_steps_per_s_tracking_host"] / row["filter_steps_per_s_tracking_off"]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "filters"}), flush=True)
    print_filters(rows[-1]["filters"])
    write_results(a.results, rows[-1]["filters"])
    return rows


def filter_rows(log, Ps, B):
    """Per filter what an --errors sweep reports of a log [steps, B]: final and mean COLA / pose error, the curves."""
    return [dict(filter=b, Pd=Ps[b]["Pd"], clutter=Ps[b]["clutter"], seed=1 + b, final_cola=float(log["cola"][-1, b]),
                 mean_cola=float(log["cola"][:, b].mean()), final_pose_error=float(log["pose_ed"][-1, b]),
                 mean_pose_error=float(log["pose_ed"][:, b].mean()), n_est=int(log["n_est"][-1, b]), n_truth=int(log["n_truth"][-1, b]),
                 curve_t=log["t"][:, b].tolist(), curve_cola=log["cola"][:, b].tolist(), curve_pose_error=log["pose_ed"][:, b].tolist())
            for b in range(B)]


def print_filters(filters):
    for r in filters:
        print("filter %3d  Pd %.2f  clutter %.0e  seed %3d  COLA final %6.2f mean %6.2f (est %2d / truth %2d)  pose error final %.4f mean %.4f"
              % (r["filter"], r["Pd"], r["clutter"], r["seed"], r["final_cola"], r["mean_cola"], r["n_est"], r["n_truth"], r["final_pose_error"], r["mean_pose_error"]))


def write_results(path, filters):
    """--results: one line per filter, Pd  c  posError  mapError (the final row's pose_ed and cola), as the reference's batchSim scripts end."""
    if not path:
        return
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        for r in filters:
            fh.write("%g  %g  %.9g  %.9g\n" % (r["Pd"], r["clutter"], r["final_pose_error"], r["final_cola"]))


def load_a2d():
    import importlib.util
    spec = importlib.util.spec_from_file_location("analysis2d_sim", os.path.join(ROOT, "tools", "analysis2d_sim.py"))
    a2d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(a2d)
    return a2d


def mh_host_route_errors(batch, datas, firsts, Ps, k, a2d):
    """The only route to an error curve of an MH batch before the metric service: per step the counts, per filter the weights of its live
    slots, the best one's mixture, scipy."""
    counts = batch.live_counts()
    wall = batch.get_weights()                    # (one read per step for all filters: the cheapest form of this route)
    out = []
    for b in range(batch.n_filters):
        w = wall[batch.block(b, counts[b])]
        i = b * batch.max_per_filter + int(np.argmax(w))
        gw, _, mean, _ = batch.export_gm(i)
        gw = 1 - 1 / (1 + np.exp(gw))             # log-odds -> existence probability (fastslam2dSim.cpp:628)
        seen = datas[b]["landmarks"][firsts[b] <= k * Ps[b]["dt"]]
        out.append(a2d.cola(mean[gw >= a2d.W_THRESHOLD], seen))
    return out


def mh_errors_sweep(pkg, a, sizes, n, stride, P0, Ps, datas, seeds, loops):
    """--mhfastslam --errors: per batch size and loop kind, filter-steps/s with tracking off / device tracking (log read in the span) /
    the host route, medians of --reps repetitions; the largest batch's per-filter figures from its last device-tracked run."""
    sim = pkg.sim2d_driver
    a2d = load_a2d()
    firsts = [sim.first_seen_times(d, P) for d, P in zip(datas, Ps)]
    rows = []
    for B in sizes:
        row = dict(B=B, particles=n, max_per_filter=stride, steps=a.steps, filter="mhfastslam", hypotheses=P0["max_hypotheses"], loop="+".join(loops))
        for loop in loops:
            for name in ("off", "device", "host"):
                figs = []
                for _ in range(max(1, a.reps)):
                    bt = pkg.MHFastSLAMBatch(B, n, stride, gm_capacity=a.capacity)
                    run = sim.Sim2dMHBatchRun(bt, datas[:B], Ps[:B], seeds[:B], n, device_loop=(loop == "device"), track_errors=(name == "device"))
                    run.step(1)
                    run.synchronize()
                    t0 = time.perf_counter()
                    for k in range(2, a.steps + 2):
                        run.step(k)
                        if name == "host":
                            mh_host_route_errors(bt, datas, firsts, Ps, k, a2d)
                    if name == "device":
                        log = run.errors()                  # the one read (it also waits for the queued work)
                    else:
                        run.synchronize()
                    figs.append(B * a.steps / (time.perf_counter() - t0))
                    bt.close()
                key = "%s_loop_filter_steps_per_s_tracking_%s" % (loop, name)
                row[key], row[key + "_reps"] = float(np.median(figs)), figs
                if name == "device":
                    row["filters"] = filter_rows(log, Ps, B)
            row[loop + "_loop_device_over_off"] = row[loop + "_loop_filter_steps_per_s_tracking_device"] / row[loop + "_loop_filter_steps_per_s_tracking_off"]
            row[loop + "_loop_device_over_host_route"] = row[loop + "_loop_filter_steps_per_s_tracking_device"] / row[loop + "_loop_filter_steps_per_s_tracking_host"]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "filters"}), flush=True)
    print_filters(rows[-1]["filters"])
    write_results(a.results, rows[-1]["filters"])
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
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
    if a.errors:
        return mh_errors_sweep(pkg, a, sizes, n, stride, P0, Ps, datas, seeds, loops)

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
                return sim.Sim2dMHBatchRun(bt, datas[:B], Ps[:B], seeds[:B], n, device_loop=(loop == "device")), bt.close
            figs, counts = timed_run(make)
            key = "batch_filter_steps_per_s" if loop == "host" else "device_loop_filter_steps_per_s"
            row[key], row[key + "_reps"] = float(np.median(figs)), figs
            row["final_counts_" + loop] = counts
        if B <= a.handles_max:
            def make_h():
                hs = [mh_handle(pkg, n, stride, a.capacity) for _ in range(B)]
                return sim.Sim2dMHBatchRun(hs, datas[:B], Ps[:B], seeds[:B], n), (lambda: [h.close() for h in hs])
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


def sensor_sweep(pkg, a, sizes):
    """--device-sensor: the device loop with host-made scans (generate() draws them, Sim2dBatchRun packs them) against the device loop
    with device-made scans (generate(measurements=False), one rfsgpu_batch_set_sensor per filter, sense_async per step).  Per batch size
    and route, from the one invocation: the setup time (generation + packing / sensor configuration) and the run time (timed span with
    the final synchronisation inside) separately, medians and all --reps repetitions, and filter-steps/s of the run alone and of setup +
    run.  With --errors both routes track the errors on the device (the log read inside the span) and the largest batch's device-sensor
    filters are listed (--results, --json as elsewhere).  The two routes run the same model on different realisations of the scans."""
    sim = pkg.sim2d_driver
    pds = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.85, 0.75, 0.65]
    clutters = [1e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 1e-1]
    # (--fastslam / --mhfastslam: the same table for a FastSLAMBatch / an MHFastSLAMBatch, whose sensor service the run switches on)
    n, stride = a.particles, 0
    P0 = sim.C1_FASTSLAM_SIM if a.fastslam else sim.C1_SIM
    if a.mhfastslam:
        P0, n_xml = mh_params(sim)
        n = a.particles or n_xml
        stride = a.max_per_filter or min(2048, 3 * n * P0["max_hypotheses"])
    Ps = [dict(P0, Pd=pds[b % len(pds)], clutter=clutters[(b // len(pds)) % len(clutters)]) for b in range(max(sizes))]
    seeds = [100 + b for b in range(max(sizes))]
    kmax = a.steps + 2
    rows = []
    routes = (("host", "device", "truth") if a.all_routes else ("device", "truth")) if a.device_truth else ("host", "device")

    def make_run(batch, B, route):
        datas = None if route == "truth" else [sim.generate(Ps[b], traj_seed=1 + b, kmax=kmax, measurements=(route == "host")) for b in range(B)]
        if a.mhfastslam:
            return sim.Sim2dMHBatchRun(batch, datas, Ps[:B], seeds[:B], n, device_loop=True, track_errors=a.errors, device_sensor=(route == "device"),
                                       device_truth=(route == "truth"), kmax=kmax)
        if route == "truth":
            return sim.Sim2dBatchRun(batch, None, Ps[:B], seeds[:B], track_errors=a.errors, fastslam=a.fastslam, device_truth=True, kmax=kmax)
        return sim.Sim2dBatchRun(batch, datas, Ps[:B], seeds[:B], track_errors=a.errors, fastslam=a.fastslam, device_loop=True, device_sensor=(route == "device"))

    for B in sizes:
        row = dict(B=B, particles=n, steps=a.steps, loop="device", reps=max(1, a.reps))
        if a.fastslam or a.mhfastslam:
            row["filter"] = "mhfastslam" if a.mhfastslam else "fastslam"
        for route in routes:
            setup, run_t = [], []
            for _ in range(max(1, a.reps)):
                batch = pkg.MHFastSLAMBatch(B, n, stride, gm_capacity=a.capacity) if a.mhfastslam else make_batch(pkg, a, B)
                batch.synchronize()
                t0 = time.perf_counter()
                rb = make_run(batch, B, route)
                setup.append(time.perf_counter() - t0)
                rb.step(1)
                batch.synchronize()
                t0 = time.perf_counter()
                if route == "truth":
                    rb.run(2, a.steps + 2)            # one call: the loop over steps is the library's
                else:
                    for k in range(2, a.steps + 2):
                        rb.step(k)
                if a.errors:
                    log = rb.errors()               # the one read (it also waits for the queued work)
                else:
                    batch.synchronize()
                run_t.append(time.perf_counter() - t0)
                if route == routes[-1]:
                    if a.mhfastslam:
                        row["final_counts_device_" + ("truth" if route == "truth" else "scans")] = batch.live_counts().tolist()
                    else:
                        row["resamples_device_" + ("truth" if route == "truth" else "scans")] = rb.resample_counts().tolist()
                    if a.errors:
                        row["filters"] = filter_rows(log, Ps, B)
                batch.close()
            key = "device_truth_" if route == "truth" else route + "_scans_"
            row[key + "setup_s"], row[key + "setup_s_reps"] = float(np.median(setup)), setup
            row[key + "run_s"], row[key + "run_s_reps"] = float(np.median(run_t)), run_t
            row[key + "filter_steps_per_s"] = B * a.steps / row[key + "run_s"]
            row[key + "filter_steps_per_s_with_setup"] = B * a.steps / (row[key + "setup_s"] + row[key + "run_s"])
            if route == "host":
                row["host_scans_packed_bytes_per_step"] = int(B * pkg.capi.MAX_Z * 2 * 8 + B * 4)
        if a.device_truth and a.all_routes:      # the host-made route (scans and truth made and packed on the host) against the device-made one
            row["device_truth_over_host_scans_run"] = row["host_scans_run_s"] / row["device_truth_run_s"]
            row["device_truth_over_host_scans_with_setup"] = (row["host_scans_setup_s"] + row["host_scans_run_s"]) / (row["device_truth_setup_s"] + row["device_truth_run_s"])
        if a.device_truth:
            row["device_over_host_truth_run"] = row["device_scans_run_s"] / row["device_truth_run_s"]
            row["device_over_host_truth_with_setup"] = (row["device_scans_setup_s"] + row["device_scans_run_s"]) / (row["device_truth_setup_s"] + row["device_truth_run_s"])
        else:
            row["device_over_host_scans_run"] = row["host_scans_run_s"] / row["device_scans_run_s"]
            row["device_over_host_scans_with_setup"] = (row["host_scans_setup_s"] + row["host_scans_run_s"]) / (row["device_scans_setup_s"] + row["device_scans_run_s"])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "filters"}), flush=True)
    if a.errors:
        print_filters(rows[-1]["filters"])
        write_results(a.results, rows[-1]["filters"])
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return rows


def host_route_estimates(batch, B, thr):
    """What a caller had to do per step for the same data before the estimate log: the weights and poses, and per filter the best
    particle's map (rfsgpu_get_map_estimate: a metric launch and the fetch of a whole particle)."""
    out = [batch.get_weights(), batch.get_poses()]
    for b in range(B):
        out.append(batch.get_map_estimate(thr, filter=b))
    return out


def estimates_sweep(pkg, a, sizes):
    """--estimates (with --device-truth; any of the three kinds): per batch size the one-call run (rfsgpu_batch_run_truth_async) with
    the estimate log off, on (rfsgpu_batch_run_log_estimates: one rfsgpu_step_estimate row per step, every Gaussian of the best
    particle) and on with the particle planes, medians of --reps repetitions from the one invocation, the span ending with the
    stream's synchronisation; the one read of the whole log is timed apart ("estimate_log_read_s_*");
    and the per-step host route to the same data (get_weights + get_poses + get_map_estimate per filter and step) once.  The variant
    with particles runs with --log-particles (or --log-dir).  --log-dir DIR:
    the largest batch's last run with particles leaves DIR/filter_NNN/ per filter (sim2d_driver.write_run_logs, 17 digits), which
    tools/analysis2d_sim.py analyses."""
    sim = pkg.sim2d_driver
    pds = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.85, 0.75, 0.65]
    clutters = [1e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 1e-1]
    n, stride = a.particles, 0
    P0 = sim.C1_FASTSLAM_SIM if a.fastslam else sim.C1_SIM
    if a.mhfastslam:
        P0, n_xml = mh_params(sim)
        n = a.particles or n_xml
        stride = a.max_per_filter or min(2048, 3 * n * P0["max_hypotheses"])
    Ps = [dict(P0, Pd=pds[b % len(pds)], clutter=clutters[(b // len(pds)) % len(clutters)]) for b in range(max(sizes))]
    seeds = [100 + b for b in range(max(sizes))]
    kmax = a.steps + 2
    thr = sim.ESTIMATE_W_THRESHOLD

    def make(B, estimates, particles):
        batch = pkg.MHFastSLAMBatch(B, n, stride, gm_capacity=a.capacity) if a.mhfastslam else make_batch(pkg, a, B)
        kw = dict(device_truth=True, kmax=kmax, track_estimates=estimates, estimate_threshold=thr, log_particles=particles)
        if a.mhfastslam:
            run = sim.Sim2dMHBatchRun(batch, None, Ps[:B], seeds[:B], n, **kw)
        else:
            run = sim.Sim2dBatchRun(batch, None, Ps[:B], seeds[:B], fastslam=a.fastslam, **kw)
        run.step(1)                       # warm-up (kernel loads, first allocations)
        batch.synchronize()
        return batch, run

    variants = [("off", False, False), ("on", True, False)]
    if a.log_particles or a.log_dir:      # (particlePose.dat needs the particle planes)
        variants.append(("on_particles", True, True))
    rows = []
    for B in sizes:
        row = dict(B=B, particles=n, steps=a.steps, loop="device", route="device_truth", reps=max(1, a.reps), max_est=a.capacity,
                   filter="mhfastslam" if a.mhfastslam else ("fastslam" if a.fastslam else "rbphd"))
        for name, est, particles in variants:
            figs, reads = [], []
            for rep in range(max(1, a.reps)):
                batch, run = make(B, est, particles)
                t0 = time.perf_counter()
                run.run(2, a.steps + 2)            # one call: the loop over steps is the library's
                batch.synchronize()
                t1 = time.perf_counter()
                figs.append(B * a.steps / (t1 - t0))
                if est:
                    trace = run.estimates()        # the one read of the whole log (timed apart: it grows with max_est and slots, not with the run)
                    reads.append(time.perf_counter() - t1)
                    row["estimate_log_mib_" + name] = sum(x.nbytes for x in trace if x is not None) / 2 ** 20
                    row["estimate_log_read_s_" + name] = float(np.median(reads))
                if particles and a.log_dir and B == max(sizes) and rep == max(1, a.reps) - 1:
                    for b in range(B):
                        sim.write_run_logs(os.path.join(a.log_dir, "filter_%03d" % b), b, trace, dict(batch.get_truth(b), dt=Ps[b]["dt"]), precision=17)
                    row["log_dir"] = a.log_dir
                batch.close()
            key = "filter_steps_per_s_estimates_" + name
            row[key], row[key + "_reps"] = float(np.median(figs)), figs
        # the host route: the per-step form of the same run, stopped after every step for the getters
        batch, run = make(B, False, False)
        if a.mhfastslam:
            batch.serve_metrics(True)
        t0 = time.perf_counter()
        for k in range(2, a.steps + 2):
            run.step(k)
            host_route_estimates(batch, B, thr)
        row["filter_steps_per_s_host_route"] = B * a.steps / (time.perf_counter() - t0)
        batch.close()
        for name, _, _ in variants[1:]:
            row[name + "_over_off"] = row["filter_steps_per_s_estimates_" + name] / row["filter_steps_per_s_estimates_off"]
            row[name + "_over_host_route"] = row["filter_steps_per_s_estimates_" + name] / row["filter_steps_per_s_host_route"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return rows


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
    ap.add_argument("--device-sensor", action="store_true", help="the device loop with host-made scans against device-made scans (rfsgpu_batch_sense_async): setup and run time of each")
    ap.add_argument("--device-truth", action="store_true", help="the device loop with device scans on a host-made ground truth against a device-made one run in one call (rfsgpu_batch_generate_truth, rfsgpu_batch_run_truth_async)")
    ap.add_argument("--fastslam", action="store_true", help="FastSLAM filters: a FastSLAMBatch against FastSLAM handles stepped in turn")
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions of every batch figure")
    ap.add_argument("--mhfastslam", action="store_true", help="multi-hypothesis FastSLAM filters: an MHFastSLAMBatch against handles on the device cycle stepped in turn")
    ap.add_argument("--results", default="", help="--errors: write one line per filter of the largest batch, 'Pd  c  posError  mapError' (the final row's pose_ed and cola)")
    ap.add_argument("--estimates", action="store_true", help="--device-truth: the one-call run with the device-side estimate log off / on (/ on with particles), and the per-step host route to the same data")
    ap.add_argument("--log-particles", action="store_true", help="--estimates: also time the log with the particle planes")
    ap.add_argument("--log-dir", default="", help="--estimates: write the largest batch's run as DIR/filter_NNN/{gtPose,gtLandmark,deadReckoning,particlePose,landmarkEst}.dat (tools/analysis2d_sim.py reads them)")
    ap.add_argument("--max-per-filter", type=int, default=0, help="--mhfastslam: particle slots per filter (default nParticlesMax x hypotheses = 9 x particles, which cannot overflow; at most 2048)")
    a = ap.parse_args()
    a.all_routes = a.device_truth and a.device_sensor      # both given: host-made scans, device-made scans and device-made truth in one line
    if a.device_truth:
        a.device_loop = a.device_sensor = True
    pkg = load_pkg()
    if a.estimates:
        if not a.device_truth:
            ap.error("--estimates times the one-call run: give --device-truth")
        if not a.mhfastslam:
            a.particles = a.particles or 200
        return estimates_sweep(pkg, a, [int(s) for s in a.sizes.split(",")])
    if a.mhfastslam and a.device_sensor:
        return sensor_sweep(pkg, a, [int(s) for s in a.sizes.split(",")])
    if a.mhfastslam:
        return mh_sweep(pkg, a, [int(s) for s in a.sizes.split(",")])
    a.particles = a.particles or 200
    sim = pkg.sim2d_driver
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.device_sensor:
        return sensor_sweep(pkg, a, sizes)
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
